''' the library exports the clearance entry points (no compute calls: no GPU here) '''
from aircraft_trajectory_optimization_amd import native


def test_library_exports_the_clearance_symbols():
    lib = native.load()
    for name in ('ato_mesh_signed_distance_strided', 'ato_clearance_set_line', 'ato_clearance'):
        assert hasattr(lib, name) and name in native.EXPORTED_SYMBOLS, name
