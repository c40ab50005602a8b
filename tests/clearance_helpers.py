'''
Clearance test fixtures: the CPU twin of the clearance kernels (tests/native/clearance_hostcheck.cpp), the
cases the CPU and the GPU tests share, their inputs, meshes and point sets.
'''
import ctypes
import functools
import os

import numpy as np

from aircraft_trajectory_optimization_amd import native
from tests import clearance_oracle
from tests.helpers import REPO, build_twin, n_points, product_spec, rel_dev  # noqa: F401
from tests.replay_helpers import MODELS, replay_inputs

CLEAR_SRC = os.path.join(REPO, 'tests', 'native', 'clearance_hostcheck.cpp')
CLEAR_LIB = os.path.join(REPO, 'tests', 'native', 'libato_clearancecheck.so')

# Twin / device positions against the numpy oracle (line.p2x), relative to max(1, |value|), over every case
# below with its three input sets, both layouts and samples 0, 1, 5. Measured once on the CPU twin: POS_MEASURED
# (the twin evaluates the cubics by Horner steps and every sum by fused multiply-adds, numpy rounds every
# product and power); the bound is 10 x that (it may not exceed 1e-9).
POS_MEASURED = 3.4084e-14
POS_TOL = 10 * POS_MEASURED
# Twin / device distances against oracle.ref_mesh, relative to max(1, |value|), over the point sets below on
# the box, the two lattices and the GPU test's 198 arena points. Measured once on the CPU twin: DIST_MEASURED (the
# largest on the arena points; 2.1467e-16 on the lattices); the bound is 10 x that (<= 1e-9).
DIST_MEASURED = 3.3307e-16
DIST_TOL = 10 * DIST_MEASURED

FRAMES = {'global': dict(frame='global', N=7), 'parametric': dict(frame='parametric', N=3, global_r=True),
          'relative': dict(frame='parametric', N=3, global_r=False)}
TRACKS = ('race', 'obstacles')
SAMPLES = (0, 1, 5)
CASES = [(t, m, f, K) for t in TRACKS for m in MODELS for f in FRAMES for K in (1, 2, 9)]
IL, IM = native.ATO_LAYOUT_INTERLEAVED, native.ATO_LAYOUT_INSTANCE_MAJOR


def case_id(c):
    return f'{c[0]}-{c[1]}-{c[2]}-K{c[3]}'


def build_clearancecheck(force=False):
    return build_twin(CLEAR_SRC, CLEAR_LIB, ('ato_sample.hpp', 'ato_clearance.hpp', 'ato_mesh_pair.hpp'), force)


@functools.lru_cache(maxsize=None)
def _lib():
    lib = ctypes.CDLL(build_clearancecheck())
    vp, ci, cl = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    lib.atoc_create.argtypes = [ctypes.POINTER(native.AtoProblemDesc), ctypes.POINTER(vp)]
    lib.atoc_last_error.restype = ctypes.c_char_p
    lib.atoc_destroy.argtypes = [vp]
    lib.atoc_set_line.argtypes = [vp, ctypes.POINTER(native.AtoLineTable)]
    lib.atoc_weights.argtypes = [vp, ci, vp]
    lib.atoc_clearance.argtypes = [vp, ci, ci, vp, ci, vp]
    lib.atoc_mesh_create.argtypes = [vp, ci, vp, ci, ctypes.POINTER(vp)]
    lib.atoc_mesh_destroy.argtypes = [vp]
    lib.atoc_mesh_tiles.argtypes = [vp]
    lib.atoc_mesh_sdist.argtypes = [vp, cl, vp, vp]
    lib.atoc_mesh_sdist_strided.argtypes = [vp, cl, vp, cl, cl, vp, ci, vp]
    return lib


class ClearanceTwin:
    ''' the positions of ato_clearance on host arrays (CPU build of csrc/ato_clearance.hpp) '''

    def __init__(self, spec, set_line=True):
        self.lib, self.spec = _lib(), spec
        self.holder = native.DescHolder(spec.native_spec())
        h = ctypes.c_void_p()
        if self.lib.atoc_create(ctypes.byref(self.holder.desc), ctypes.byref(h)) != 0:
            raise RuntimeError(self.lib.atoc_last_error().decode())
        self.h = h
        if set_line and spec.param and not spec.rk4:
            t, self._keep = native.line_table_struct(spec.line_table())
            self.lib.atoc_set_line(self.h, ctypes.byref(t))

    def __del__(self):
        try:
            self.lib.atoc_destroy(self.h)
        except Exception:  # pylint: disable=broad-except
            pass

    def last_error(self):
        return self.lib.atoc_last_error().decode()

    def weights(self, samples):
        wt = np.zeros((n_points(self.spec, samples), self.spec.K1))
        self.lib.atoc_weights(self.h, samples, wt.ctypes.data)
        return wt

    def raw(self, W, samples, layout=IL, batch=None, fill=0.0):
        '''
        W (B, nw) -> (rc, pos in the library's own layout: (3, N, S1, B) interleaved, (B, N, S1, 3)
        instance-major), the output starting from `fill`. batch: the batch argument where it shall differ.
        '''
        sp_ = self.spec
        W = np.ascontiguousarray(np.atleast_2d(W), np.float64)
        B = W.shape[0]
        il = layout == IL
        S1 = n_points(sp_, min(max(int(samples), 0), 64))
        pos = np.full((3, sp_.N, S1, B) if il else (B, sp_.N, S1, 3), fill)
        win = np.ascontiguousarray(W.T) if il else W
        rc = self.lib.atoc_clearance(self.h, B if batch is None else batch, layout, win.ctypes.data, int(samples),
                                     pos.ctypes.data)
        return rc, pos

    def positions(self, W, samples, layout=IL):
        ''' W (B, nw) -> (B, N, S1, 3) '''
        rc, pos = self.raw(W, samples, layout)
        if rc != 0:
            raise RuntimeError(f'twin clearance error {rc}: {self.last_error()}')
        return np.ascontiguousarray(np.moveaxis(pos, (0, 3), (3, 0))) if layout == IL else pos


class MeshTwin:
    ''' the tiles of ato_mesh_create and both distance kernels on host arrays '''

    def __init__(self, V, F):
        self.lib = _lib()
        self.V, self.F = np.ascontiguousarray(V, np.float64), np.ascontiguousarray(F, np.int32)
        h = ctypes.c_void_p()
        if self.lib.atoc_mesh_create(self.V.ctypes.data, len(self.V), self.F.ctypes.data, len(self.F),
                                     ctypes.byref(h)) != 0:
            raise RuntimeError('twin mesh: bad faces')
        self.h = h
        self.tiles = self.lib.atoc_mesh_tiles(h)

    def __del__(self):
        try:
            self.lib.atoc_mesh_destroy(self.h)
        except Exception:  # pylint: disable=broad-except
            pass

    def sdist(self, X):
        ''' brute force in face order (k_mesh_sdist): X (n, 3) -> (n,) '''
        X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
        d = np.zeros(len(X))
        self.lib.atoc_mesh_sdist(self.h, len(X), X.ctypes.data, d.ctypes.data)
        return d

    def sdist_strided(self, A, n, stride_point, stride_comp, cull):
        ''' tiled (k_mesh_sdist_tiles) on the flat array A -> (dist (n,), (wave-tile pairs, distance passes
        skipped, crossing passes skipped)) '''
        A = np.ascontiguousarray(A, np.float64).reshape(-1)
        assert (n - 1) * stride_point + 2 * stride_comp < A.size
        d = np.zeros(n)
        counts = (ctypes.c_long * 3)()
        self.lib.atoc_mesh_sdist_strided(self.h, n, A.ctypes.data, stride_point, stride_comp, d.ctypes.data,
                                         int(cull), counts)
        return d, tuple(counts)


@functools.lru_cache(maxsize=None)
def case_spec(track, model, frame, K):
    return product_spec(track=track, K=K, **{**MODELS[model], **FRAMES[frame]})


def node_s_view(spec, W):
    ''' view (B, N, K1) of the s (first state component) of every node of W (B, nw) '''
    return W[:, spec.N:spec.N + spec.P * spec.nv].reshape(W.shape[0], spec.N, spec.K1, spec.nv)[..., 0]


@functools.lru_cache(maxsize=None)
def case_inputs(track, model, frame, K, B=3):
    '''
    The three input sets of a case, each (B, nw): replay_inputs; the same with s pushed just outside
    [s_min, s_max] in the first and the last interval (the extrapolation pieces); the same with s exactly on
    knots of x_c and of r_y. The global frame has no s: its three sets are three seeds.
    '''
    spec = case_spec(track, model, frame, K)
    if not spec.param:
        sets = [replay_inputs(spec, B, seed) for seed in (0, 1, 2)]
    else:
        base = replay_inputs(spec, B, 0)
        out = base.copy()
        s = node_s_view(spec, out)
        rng = np.random.default_rng(5)
        s[:, 0, :] = spec.line.s_min() - 0.02 - 0.2 * rng.random(s[:, 0, :].shape)
        s[:, -1, :] = spec.line.s_max() + 0.02 + 0.2 * rng.random(s[:, -1, :].shape)
        knots = base.copy()
        s = node_s_view(spec, knots)
        kx, kr = spec.line._xc.knots, spec.line._ry.knots      # pylint: disable=protected-access
        pool = np.concatenate([kx, kr])
        s[...] = pool[np.random.default_rng(6).integers(0, len(pool), s.shape)]
        s[0, 0, 0], s[0, -1, -1] = kx[0], kx[-1]
        sets = [base, out, knots]
    for a in sets:
        a.setflags(write=False)
    return tuple(sets)


# ------------------------------------------------------------------ meshes and point sets
# the lattices stand in the volume the race track's trajectories cross
LATTICE = dict(pitch=(4.5, 4.0, 1.0), side=(1.5, 1.5, 0.5), origin=(-4.5, -6.0, 0.8))


@functools.lru_cache(maxsize=None)
def mesh(name):
    ''' 'box': one box, 12 triangles; 'lattice': 4 x 4 x 4 boxes, 768 triangles = 24 tiles; 'lattice63': 63
    boxes, 756 triangles, no multiple of the tile '''
    if name == 'box':
        V, F = clearance_oracle.box_mesh((-1.0, -0.5, 0.25), (1.5, 1.0, 1.75))
    else:
        V, F = clearance_oracle.lattice_mesh(64 if name == 'lattice' else 63, **LATTICE)
    V.setflags(write=False)
    F.setflags(write=False)
    return V, F


@functools.lru_cache(maxsize=None)
def random_points(name, n, seed):
    ''' n points uniform over twice the mesh's box, inside and outside the boxes '''
    V, _ = mesh(name)
    lo, hi = V.min(0), V.max(0)
    c, e = (lo + hi) / 2, (hi - lo)
    X = c + e * (np.random.default_rng(seed).random((n, 3)) - 0.5) * 2
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def oracle_distance(name, n, seed):
    ''' ref_mesh's signed distance of random_points(name, n, seed); computed once '''
    d = clearance_oracle.signed_distance(random_points(name, n, seed), *mesh(name))
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def coherent_batch(B=65, samples=5):
    ''' (spec, W (B, nw), twin positions (3, N, S1, B) in the interleaved layout) of the parametric point mass
    on the race track: consecutive points are one (interval, sample) of neighbouring instances '''
    spec = case_spec('race', 'point', 'parametric', 2)
    W = replay_inputs(spec, B, 3)
    rc, pos = ClearanceTwin(spec).raw(W, samples, IL)
    assert rc == 0
    W.setflags(write=False)
    pos.setflags(write=False)
    return spec, W, pos
