'''
Time ato_remesh with HIP events around the call, at config 3's shape (racetrack, ESP, B = 512) and
config 5's (fig-8, DCM, B = 8192): N = 50, K = 4, parametric, to N * r intervals of degree K', seeded
instances as w. Reports the bytes moved, (nw + nw') * 8 * B, against the 8 TB/s HBM peak.

    python tools/bench_remesh.py [--reps 20] [--factor 2] [--K 4] [--out f.json]
'''
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8e12          # bytes / s


def time_shape(track, pose, B, factor, Kd, reps, layout):
    from aircraft_trajectory_optimization_amd import native
    from aircraft_trajectory_optimization_amd.raceline.batched import BatchedNLP
    from aircraft_trajectory_optimization_amd.raceline.instances import seeded_instances
    from aircraft_trajectory_optimization_amd.raceline.refine import refined_spec
    from aircraft_trajectory_optimization_amd.tracks import make_spec
    spec = make_spec(track=track, model='drone', frame='parametric', N=50, K=4, use_quat=True, global_r=True,
                     use_dcm=pose == 'dcm')
    dspec = refined_spec(spec, factor, Kd)
    W, _, _ = seeded_instances(spec, list(range(B)))
    il = layout == native.ATO_LAYOUT_INTERLEAVED
    src = BatchedNLP(spec, B, layout=layout, buffers=False)
    dst = BatchedNLP(dspec, B, layout=layout, device=src.device, buffers=False)
    W = np.asarray(W, np.float64)
    X = torch.as_tensor(np.ascontiguousarray(W.T if il else W), device=src.device)
    out = dst.remesh_from(src, X)                  # weight table, first launch
    st = torch.cuda.current_stream(src.device)
    ms = []
    for i in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        dst.problem.remesh_ptrs(src.problem, B, B, X.data_ptr(), out.data_ptr(), layout=layout, stream=st.cuda_stream)
        e1.record(st)
        e1.synchronize()
        if i >= 3:
            ms.append(e0.elapsed_time(e1))
    nbytes = (spec.nw + dspec.nw) * 8 * B
    med = float(np.median(ms))
    return {'track': track, 'pose': pose, 'batch': B, 'N': spec.N, 'K': spec.K, 'N_dst': dspec.N, 'K_dst': dspec.K,
            'layout': 'interleaved' if il else 'instance_major', 'reps': reps, 'ms_median': med,
            'ms_min': float(np.min(ms)), 'ms_max': float(np.max(ms)), 'bytes': int(nbytes),
            'GBps': nbytes / (med * 1e-3) / 1e9, 'fraction_of_hbm_peak': nbytes / (med * 1e-3) / HBM_PEAK}


def main():
    from aircraft_trajectory_optimization_amd import native
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--factor', type=int, default=2)
    ap.add_argument('--K', type=int, default=4)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    out = []
    for track, pose, B in (('race', 'esp', 512), ('fig8', 'dcm', 8192)):
        for layout in (native.ATO_LAYOUT_INTERLEAVED, native.ATO_LAYOUT_INSTANCE_MAJOR):
            r = time_shape(track, pose, B, a.factor, a.K, a.reps, layout)
            print(json.dumps(r), flush=True)
            out.append(r)
    if a.out:
        json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
