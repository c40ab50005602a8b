'''
Time ato_replay with HIP events around the call, at config 3's shape (racetrack, ESP, B = 512) and
config 5's (fig-8, DCM, B = 8192): N = 50, K = 4, parametric, 16 substeps, seeded instances as w.

    python tools/bench_replay.py [--reps 20] [--substeps 16] [--out f.json]
'''
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_shape(track, pose, B, S, reps, trajectory):
    from aircraft_trajectory_optimization_amd.raceline.batched import BatchedNLP
    from aircraft_trajectory_optimization_amd.raceline.instances import seeded_instances
    from aircraft_trajectory_optimization_amd.tracks import make_spec
    spec = make_spec(track=track, model='drone', frame='parametric', N=50, K=4, use_quat=True, global_r=True,
                     use_dcm=pose == 'dcm')
    W, _, _ = seeded_instances(spec, list(range(B)))
    nlp = BatchedNLP(spec, B, buffers=False)
    X = torch.as_tensor(np.ascontiguousarray(np.asarray(W).T), device=nlp.device)
    nlp.replay(X, substeps=S)                      # lift and weight tables, first launch
    opts = {'device': nlp.device, 'dtype': torch.float64}
    zs, er = torch.empty((spec.N, spec.nz, B), **opts), torch.empty((spec.N, 4, B), **opts)
    tj = torch.empty((spec.N, S, spec.nz, B), **opts) if trajectory else None
    st = torch.cuda.current_stream(nlp.device)
    ms = []
    for i in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        nlp.problem.replay_ptrs(B, X.data_ptr(), S, zs.data_ptr(), er.data_ptr(), tj.data_ptr() if trajectory else 0,
                                stream=st.cuda_stream)
        e1.record(st)
        e1.synchronize()
        if i >= 3:
            ms.append(e0.elapsed_time(e1))
    return {'track': track, 'pose': pose, 'batch': B, 'N': spec.N, 'K': spec.K, 'substeps': S,
            'trajectory': trajectory, 'reps': reps, 'ms_median': float(np.median(ms)), 'ms_min': float(np.min(ms)),
            'ms_max': float(np.max(ms)), 'model_evaluations': int(B) * spec.N * S * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--substeps', type=int, default=16)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    out = []
    for track, pose, B in (('race', 'esp', 512), ('fig8', 'dcm', 8192)):
        for trajectory in (False, True):
            r = time_shape(track, pose, B, a.substeps, a.reps, trajectory)
            print(json.dumps(r), flush=True)
            out.append(r)
    if a.out:
        json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
