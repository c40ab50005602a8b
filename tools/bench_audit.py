'''
Time the between-node audit kernel (ato_audit) with HIP events around each call at two shapes of the 50 x 4
collocation: B = 512 of the parametric ESP drone (config 3's shape) and B = 8192 of the parametric DCM drone, both
at samples = 16 with the problem's own bounds; inputs are the cold start replicated with a small seeded
perturbation of every node variable. Warm-up launches first, every figure the median over --reps launches,
everything in one process on one device. The byte model is what the algorithm must move: every decision-vector
element once (the re-reads by the other samples of an interval are cache hits) and every output once,
8 (nw + NCH N S1) B bytes; the share is of the 8 TB/s HBM peak.

    python tools/bench_audit.py [--reps 20] [--samples 16] [--out f.json]
'''
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP = 3
PEAK = 8.0e12


def timed(fn, reps, st):
    ms = []
    for i in range(reps + WARMUP):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        if i >= WARMUP:
            ms.append(e0.elapsed_time(e1))
    return {'ms_median': float(np.median(ms)), 'ms_min': float(np.min(ms)), 'ms_max': float(np.max(ms))}


def time_shape(name, B, samples, reps, **kw):
    from aircraft_trajectory_optimization_amd import native
    from aircraft_trajectory_optimization_amd.raceline.audit import path_bounds
    from aircraft_trajectory_optimization_amd.raceline.batched import BatchedNLP
    from aircraft_trajectory_optimization_amd.tracks import make_spec
    spec = make_spec(track='race', N=50, K=4, frame='parametric', global_r=True, **kw)
    rng = np.random.default_rng(0)
    W = np.repeat(np.array(spec.w0)[None], B, axis=0)
    W[:, spec.N:spec.N + spec.P * spec.nv] += 0.02 * rng.standard_normal((B, spec.P * spec.nv))
    nlp = BatchedNLP(spec, B, buffers=False)
    X = torch.as_tensor(np.ascontiguousarray(W.T), device=nlp.device)
    lb, ub = (torch.as_tensor(v, device=nlp.device) for v in path_bounds(spec))
    st = torch.cuda.current_stream(nlp.device)
    val = nlp.audit(X, samples=samples, lb=lb, ub=ub)           # line table, weight tables, first launch
    torch.cuda.synchronize()
    t = timed(lambda: nlp.problem.audit_ptrs(B, X.data_ptr(), samples, val.data_ptr(), lb.data_ptr(), ub.data_ptr(),
                                             stream=st.cuda_stream), reps, st)
    S1 = samples + 1
    nbytes = 8 * (spec.nw + native.ATO_AUDIT_NCH * spec.N * S1) * B
    out = {'shape': name, 'batch': B, 'N': spec.N, 'K': spec.K, 'samples': samples, 'items': spec.N * S1 * B,
           'reps': reps, 'bytes': nbytes, **t}
    out['GBps'] = nbytes / (t['ms_median'] * 1e-3) / 1e9
    out['share_of_8TBps'] = nbytes / (t['ms_median'] * 1e-3) / PEAK
    out['finite_share'] = float(torch.isfinite(val[9:]).double().mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = [time_shape('esp-parametric B=512', 512, a.samples, a.reps, model='drone', use_quat=True),
           time_shape('dcm-parametric B=8192', 8192, a.samples, a.reps, model='drone', use_dcm=True)]
    for r in res:
        print(f"{r['shape']}: {r['items']} items, {r['ms_median'] * 1e3:.1f} us median ({r['ms_min'] * 1e3:.1f} - "
              f"{r['ms_max'] * 1e3:.1f}), {r['bytes'] / 1e6:.1f} MB, {r['GBps']:.0f} GB/s = "
              f"{100 * r['share_of_8TBps']:.1f} % of 8 TB/s")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
