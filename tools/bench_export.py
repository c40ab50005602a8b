'''
Time the export of solved racelines (ato_export: k_export_tstart, k_export_sample, k_export_qchain) with HIP events
at five shapes of the 50 x 4 collocation on the race track, n_times = 1000 times in seconds over the lap: B = 512 of
the parametric point mass (lift only), of the global-frame and the parametric ESP drone (config 3's shape: lift and
sign pass) and of the parametric DCM drone (lift, polar factor, sign pass), and B = 8192 of the parametric DCM drone.
Inputs are the cold start replicated with a small seeded perturbation of every node variable. Warm-up first; every
figure is the time per call of INNER back-to-back calls between one pair of events, the median over --reps such
pairs; everything in one process on one device. The node table alone (start times, search, interpolation), the state
table alone (the default of BatchedNLP.export) and both; the differences between the shapes at one B are what the
lift, the sign pass and the polar factor cost, since the three kernels of a call are not timed apart. The byte model
is what the call must move at the least: the outputs, 8 (30 [+ NV]) n_times B bytes, written once (the sign pass reads and rewrites 4 of the 30 channels on top); the decision vectors
(8 nw B bytes, re-read per time through the caches) are left out, so the share of the peak is that of the outputs.

    python tools/bench_export.py [--reps 20] [--times 1000] [--out f.json]
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
INNER = 10              # calls per event pair
PEAK = 8.0e12


def timed(fn, reps, st):
    ''' ms per call: every event pair spans INNER back-to-back calls on the stream '''
    ms = []
    for i in range(reps + WARMUP):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(INNER):
            fn()
        e1.record(st)
        e1.synchronize()
        if i >= WARMUP:
            ms.append(e0.elapsed_time(e1) / INNER)
    return {'ms_median': float(np.median(ms)), 'ms_min': float(np.min(ms)), 'ms_max': float(np.max(ms))}


def time_shape(name, B, T, reps, **kw):
    from aircraft_trajectory_optimization_amd import native
    from aircraft_trajectory_optimization_amd.raceline.batched import BatchedNLP
    from aircraft_trajectory_optimization_amd.tracks import make_spec
    spec = make_spec(track='race', N=50, K=4, **kw)
    rng = np.random.default_rng(0)
    W = np.repeat(np.array(spec.w0)[None], B, axis=0)
    W[:, spec.N:spec.N + spec.P * spec.nv] += 0.02 * rng.standard_normal((B, spec.P * spec.nv))
    nlp = BatchedNLP(spec, B, buffers=False)
    X = torch.as_tensor(np.ascontiguousarray(W.T), device=nlp.device)
    times = torch.linspace(0.0, float(W[:, :spec.N].sum(1).max()), T, dtype=torch.float64, device=nlp.device)
    st = torch.cuda.current_stream(nlp.device)
    state, nodes = nlp.export(X, times=times, nodes=True)          # line table, scratch, first launches
    torch.cuda.synchronize()
    prob, nch = nlp.problem, native.ATO_EXPORT_NCH

    def call(with_state, with_nodes):
        prob.export_ptrs(B, X.data_ptr(), T, times.data_ptr(), False, nodes.data_ptr() if with_nodes else 0,
                         state.data_ptr() if with_state else 0, stream=st.cuda_stream)

    # nodes alone: start times, search and interpolation (no lift, no polar factor, no sign pass); across the shapes
    # at one B the state column adds the lift (point mass), the sign pass (ESP, global attitude) and the polar factor (DCM)
    modes = {'nodes': (False, True), 'state': (True, False), 'state_and_nodes': (True, True)}
    t = {k: timed(lambda m=m: call(*m), reps, st) for k, m in modes.items()}
    nbytes = {k: 8 * (nch * m[0] + spec.nv * m[1]) * T * B for k, m in modes.items()}
    out = {'shape': name, 'batch': B, 'N': spec.N, 'K': spec.K, 'n_times': T, 'reps': reps,
           'calls_per_event_pair': INNER, 'ms': t, 'bytes': nbytes,
           'finite_share_of_state': float(torch.isfinite(state).double().mean())}
    out['GBps'] = {k: nbytes[k] / (t[k]['ms_median'] * 1e-3) / 1e9 for k in nbytes}
    out['share_of_8TBps'] = {k: nbytes[k] / (t[k]['ms_median'] * 1e-3) / PEAK for k in nbytes}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--times', type=int, default=1000)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = [time_shape('point-parametric B=512', 512, a.times, a.reps, model='point', frame='parametric'),
           time_shape('esp-global B=512', 512, a.times, a.reps, model='drone', use_quat=True, frame='global'),
           time_shape('esp-parametric B=512', 512, a.times, a.reps, model='drone', use_quat=True, frame='parametric'),
           time_shape('dcm-parametric B=512', 512, a.times, a.reps, model='drone', use_dcm=True, frame='parametric'),
           time_shape('dcm-parametric B=8192', 8192, a.times, a.reps, model='drone', use_dcm=True, frame='parametric')]
    for r in res:
        print(f"{r['shape']}: {r['n_times']} times, {r['n_times'] * r['batch']} (time, instance) items")
        for k, v in r['ms'].items():
            print(f"    {k}: {v['ms_median'] * 1e3:.1f} us median ({v['ms_min'] * 1e3:.1f} - {v['ms_max'] * 1e3:.1f}), "
                  f"{r['bytes'][k] / 1e6:.1f} MB of outputs, {r['GBps'][k]:.0f} GB/s = "
                  f"{100 * r['share_of_8TBps'][k]:.1f} % of 8 TB/s")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
