'''
Time the three launches of the gate-passage check (ato_gatecheck: the clearance's positions, k_gate_cross,
k_gate_reduce) with HIP events, each launch alone (ato_gatecheck_launches) and the whole call, at two shapes of
the 50 x 4 collocation on the race track (7 square gates): B = 512 of the parametric ESP drone (config 3's shape)
and B = 8192 of the parametric DCM drone, both at samples = 16; in the same run, ato_clearance's positions alone at
the same shape (the same kernel into a caller's buffer). Inputs are the cold start replicated with a small seeded
perturbation of every node variable. Warm-up first; every figure is the time per launch of 50 back-to-back launches
between one pair of events, the median over --reps such pairs;
everything in one process on one device. A launch that runs alone reads what the whole call before it left in the
handle's buffers, so it does the same work. The byte model is what the algorithm must move: positions read the
node block once and write 3 N S1 B doubles; the crossings read those positions once per gate and write G N 7 B
record doubles; the reduction reads the records and N step sizes per (gate, instance) and writes 9 G B doubles.

    python tools/bench_gatecheck.py [--reps 20] [--samples 16] [--out f.json]
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
INNER = 50              # launches per event pair
PEAK = 8.0e12
GATE_PART = 7           # doubles per partial record (csrc/ato_gatecheck.hpp)


def timed(fn, reps, st):
    ''' ms per launch: every event pair spans INNER back-to-back launches on the stream, so that a 16 us kernel is
    timed over about a millisecond of work and not over one launch's overhead and the events' resolution; the figure
    still includes the gap between two launches of one stream '''
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


def time_shape(name, B, samples, reps, **kw):
    from aircraft_trajectory_optimization_amd import native
    from aircraft_trajectory_optimization_amd.raceline.batched import BatchedNLP
    from aircraft_trajectory_optimization_amd.tracks import make_spec
    spec = make_spec(track='race', N=50, K=4, frame='parametric', global_r=True, **kw)
    rng = np.random.default_rng(0)
    W = np.repeat(np.array(spec.w0)[None], B, axis=0)
    W[:, spec.N:spec.N + spec.P * spec.nv] += 0.02 * rng.standard_normal((B, spec.P * spec.nv))
    nlp = BatchedNLP(spec, B, buffers=False)
    X = torch.as_tensor(np.ascontiguousarray(W.T), device=nlp.device)
    st = torch.cuda.current_stream(nlp.device)
    val = nlp.gatecheck(X, samples=samples)                    # line table, weight table, buffers, first launches
    pos, _ = nlp.clearance(None, X, samples=samples)
    torch.cuda.synchronize()
    G, N, S1 = len(spec.gates), spec.N, samples + 1
    prob = nlp.problem

    def launches(mask):
        rc = prob.gatecheck_rc(B, X.data_ptr(), samples, val.data_ptr(), 1e-6, stream=st.cuda_stream, launches=mask)
        assert rc == 0, rc

    t = {'positions': timed(lambda: launches(1), reps, st), 'cross': timed(lambda: launches(2), reps, st),
         'reduce': timed(lambda: launches(4), reps, st), 'whole_call': timed(lambda: launches(7), reps, st),
         'clearance_positions': timed(lambda: prob.clearance_ptrs(B, X.data_ptr(), samples, pos.data_ptr(),
                                                                  stream=st.cuda_stream), reps, st)}
    nbytes = {'positions': 8 * (spec.P * 3 + 3 * N * S1) * B, 'cross': 8 * (3 * N * S1 + N) * B * G + 8 * G * N * GATE_PART * B,
              'reduce': 8 * (G * N * GATE_PART + G * N + native.ATO_GATECHECK_NCH * G) * B}
    out = {'shape': name, 'batch': B, 'N': N, 'K': spec.K, 'gates': G, 'samples': samples, 'reps': reps,
           'launches_per_event_pair': INNER, 'items_cross': G * N * B, 'crossings_found': float(val[0].sum()), 'ms': t, 'bytes': nbytes}
    out['GBps'] = {k: nbytes[k] / (t[k]['ms_median'] * 1e-3) / 1e9 for k in nbytes}
    out['share_of_8TBps'] = {k: nbytes[k] / (t[k]['ms_median'] * 1e-3) / PEAK for k in nbytes}
    ref = t['clearance_positions']['ms_median']
    out['ratio_to_clearance_positions'] = {k: t[k]['ms_median'] / ref for k in ('positions', 'cross', 'reduce',
                                                                                  'whole_call')}
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
        print(f"{r['shape']}: {r['gates']} gates, {r['items_cross']} (gate, interval, instance) items, "
              f"{r['crossings_found']:.0f} crossings")
        for k, v in r['ms'].items():
            extra = (f", {r['bytes'][k] / 1e6:.1f} MB, {r['GBps'][k]:.0f} GB/s = {100 * r['share_of_8TBps'][k]:.1f} % "
                     f"of 8 TB/s") if k in r['bytes'] else ''
            ratio = r['ratio_to_clearance_positions'].get(k)
            print(f"    {k}: {v['ms_median'] * 1e3:.1f} us median ({v['ms_min'] * 1e3:.1f} - {v['ms_max'] * 1e3:.1f})"
                  f"{extra}" + (f", {ratio:.2f} x the clearance's positions" if ratio is not None else ''))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
