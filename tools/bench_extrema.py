'''
Time the whole-interval extrema (ato_extrema) beside the between-node audit (ato_audit at samples = 16) on the same
inputs at two shapes of the 50 x 4 collocation: B = 512 of the parametric ESP drone on the race track (config 3's
shape) and B = 8192 of the parametric DCM drone on the fig-8. HIP events around 50 back-to-back launches, the time
per launch, the median of --reps such windows after 3 warm-up windows, one process on one device. Inputs are the
cold start replicated with a small seeded perturbation of every node variable (bench_audit.py's), so nearly every
polynomial has interior extrema; the visit count of the branch and bound depends on the data, the figure of a
solved batch is --batch-figure's. The flags the search left (visit cap) are counted.

--batch-figure: solve config 3's 512 seeded cold starts (raceline/instances.py, max_iter 1000) and print how many
columns extrema_solutions passes and certifies at --tol, the failing columns and the median overshoot per group,
the worst slack and the time of that one call.

    python tools/bench_extrema.py [--reps 20] [--batch-figure] [--tol 1e-6] [--out f.json]
'''
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, LAUNCHES = 3, 50


def timed(fn, reps, st):
    ''' time per launch (ms) over LAUNCHES back-to-back launches: median, min, max of reps windows '''
    ms = []
    for i in range(reps + WARMUP):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(LAUNCHES):
            fn()
        e1.record(st)
        e1.synchronize()
        if i >= WARMUP:
            ms.append(e0.elapsed_time(e1) / LAUNCHES)
    return {'ms_median': float(np.median(ms)), 'ms_min': float(np.min(ms)), 'ms_max': float(np.max(ms))}


def time_shape(name, B, reps, samples=16, **kw):
    from aircraft_trajectory_optimization_amd.raceline.audit import path_bounds
    from aircraft_trajectory_optimization_amd.raceline.batched import BatchedNLP
    from aircraft_trajectory_optimization_amd.tracks import make_spec
    spec = make_spec(N=50, K=4, frame='parametric', global_r=True, **kw)
    rng = np.random.default_rng(0)
    W = np.repeat(np.array(spec.w0)[None], B, axis=0)
    W[:, spec.N:spec.N + spec.P * spec.nv] += 0.02 * rng.standard_normal((B, spec.P * spec.nv))
    nlp = BatchedNLP(spec, B, buffers=False)
    X = torch.as_tensor(np.ascontiguousarray(W.T), device=nlp.device)
    lb, ub = (torch.as_tensor(v, device=nlp.device) for v in path_bounds(spec, varying='outer'))
    st = torch.cuda.current_stream(nlp.device)
    aval = nlp.audit(X, samples=samples, lb=lb, ub=ub)          # line table, weight tables, first launches
    val, _ = nlp.extrema(X)
    torch.cuda.synchronize()
    p = nlp.problem
    ext = timed(lambda: p.extrema_ptrs(B, X.data_ptr(), val.data_ptr(), stream=st.cuda_stream), reps, st)
    aud = timed(lambda: p.audit_ptrs(B, X.data_ptr(), samples, aval.data_ptr(), lb.data_ptr(), ub.data_ptr(),
                                     stream=st.cuda_stream), reps, st)
    flag = val[7]
    return {'shape': name, 'batch': B, 'N': spec.N, 'K': spec.K, 'nvx': int(val.shape[1]),
            'polynomials': int(val.shape[1]) * spec.N * B, 'reps': reps, 'launches': LAUNCHES, 'extrema': ext,
            'audit_s16': aud, 'ratio': ext['ms_median'] / aud['ms_median'], 'capped': int((flag == 1).sum()),
            'nonfinite': int(torch.isnan(flag).sum()),
            'slack_max_rel': float((val[6] / torch.maximum(val[0].abs(), val[3].abs()).clamp_min(1.0)).max())}


def batch_figure(tol, max_iter):
    from aircraft_trajectory_optimization_amd.raceline.audit import EXTREMA_GROUPS, extrema_solutions, path_bounds
    from aircraft_trajectory_optimization_amd.raceline.batched_solve import solve_shard
    from aircraft_trajectory_optimization_amd.raceline.instances import seeded_instances
    from aircraft_trajectory_optimization_amd.solver.ipm import IPMOptions
    from aircraft_trajectory_optimization_amd.tracks import make_spec
    B = 512
    spec = make_spec(track='race', model='drone', use_quat=True, frame='parametric', global_r=True, N=50, K=4)
    _, LBW, UBW = seeded_instances(spec, range(B))
    res, _, _ = solve_shard(spec, range(B), IPMOptions(max_iter=max_iter))
    status = list(res.status)
    lb, ub = path_bounds(spec, LBW, UBW, varying='outer')
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    extrema_solutions(spec, res.x, tol=tol, lb=lb, ub=ub)      # handle, table, first launch
    e0.record()
    r = extrema_solutions(spec, res.x, tol=tol, lb=lb, ub=ub)
    e1.record()
    e1.synchronize()
    m = r.margin.cpu().numpy()
    over = np.clip(-m[:, :7], 0.0, None)
    fails = ~(m >= -tol)
    return {'config': 3, 'batch': B, 'tol': tol, 'statuses': {s: status.count(s) for s in sorted(set(status))},
            'passed': int(r.passed.sum()), 'certified': int(r.certified.sum()),
            'failed_per_group': {g: int(fails[:, i].sum()) for i, g in enumerate(EXTREMA_GROUPS)},
            'median_overshoot_of_failing': {g: float(np.median(over[fails[:, i], i])) if fails[:, i].any() else 0.0
                                            for i, g in enumerate(EXTREMA_GROUPS)},
            'median_overshoot_all': {g: float(np.median(over[:, i])) for i, g in enumerate(EXTREMA_GROUPS)},
            'worst_margin': {g: float(np.nanmin(m[:, i])) for i, g in enumerate(EXTREMA_GROUPS)},
            'capped': int((r.val[7] == 1).sum()), 'nonfinite': int(torch.isnan(r.val[7]).sum()),
            'slack_max': float(r.val[6].max()), 'extrema_solutions_ms': float(e0.elapsed_time(e1))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch-figure', action='store_true')
    ap.add_argument('--tol', type=float, default=1e-6)
    ap.add_argument('--max-iter', type=int, default=1000)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = {'timing': [time_shape('race esp-parametric B=512', 512, a.reps, track='race', model='drone', use_quat=True),
                      time_shape('fig8 dcm-parametric B=8192', 8192, a.reps, track='fig8', model='drone',
                                 use_dcm=True)]}
    for r in res['timing']:
        e, d = r['extrema'], r['audit_s16']
        print(f"{r['shape']}: {r['polynomials']} polynomials, ato_extrema {e['ms_median'] * 1e3:.1f} us per call "
              f"({e['ms_min'] * 1e3:.1f} - {e['ms_max'] * 1e3:.1f}), ato_audit S=16 {d['ms_median'] * 1e3:.1f} us "
              f"({d['ms_min'] * 1e3:.1f} - {d['ms_max'] * 1e3:.1f}), ratio {r['ratio']:.1f}; capped {r['capped']}, "
              f"non-finite {r['nonfinite']}, largest slack / max(1, |extremum|) {r['slack_max_rel']:.2e}", flush=True)
    if a.batch_figure:
        f = res['batch_figure'] = batch_figure(a.tol, a.max_iter)
        print(f"--- config 3, {f['batch']} columns ({f['statuses']}), tol {f['tol']}: {f['passed']} pass, "
              f"{f['certified']} certified; capped {f['capped']}, non-finite {f['nonfinite']}, largest slack "
              f"{f['slack_max']:.2e}; extrema_solutions {f['extrema_solutions_ms']:.2f} ms")
        print('    failing columns per group:', f['failed_per_group'])
        print('    median overshoot of the failing columns:', f['median_overshoot_of_failing'])
        print('    median overshoot over all columns:', f['median_overshoot_all'])
        print('    worst margin:', f['worst_margin'], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    torch.cuda.synchronize()


if __name__ == '__main__':
    main()
