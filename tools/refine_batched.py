'''
Solve a seeded batch of racelines on the device, refine it (raceline/refine.py: replay, select the columns
whose replayed position error exceeds --pos-tol, transfer them to the finer mesh, warm re-solve, replay
again), and print the replay quantiles before and after, by solver status.

The batch is bench.py's config 3 (--track race: seeded cold starts of the racetrack 50 x 4 drone).

    python tools/refine_batched.py [--track race] [--pose esp] [--batch 512] [--factor 2] [--K-dst 4]
                                   [--pos-tol 0.05] [--select replay] [--max-iter 1000]
'''
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

QUANTILES = (0.5, 0.9, 0.99, 1.0)
ERRORS = (('pos_err', 'm'), ('att_err', 'rad'), ('vel_err', 'm/s'), ('rate_err', 'rad/s'))


def by_group(rep, groups, cols=None):
    ''' {group: {instances, nonfinite, replay_errors: {error: {quantile: value}}}}: quantiles on the host over the
    columns `cols` of the replay (default all) whose four errors are all finite; the others are counted '''
    groups = np.array(groups)
    err = {name: getattr(rep, name).cpu().numpy() for name, _ in ERRORS}
    if cols is not None:
        err = {k: v[cols] for k, v in err.items()}
    finite = np.all([np.isfinite(v) for v in err.values()], axis=0)
    out = {}
    for g in sorted(set(groups)):
        m = groups == g
        rec = {'instances': int(m.sum()), 'nonfinite': int((m & ~finite).sum()), 'replay_errors': {}}
        if (m & finite).any():
            for name, unit in ERRORS:
                q = np.quantile(err[name][m & finite], QUANTILES)
                rec['replay_errors'][f'{name} [{unit}]'] = {('max' if p == 1.0 else f'q{int(round(p * 100))}'): float(x)
                                                           for p, x in zip(QUANTILES, q)}
        out[str(g)] = rec
    return out


def show(title, table):
    print(f'=== {title}')
    for s, rec in table.items():
        print(f'--- {s}: {rec["instances"]} instances, {rec["nonfinite"]} of them with a non-finite error (left out)')
        for name, v in rec['replay_errors'].items():
            print(f'  {name:18s} ' + '  '.join(f'{k} {x:.3e}' for k, x in v.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--track', choices=['race'], default='race')
    ap.add_argument('--pose', choices=['esp', 'dcm'], default='esp')
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--factor', type=int, default=2)
    ap.add_argument('--K-dst', type=int, default=None)
    ap.add_argument('--select', choices=['replay', 'all'], default='replay')
    ap.add_argument('--pos-tol', type=float, default=0.05)
    ap.add_argument('--max-iter', type=int, default=1000)
    ap.add_argument('--tol', type=float, default=1e-8)
    ap.add_argument('--substeps', type=int, default=16)
    ap.add_argument('-N', type=int, default=50)
    ap.add_argument('-K', type=int, default=4)
    ap.add_argument('--progress', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from aircraft_trajectory_optimization_amd.raceline.batched_solve import solve_shard
    from aircraft_trajectory_optimization_amd.raceline.refine import refine_solutions
    from aircraft_trajectory_optimization_amd.solver.ipm import IPMOptions
    from aircraft_trajectory_optimization_amd.tracks import make_spec
    dev = torch.device('cuda', torch.cuda.current_device())
    spec = make_spec(track=a.track, model='drone', frame='parametric', N=a.N, K=a.K, use_quat=True, global_r=True,
                     use_dcm=a.pose == 'dcm')
    opts = IPMOptions(max_iter=a.max_iter, tol=a.tol)
    t0 = time.perf_counter()
    res, _, _ = solve_shard(spec, list(range(a.batch)), opts, progress=a.progress)
    torch.cuda.synchronize(dev)
    t_solve = time.perf_counter() - t0
    t0 = time.perf_counter()
    ref = refine_solutions(spec, res.x, factor=a.factor, K=a.K_dst, select=a.select, pos_tol=a.pos_tol,
                           options=opts, substeps=a.substeps)
    torch.cuda.synchronize(dev)
    t_refine = time.perf_counter() - t0
    coarse = np.array([str(s) for s in res.status])
    out = {'workload': f'{a.track}_parametric_{a.pose}_drone_colloc_N{spec.N}_K{spec.K} -> N{ref.spec.N}_K{ref.spec.K} '
                       'batched solve + refinement',
           'batch': a.batch, 'tol': a.tol, 'max_iter': a.max_iter, 'substeps': a.substeps, 'select': a.select,
           'pos_tol': a.pos_tol, 'solve_s': t_solve, 'refine_s': t_refine, 'selected': int(len(ref.cols)),
           'coarse_statuses': {str(s): int((coarse == s).sum()) for s in sorted(set(coarse))},
           'selected_by_coarse_status': {str(s): int((coarse[ref.cols] == s).sum()) for s in sorted(set(coarse))},
           'before_all': by_group(ref.before, coarse)}
    show(f'coarse solve, all {a.batch} columns, by coarse status', out['before_all'])
    print(f'selected {len(ref.cols)} of {a.batch} columns (pos_err > {a.pos_tol} m or not finite): '
          f'{out["selected_by_coarse_status"]}')
    if len(ref.cols):
        fine = np.array([str(s) for s in ref.status])
        it = np.asarray(ref.iters)
        out['refined_statuses'] = {str(s): int((fine == s).sum()) for s in sorted(set(fine))}
        out['refined_iterations'] = {str(s): {'min': int(it[fine == s].min()), 'median': float(np.median(it[fine == s])),
                                         'max': int(it[fine == s].max())} for s in sorted(set(fine))}
        trans = np.array([f'{c} -> {f}' for c, f in zip(coarse[ref.cols], fine)])
        out['status_transitions'] = {str(t): int((trans == t).sum()) for t in sorted(set(trans))}
        out['before_selected'] = by_group(ref.before, trans, ref.cols)
        out['after_selected'] = by_group(ref.after, trans)
        pb, pa = ref.before.pos_err.cpu().numpy()[ref.cols], ref.after.pos_err.cpu().numpy()
        better = ~(pa >= pb) & np.isfinite(pa)           # smaller than before, or finite where it was not
        out['pos_err_improved'] = {str(t): int(better[trans == t].sum()) for t in sorted(set(trans))}
        out['sound_after'] = {str(t): int((pa[trans == t] <= a.pos_tol).sum()) for t in sorted(set(trans))}
        print(f're-solve statuses {out["refined_statuses"]}, iterations {out["refined_iterations"]}')
        print(f'transitions {out["status_transitions"]}; position error smaller after: {out["pos_err_improved"]}; '
              f'within pos_tol after: {out["sound_after"]}')
        show('selected columns before, by coarse status -> status of the re-solve', out['before_selected'])
        show('selected columns after, by coarse status -> status of the re-solve', out['after_selected'])
    print(json.dumps(out), flush=True)
    if a.out:
        json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
