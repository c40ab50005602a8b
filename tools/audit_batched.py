'''
Solve (or load) a batch of 50 x 4 parametric drone racelines and audit every solution between its nodes
(raceline/audit.py): how many instances pass every margin at the collocation nodes (samples 0) and at --samples
points per interval, how many pass at the nodes and fail between them per channel, the medians and maxima of the
four ODE defects at the nodes (the frozen-geometry error plus the solver's residual; node 0 of every interval,
where the NLP has no ODE row, is among them) and between them, the
columns worst in each channel, and the instances the replay passes and the audit fails, and the reverse.

--config 3: the seeded cold-start instances of the benchmark (raceline/instances.py); --config 5: a corridor
batch (raceline/batch_instances.corridor_batch: per-instance corridors whose half-width varies along the lap,
so the audit holds y to every instance's widest corridor, path_bounds(varying='outer')). --load f.npy: decision
vectors (B, nw) of --config's problem instead of a solve (e.g. x.npy of bench.py --dump-outputs).

    python tools/audit_batched.py [--config 3] [--batch 512] [--samples 16] [--max-iter 1000] [--load x.npy]
                                  [--pos-tol 0.05] [--out f.json]
'''
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(r):
    from aircraft_trajectory_optimization_amd.raceline.audit import DEFECTS, MARGINS
    m, d = r.margin.cpu().numpy(), r.defect.cpu().numpy()
    where = r.where.cpu().numpy()
    worst = np.where(np.isnan(m), -np.inf, m).argmin(0)
    return {'passed': int(r.passed.sum()),
            'failed_per_channel': {c: int((~(m[:, i] >= -r.tol)).sum()) for i, c in enumerate(MARGINS)},
            'worst_per_channel': {c: {'instance': int(worst[i]), 'margin': float(m[worst[i], i]),
                                      'interval': int(where[worst[i], i, 0]), 'sample': int(where[worst[i], i, 1])}
                                  for i, c in enumerate(MARGINS)},
            'defect_median': {c: float(np.nanmedian(d[:, i])) for i, c in enumerate(DEFECTS)},
            'defect_max': {c: float(np.nanmax(d[:, i])) for i, c in enumerate(DEFECTS)},
            'att_dev_max': float(np.nanmax(r.att_dev.cpu().numpy()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', type=int, choices=(3, 5), default=3)
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--max-iter', type=int, default=1000)
    ap.add_argument('--tol', type=float, default=1e-6, help='a margin passes at >= -tol (the solver holds bounds to its own)')
    ap.add_argument('--pos-tol', type=float, default=0.05, help='replay position error (m) that counts as flying')
    ap.add_argument('--load', default=None)
    ap.add_argument('--progress', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from aircraft_trajectory_optimization_amd.raceline.audit import MARGINS, audit_solutions
    from aircraft_trajectory_optimization_amd.raceline.replay import replay_solutions
    from aircraft_trajectory_optimization_amd.solver.ipm import IPMOptions
    from aircraft_trajectory_optimization_amd.tracks import make_spec
    opts = IPMOptions(max_iter=a.max_iter)
    status = None
    if a.config == 3:
        from aircraft_trajectory_optimization_amd.raceline.batched_solve import solve_shard
        from aircraft_trajectory_optimization_amd.raceline.instances import seeded_instances
        spec = make_spec(track='race', model='drone', use_quat=True, frame='parametric', global_r=True, N=50, K=4)
        _, LBW, UBW = seeded_instances(spec, range(a.batch))
        if a.load:
            X = np.load(a.load)[:a.batch]
        else:
            res, _, _ = solve_shard(spec, range(a.batch), opts, progress=a.progress)
            X, status = res.x, list(res.status)
    else:
        from aircraft_trajectory_optimization_amd.raceline.batch_instances import corridor_batch
        from aircraft_trajectory_optimization_amd.solver.batched_ipm import device_solver
        spec, W, LBW, UBW, _, _ = corridor_batch(a.batch, track='fig8', frame='parametric', N=50, K=4, use_quat=True,
                                                 global_r=True, use_dcm=True, progress=a.progress)
        if a.load:
            X = np.load(a.load)[:a.batch]
        else:
            res = device_solver(spec, a.batch, LBW, UBW, opts).solve(W, progress=a.progress)
            X, status = res.x, list(res.status)
    out = {'config': a.config, 'batch': a.batch, 'N': spec.N, 'K': spec.K, 'samples': a.samples, 'tol': a.tol,
           'statuses': None if status is None else {s: status.count(s) for s in sorted(set(status))}}
    nodes = audit_solutions(spec, X, samples=0, LBW=LBW, UBW=UBW, tol=a.tol, varying='outer')
    dense = audit_solutions(spec, X, samples=a.samples, LBW=LBW, UBW=UBW, tol=a.tol, varying='outer')
    out['nodes'], out['dense'] = summary(nodes), summary(dense)
    mn, md = nodes.margin.cpu().numpy(), dense.margin.cpu().numpy()
    out['pass_at_nodes_fail_between'] = {c: int(((mn[:, i] >= -a.tol) & ~(md[:, i] >= -a.tol)).sum())
                                         for i, c in enumerate(MARGINS)}
    try:
        rep = replay_solutions(spec, X, substeps=a.samples)
        flies = (rep.pos_err <= a.pos_tol).cpu().numpy()
        ok = dense.passed.cpu().numpy()
        out['replay'] = {'pos_tol': a.pos_tol, 'fly': int(flies.sum()), 'fly_and_audit_fails': int((flies & ~ok).sum()),
                         'audit_passes_and_does_not_fly': int((ok & ~flies).sum())}
    except NotImplementedError as exc:
        out['replay'] = str(exc)
    print(f"--- of {a.batch} instances {out['nodes']['passed']} pass every margin at the nodes, "
          f"{out['dense']['passed']} at {a.samples} samples per interval (tol {a.tol})")
    print('    fail at the nodes, per channel:', out['nodes']['failed_per_channel'])
    print(f'    fail at {a.samples} samples, per channel:', out['dense']['failed_per_channel'])
    print('    pass at the nodes, fail between them:', out['pass_at_nodes_fail_between'])
    print('    defects at the nodes, median / max:', out['nodes']['defect_median'], out['nodes']['defect_max'])
    print('    defects between, median / max:', out['dense']['defect_median'], out['dense']['defect_max'])
    print('    replay:', out['replay'])
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
    torch.cuda.synchronize()


if __name__ == '__main__':
    main()
