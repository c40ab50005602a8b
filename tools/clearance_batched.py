'''
Solve config 4 (the obstacle drone raceline over a batch of perturbed planning tubes,
raceline/obstacle_batch.py) and audit every solution against the arena mesh (raceline/clearance.py): how
many instances pass the reference's own test at the collocation nodes (samples 0), how many pass and how many
are certified at --samples points per interval, the same for the trajectory the vehicle ODE flies (--flown),
and the worst distance with its location.

    python tools/clearance_batched.py [--batch 512] [--samples 16] [--flown] [--max-iter 1000] [--out f.json]
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


def summary(r, mask):
    ''' counts and the worst instance of a ClearanceResult over the instances of mask '''
    idx = np.flatnonzero(mask)
    d_min = r.d_min.cpu().numpy()[idx]
    w = int(idx[d_min.argmin()]) if len(idx) else -1
    where = r.where.cpu().numpy()
    return {'instances': int(len(idx)), 'passed': int(r.passed.cpu().numpy()[idx].sum()),
            'certified': int(r.certified.cpu().numpy()[idx].sum()),
            'worst_d_min': float(d_min.min()) if len(idx) else None, 'worst_instance': w,
            'worst_interval': int(where[w, 0]) if w >= 0 else None, 'worst_sample': int(where[w, 1]) if w >= 0 else None,
            'median_d_min': float(np.median(d_min)) if len(idx) else None,
            'max_gap': float(r.gap.cpu().numpy()[idx].max()) if len(idx) else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--flown', action='store_true', help='also audit the replayed (flown) trajectory')
    ap.add_argument('--max-iter', type=int, default=1000)
    ap.add_argument('--progress', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from aircraft_trajectory_optimization_amd.obstacles.mesh_obstacle import MeshObstacle
    from aircraft_trajectory_optimization_amd.raceline.clearance import clearance_solutions
    from aircraft_trajectory_optimization_amd.raceline.obstacle_batch import config4_problem, solve_config4_shard
    from aircraft_trajectory_optimization_amd.raceline.problem import ProblemSpec
    from aircraft_trajectory_optimization_amd.solver.ipm import IPMOptions
    prob = config4_problem()
    t0 = time.perf_counter()
    res = solve_config4_shard(range(a.batch), IPMOptions(max_iter=a.max_iter), prob=prob, progress=a.progress)
    t_solve = time.perf_counter() - t0
    # positions depend on the discretisation alone: one spec serves both closure signs
    spec = ProblemSpec(prob['line'], prob['cfg'].copy(), prob['dveh'], 'parametric', sphere_table=prob['table'])
    mesh = MeshObstacle()
    X = torch.as_tensor(res['x'], device=mesh.device)
    r_c = prob['dveh'].collision_radius
    status = np.array(res['status'])
    optimal = status == 'optimal'
    out = {'workload': f'config 4: obstacle drone raceline N{spec.N} K{spec.K}, perturbed tubes, solve + clearance',
           'batch': a.batch, 'collision_radius': r_c, 'solve_s': t_solve,
           'statuses': {s: int((status == s).sum()) for s in sorted(set(res['status']))}, 'audits': {}}
    audits = [('nodes (samples 0)', dict(samples=0)), (f'samples {a.samples}', dict(samples=a.samples))]
    if a.flown:
        audits.append((f'flown, {a.samples} substeps', dict(samples=a.samples, flown=True)))
    for name, kw in audits:
        t0 = time.perf_counter()
        r = clearance_solutions(spec, X, mesh, collision_radius=r_c, **kw)
        torch.cuda.synchronize()
        out['audits'][name] = {'seconds_with_setup': time.perf_counter() - t0, 'all': summary(r, np.ones(a.batch, bool)),
                               'optimal': summary(r, optimal)}
        s = out['audits'][name]['optimal']
        print(f'--- {name}: of {s["instances"]} optimal instances {s["passed"]} pass, {s["certified"]} are certified '
              f'at r_c = {r_c} m; worst d_min {s["worst_d_min"]:.4f} m (instance {s["worst_instance"]}, interval '
              f'{s["worst_interval"]}, sample {s["worst_sample"]}), median d_min {s["median_d_min"]:.4f} m, longest '
              f'chord {s["max_gap"]:.4f} m')
    print(json.dumps(out), flush=True)
    if a.out:
        json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
