'''
Time the clearance kernels with HIP events around each call, at config 4's shape (the obstacle drone raceline,
N = 50, K = 4, samples 16: B = 512 is 435 k points) and at one large batch (B = 8192 of the same problem, 7 M
points); inputs are the problem's cold start replicated with a small seeded perturbation of every node's (y, n).
Per shape: the position kernel alone, then the signed distance to the arena mesh three ways on the same points:
ato_mesh_signed_distance (brute force through LDS, what the library had before; its [n][3] copy of the points is
made outside the timed region), and ato_mesh_signed_distance_strided with cull = 0 and cull = 1. Warm-up
launches first, every figure the median over --reps launches, everything in one process on one device.

    python tools/bench_clearance.py [--reps 20] [--big-reps 5] [--samples 16] [--out f.json]
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


def time_shape(prob, mesh, B, samples, reps):
    from aircraft_trajectory_optimization_amd.raceline.batched import BatchedNLP
    from aircraft_trajectory_optimization_amd.raceline.problem import ProblemSpec
    spec = ProblemSpec(prob['line'], prob['cfg'].copy(), prob['dveh'], 'parametric', sphere_table=prob['table'])
    rng = np.random.default_rng(0)
    W = np.repeat(np.array(spec.w0)[None], B, axis=0)
    nodes = W[:, spec.N:].reshape(B, spec.P, spec.nv)
    nodes[:, :, 1:3] += 0.05 * rng.standard_normal((B, spec.P, 2))
    nlp = BatchedNLP(spec, B, buffers=False)
    X = torch.as_tensor(np.ascontiguousarray(W.T), device=nlp.device)
    st = torch.cuda.current_stream(nlp.device)
    pos, dist = nlp.clearance(mesh, X, samples=samples, cull=True)       # line table, weights, first launches
    n = dist.numel()
    rows = pos.reshape(3, n).T.contiguous()
    d_old = torch.empty(n, dtype=torch.float64, device=nlp.device)
    out = {'batch': B, 'N': spec.N, 'K': spec.K, 'samples': samples, 'points': n, 'triangles': len(mesh.faces),
           'reps': reps}
    out['positions'] = timed(lambda: nlp.problem.clearance_ptrs(B, X.data_ptr(), samples, pos=pos.data_ptr(),
                                                                stream=st.cuda_stream), reps, st)
    # the bytes the algorithm needs: every source element once (its re-reads by the other samples of the interval
    # are cache hits) and every position written once
    nbytes = (3 * spec.P * B + 3 * n) * 8
    out['positions']['bytes'] = int(nbytes)
    out['positions']['GBps'] = nbytes / (out['positions']['ms_median'] * 1e-3) / 1e9
    out['distance_brute_force'] = timed(lambda: mesh.lib.ato_mesh_signed_distance(
        mesh.handle, n, rows.data_ptr(), d_old.data_ptr(), None, st.cuda_stream), reps, st)
    res = {}
    for name, cull in (('distance_strided_cull0', False), ('distance_strided_cull1', True)):
        d = torch.empty(n, dtype=torch.float64, device=nlp.device)
        out[name] = timed(lambda d=d, cull=cull: mesh.signed_distance_strided(pos, n, 1, n, cull=cull, out=d), reps, st)
        res[name] = d
    torch.cuda.synchronize()
    out['cull1_equals_cull0_bitwise'] = bool(torch.equal(res['distance_strided_cull0'], res['distance_strided_cull1']))
    out['strided_equals_brute_force_bitwise'] = bool(torch.equal(res['distance_strided_cull0'], d_old))
    out['max_abs_strided_minus_brute_force'] = float((res['distance_strided_cull0'] - d_old).abs().max())
    out['d_min'] = float(d_old.min())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--big-reps', type=int, default=5)
    ap.add_argument('--samples', type=int, default=16)
    ap.add_argument('--big-batch', type=int, default=8192)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from aircraft_trajectory_optimization_amd.obstacles.mesh_obstacle import MeshObstacle
    from aircraft_trajectory_optimization_amd.raceline.obstacle_batch import config4_problem
    prob = config4_problem()
    mesh = MeshObstacle()
    out = []
    for B, reps in ((512, a.reps), (a.big_batch, a.big_reps)):
        r = time_shape(prob, mesh, B, a.samples, reps)
        print(json.dumps(r), flush=True)
        out.append(r)
    if a.out:
        json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
