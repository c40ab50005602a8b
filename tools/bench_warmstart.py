'''
Time ato_warmstart against raceline.warmstart.drone_guess_batch on the same machine and the same inputs: fig-8,
parametric, N = 50, K = 4, quaternion and DCM pose, B = 512 and B = 8192, swept-heading point-mass vectors (three
quarters of a turn along the lap: quaternion signs flip along the chain and at the closure). The device figure is the
time per call over 50 back-to-back launches between two HIP events (median, min and max of 5 such windows, after
3 warm-up calls); the host figure is one call by the wall clock. Also reports the largest deviation of the device's
W from the host's, relative to max(1, |value|). Every (pose, batch) step is a child process under its own time limit;
the first one that fails ends the run.

    python tools/bench_warmstart.py [--launches 50] [--windows 5] [--limit 300] [--out f.json]
'''
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [('esp', 512), ('dcm', 512), ('esp', 8192), ('dcm', 8192)]


def swept_vectors(point, B, turns=0.75, seed=11):
    ''' (B, nw) point-mass vectors whose heading sweeps `turns` turns along the lap '''
    rng = np.random.default_rng(seed)
    N, P = point.N, point.P
    phi = 2 * np.pi * turns * np.arange(P)[None] / P + rng.uniform(0, 2 * np.pi, (B, 1))
    node = np.zeros((B, P, point.nv))
    node[..., :3] = rng.normal(size=(B, P, 3))
    node[..., 3:6] = 8 * np.stack([np.cos(phi), np.sin(phi), 0 * phi], axis=2) + [0, 0, 0.5]
    node[..., 6:9] = 4 * np.stack([np.cos(phi + 0.3), np.sin(phi + 0.3), 0 * phi], axis=2) + [0, 0, 9.81] + \
        rng.normal(0, 0.3, (B, P, 3))
    node[..., 9:12] = rng.normal(size=(B, P, 3))
    X = np.zeros((B, point.nw))
    X[:, :N] = rng.uniform(0.05, 0.2, (B, N))
    X[:, N:N + P * point.nv] = node.reshape(B, -1)
    return X


def one_step(pose, B, launches, windows):
    import torch
    from aircraft_trajectory_optimization_amd import native
    from aircraft_trajectory_optimization_amd.raceline.warmstart import drone_guess_batch, drone_guess_batch_device
    from aircraft_trajectory_optimization_amd.tracks import make_spec
    kw = dict(track='fig8', frame='parametric', N=50, K=4, global_r=True)
    drone = make_spec(**kw, model='drone', use_quat=True, use_dcm=pose == 'dcm')
    point = make_spec(**kw, model='point', use_quat=False)
    X = swept_vectors(point, B)
    t0 = time.perf_counter()
    Wh = drone_guess_batch(drone, point, X)[0]
    host_s = time.perf_counter() - t0
    dev = torch.device('cuda', torch.cuda.current_device())
    XP = torch.as_tensor(np.ascontiguousarray(X.T), device=dev)
    Wd = drone_guess_batch_device(drone, point, XP)[0]
    deviation = float(np.max(np.abs(Wd.T.cpu().numpy() - Wh) / np.maximum(1.0, np.abs(Wh))))
    pp, pd = native.NativeProblem(point.native_spec()), native.NativeProblem(drone.native_spec())
    W = torch.empty((drone.nw, B), dtype=torch.float64, device=dev)
    lo, hi = torch.empty((drone.N, B), dtype=torch.float64, device=dev), torch.empty((drone.N, B), dtype=torch.float64, device=dev)
    info = torch.empty((3, B), dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev)

    def call():
        pd.warmstart_ptrs(pp, B, XP.data_ptr(), W.data_ptr(), info.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                          stream=st.cuda_stream)
    for _ in range(3):
        call()
    st.synchronize()
    ms = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(launches):
            call()
        e1.record(st)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / launches)
    nbytes = (point.nw + drone.nw + 2 * drone.N + 3) * 8 * B
    return {'pose': pose, 'batch': B, 'N': drone.N, 'K': drone.K, 'launches': launches, 'windows': windows,
            'device_ms_per_call_median': float(np.median(ms)), 'device_ms_per_call_min': float(np.min(ms)),
            'device_ms_per_call_max': float(np.max(ms)), 'host_s_per_call': host_s,
            'bytes_read_and_written_once': int(nbytes), 'device_vs_host_max_rel_dev': deviation}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--launches', type=int, default=50)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--limit', type=int, default=300, help='seconds per (pose, batch) step')
    ap.add_argument('--out', default=None)
    ap.add_argument('--one', nargs=2, metavar=('POSE', 'BATCH'), default=None, help='run one step in this process')
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one_step(a.one[0], int(a.one[1]), a.launches, a.windows)), flush=True)
        return 0
    out = []
    for pose, B in STEPS:
        res = subprocess.run(['timeout', '-k', '10', str(a.limit), sys.executable, os.path.abspath(__file__), '--one',
                              pose, str(B), '--launches', str(a.launches), '--windows', str(a.windows)],
                             capture_output=True, text=True, check=False)
        if res.returncode != 0:
            print(res.stdout + res.stderr, file=sys.stderr)
            print(f'step {pose} B={B} ended with status {res.returncode}: stopping', file=sys.stderr)
            return res.returncode
        line = res.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        out.append(json.loads(line))
    if a.out:
        with open(a.out, 'w', encoding='utf-8') as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
