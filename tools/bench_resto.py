'''
Microbenchmark of the restoration phase's five wrapper sites (solver/batched_ipm.py: the KKT residual of the
nested solve, _RestorationEvaluator.eval / hess, _RestorationKKT.factor / solve), torch formulation
(BatchedInteriorPoint.FUSED_RESTO off) against the fused column kernels (on), on the config-3 structure
(race, N = 50, K = 4) with seeded random values. Single-threaded, no profiler needed.

Per site, path and width W: device launches per call (torch operators that launch, counted with a torch
dispatch mode as tools/diag/glue_sites.py does, plus the library's own launches), the bytes moved (torch: the
inputs and outputs of every counted operator; fused: each operand once), the time per call from device events
over --reps calls after a warm-up, and the achieved GB/s with its fraction of --stream-gbs (the rate a
streaming kernel achieves on the device; the residual is gather-bound and its fraction is what it is).
The base factorisation is replaced by a stub, so only the wrappers are timed.

    python tools/bench_resto.py [--widths 35 185 512] [--reps 50] [--json out.json]
'''
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FREE = ('aten.view', 'aten._unsafe_view', 'aten.t.', 'aten.alias', 'aten.detach', 'aten.unsqueeze', 'aten.squeeze',
        'aten.expand', 'aten.reshape', 'aten.select.', 'aten.slice.', 'aten.as_strided.', 'aten.permute',
        'aten.transpose', 'aten.empty', 'aten._local_scalar_dense', 'aten.size', 'aten.stride', 'aten.is_nonzero',
        'aten.lift_fresh', 'aten.unbind', 'aten.split.', 'aten.chunk', 'aten.sym_')


class _Base:
    def __init__(self, ev, W, dev):
        self.n, self.m, self.batch, self.device = ev.n, ev.m, W, dev
        for k in ('j_row_ptr', 'j_col', 'h_row_ptr', 'h_col'):
            setattr(self, k, np.asarray(getattr(ev, k), np.int64))
        self.lbg, self.ubg = np.asarray(ev.lbg, float), np.asarray(ev.ubg, float)
        self.vals = {}

    def eval(self, x):
        return self.vals['f'], self.vals['g'], self.vals['gf'], self.vals['jv']

    def eval_fg(self, x):
        return self.vals['f'], self.vals['g']

    def hess(self, x, lam, sigma):
        return self.vals['H0']


class _StubKKT:
    def __init__(self, W, dev):
        self.inertia = torch.zeros((W, 3), dtype=torch.int32, device=dev)

    def factor(self, H, J, dx, dr, instances):
        return self.inertia

    def solve(self, x, instances):
        return x


def _nbytes(ts):
    return sum(t.numel() * t.element_size() for t in ts if torch.is_tensor(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--widths', type=int, nargs='+', default=[35, 185, 512])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--stream-gbs', type=float, default=6300.0,
                    help='achievable rate of a streaming kernel on the device (GB/s) the fractions refer to')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    from torch.utils._python_dispatch import TorchDispatchMode
    from aircraft_trajectory_optimization_amd.solver import ipm_device
    from aircraft_trajectory_optimization_amd.solver.batched_ipm import (BatchedDeviceEvaluator, BatchedInteriorPoint,
                                                                         _RestorationEvaluator, _RestorationKKT,
                                                                         _RestorationStructure)
    from aircraft_trajectory_optimization_amd.tracks import make_spec
    dev = torch.device('cuda', 0)
    spec = make_spec(track='race', N=50, K=4)
    ev = BatchedDeviceEvaluator(spec, 1, dev)
    count = {'ops': 0, 'bytes': 0, 'native': 0}

    class Count(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            flat = list(args) + list((kwargs or {}).values())
            if any(torch.is_tensor(t) and t.is_cuda for t in flat) and not str(func).startswith(FREE):
                count['ops'] += 1
                count['bytes'] += _nbytes(flat) + _nbytes(out if isinstance(out, (tuple, list)) else [out])
            return out

    rc = ipm_device._rc

    def counting_rc(lib, code, what):
        count['native'] += 1
        return rc(lib, code, what)
    ipm_device._rc = counting_rc

    rows = []
    for W in args.widths:
        base = _Base(ev, W, dev)
        n, m = base.n, base.m
        g = torch.Generator(device='cpu').manual_seed(W)

        def rnd(r, lo=-3.0, hi=3.0):
            mag = 10.0 ** (lo + (hi - lo) * torch.rand((r, W), generator=g, dtype=torch.float64))
            sign = torch.where(torch.rand((r, W), generator=g) < 0.5, -1.0, 1.0)
            return (mag * sign).to(dev)
        base.vals = {'f': torch.zeros(W, dtype=torch.float64, device=dev), 'g': rnd(m), 'gf': rnd(n),
                     'jv': rnd(len(base.j_col)), 'H0': rnd(len(base.h_col))}
        st = _RestorationStructure(base)
        sg = rnd(m, -2.0, 0.0).abs()
        lbg = torch.as_tensor(np.repeat(base.lbg[:, None], W, axis=1), device=dev)
        ubg = torch.as_tensor(np.repeat(base.ubg[:, None], W, axis=1), device=dev)
        zeta = torch.rand(W, generator=g, dtype=torch.float64).to(dev)
        rev = _RestorationEvaluator(base, sg, rnd(n), zeta, 1000.0, lbg, ubg, st)
        nr = rev.n
        ipm = BatchedInteriorPoint(rev, _StubKKT(W, dev), np.full(nr, -1.0), np.full(nr, 1.0))
        kkt = _RestorationKKT(_StubKKT(W, dev), rev)
        X, lam, sigma = rnd(n + 2 * m), rnd(m), torch.rand(W, generator=g, dtype=torch.float64).to(dev)
        H, J = rnd(st.nnz_h), rnd(len(st.j_col))
        dxk, drk, v, rhs = rnd(nr), rnd(m), rnd(nr + m), rnd(nr + m)
        dx, dr, x = rnd(n + 2 * m), rnd(m), rnd(n + 3 * m)
        lst = np.arange(0, W, 2, dtype=np.int32)
        nj0, nh0, nh, nj = len(base.j_col), len(base.h_col), st.nnz_h, len(st.j_col)
        d = 8 * W

        def factor_first():
            kkt.invalidate()
            return kkt.factor(H, J, dx, dr, lst)
        # fused bytes: every operand of the site once (index arrays left out: they are shared by the W columns)
        sites = {
            'residual': (lambda: ipm._residual(H, J, dxk, drk, v, rhs), d * (nh + nj + nr + m + 3 * (nr + m))),
            'eval': (lambda: rev.eval(X), d * (3 * m + nj0 + 2 * n + (n + 2 * m) + nj + (n + 2 * m))),
            'eval_fg': (lambda: rev.eval_fg(X), d * (5 * m)),
            'hess': (lambda: rev.hess(X, lam, sigma), d * (nh0 + n + nh)),
            'factor_first_pass': (factor_first, d * (nh + nj + nh0 + nj0 + n + (n + 2 * m) + m + n + n + 3 * m)),
            'factor_next_pass': (lambda: kkt.factor(H, J, dx, dr, lst), d * ((n + 2 * m) + m + n + n + 3 * m)),
            'solve': (lambda: kkt.solve(x, lst), d * ((n + 3 * m) + 2 * m + 2 * (n + m) + 2 * m + (n + 3 * m))),
        }
        for site, (fn, fused_bytes) in sites.items():
            for fused in (False, True):
                BatchedInteriorPoint.FUSED_RESTO = fused
                for _ in range(args.warmup):
                    fn()
                count.update(ops=0, bytes=0, native=0)
                with Count():
                    fn()
                launches = count['ops'] + count['native']
                nbytes = fused_bytes if fused else count['bytes']
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    fn()
                e1.record()
                e1.synchronize()
                us = e0.elapsed_time(e1) * 1e3 / args.reps
                gbs = nbytes / us / 1e3
                rows.append({'site': site, 'W': W, 'path': 'fused' if fused else 'torch', 'launches': launches,
                             'torch_ops': count['ops'], 'native_launches': count['native'], 'bytes': nbytes,
                             'us_per_call': us, 'gb_per_s': gbs, 'frac_of_stream': gbs / args.stream_gbs})
                r = rows[-1]
                print(f"{site:18s} W={W:4d} {r['path']:5s} launches {launches:3d}  {nbytes / 1e6:9.2f} MB  "
                      f"{us:9.1f} us  {gbs:8.1f} GB/s  ({r['frac_of_stream']:.2f} of {args.stream_gbs:.0f})", flush=True)
        BatchedInteriorPoint.FUSED_RESTO = True
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w', encoding='utf-8') as fh:
            json.dump({'reps': args.reps, 'stream_gbs': args.stream_gbs, 'rows': rows}, fh, indent=1)


if __name__ == '__main__':
    main()
