'''
Time the comparison of solutions (ato_compare_sample, ato_compare_pairs: k_compare_pairs, ato_compare_groups) with
HIP events at B = 512 of config 3's shape (race track, 50 x 4, parametric ESP drone) and B = 8192 of config 5's
(figure of eight, parametric DCM drone), at count = 64 and 256 samples. Inputs are the cold start replicated with a
small seeded perturbation of every node variable (every column another line: the groups are singletons and the pair
kernel does all its work). Warm-up first; every figure is the time per call of INNER = 50 back-to-back calls between
one pair of events, the median over --reps such pairs; everything in one process on one device. Timed: the position
table; the self-comparison with the three distance planes and the bits; the self-comparison with the bits alone (what
a grouping call needs); the groups. Beside them the same three planes by a chunked torch broadcast on the device on
the same table (the baseline, not the code under test; a few calls, it is slow), checked against the kernel's.
The path kernel (ato_compare_path: k_compare_path) is timed on the same tables the same way, eight planes and bits
and bits alone, beside a chunked torch broadcast of its formula (both directions; one call per window).
Its flop model: 23 per (directed pair, sample, segment) -- 3 differences, the dot product 5, the product with inv 1,
the clamp 2, c = r - t e 6, c.c 5, the comparison 1, fused multiply-adds counted as two, no selects -- over both
directions of the B (B + 64) / 2 pairs of the tiles that run, M samples and M - 1 segments each. At B = 8192 a call
takes seconds: there the event pairs span PATH_INNER_LARGE calls, and the torch broadcast is timed on its first row
chunk alone and scaled to the B rows (it is linear in them).
Flop model of the pair kernel: 8 per (pair, sample) (3 differences, 1 product, 2 fused multiply-adds counted once, 1 sum, 1 maximum)
over the B (B + 64) / 2 pairs of the tiles on and above the diagonal; the share is of the 78.6 TF/s fp64 vector peak.

    python tools/bench_compare.py [--reps 5] [--out f.json]
'''
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP = 2
INNER = 50              # calls per event pair
PEAK = 78.6e12
CHUNK_BYTES = 2 ** 30   # the torch baseline's largest temporary
PATH_INNER_LARGE = 2


def timed(fn, reps, st, inner=INNER):
    ''' ms per call: every event pair spans `inner` back-to-back calls on the stream '''
    ms = []
    for i in range(reps + WARMUP):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(inner):
            fn()
        e1.record(st)
        e1.synchronize()
        if i >= WARMUP:
            ms.append(e0.elapsed_time(e1) / inner)
    return {'ms_median': float(np.median(ms)), 'ms_min': float(np.min(ms)), 'ms_max': float(np.max(ms))}


def torch_pairs(X, out):
    ''' rms, max and lap fraction of the max of every pair of the table X (3, M, B) into out (3, B, B), row chunks '''
    _, M, B = X.shape
    rows = max(1, CHUNK_BYTES // (3 * M * B * 8))
    for a0 in range(0, B, rows):
        d2 = ((X[:, :, a0:a0 + rows, None] - X[:, :, None, :]) ** 2).sum(0)
        mx, at = d2.max(0)
        out[0, a0:a0 + rows] = d2.mean(0).sqrt()
        out[1, a0:a0 + rows] = mx.sqrt()
        out[2, a0:a0 + rows] = at.double() / (M - 1)


def torch_path(X, out, first_only=False):
    ''' the eight channels of ato_compare_path of the table X (3, M, B) against itself into out (8, B, B), row chunks;
    the rows' samples against the columns' segments, the other direction is the transpose '''
    _, M, B = X.shape
    x = X.permute(1, 2, 0)                                  # (M, B, 3)
    q0 = x[None, None, :-1]
    e = x[None, None, 1:] - q0                              # (1, 1, S, B, 3)
    ee = (e * e).sum(-1)
    inv = torch.where(ee == 0, 0.0, 1.0 / ee)
    rows = max(1, CHUNK_BYTES // (3 * M * (M - 1) * B * 8))
    for a0 in range(0, B, rows):
        r = x[:, a0:a0 + rows, None, None] - q0             # (M, rows, S, B, 3)
        t = ((r * e).sum(-1) * inv).clamp(0, 1)
        d2, seg = ((r - t[..., None] * e) ** 2).sum(-1).min(2)      # (M, rows, B)
        mx, at = d2.max(0)
        s = seg.gather(0, at[None])[0]
        out[0, a0:a0 + rows] = d2.mean(0).sqrt()
        out[1, a0:a0 + rows] = mx.sqrt()
        out[2, a0:a0 + rows] = at.double() / (M - 1)
        out[3, a0:a0 + rows] = (s.double() + t.gather(2, seg[:, :, None]).squeeze(2).gather(0, at[None])[0]) / (M - 1)
        if first_only:
            return min(rows, B)
    out[4:] = out[:4].transpose(1, 2)
    return B


def time_shape(name, B, count, reps, track, path_inner=INNER, **kw):
    from aircraft_trajectory_optimization_amd import native
    from aircraft_trajectory_optimization_amd.raceline.batched import BatchedNLP
    from aircraft_trajectory_optimization_amd.tracks import make_spec
    spec = make_spec(track=track, N=50, K=4, model='drone', frame='parametric', global_r=True, **kw)
    rng = np.random.default_rng(0)
    W = np.repeat(np.array(spec.w0)[None], B, axis=0)
    W[:, spec.N:spec.N + spec.P * spec.nv] += 0.02 * rng.standard_normal((B, spec.P * spec.nv))
    nlp = BatchedNLP(spec, B, buffers=False)
    dev = nlp.device
    X = torch.as_tensor(np.ascontiguousarray(W.T), device=dev)
    st = torch.cuda.current_stream(dev)
    pos, lap = nlp.compare_sample(X, count=count)
    val = torch.empty((native.ATO_COMPARE_NCH, B, B), device=dev, dtype=torch.float64)
    bits = torch.empty((B, (B + 63) // 64), device=dev, dtype=torch.int64)
    group, info = (torch.empty((n,), device=dev, dtype=torch.int32) for n in (B, 2))

    def check(rc):
        if rc != native.ATO_OK:
            raise RuntimeError(native.load().ato_last_error().decode())

    def sample():
        nlp.problem.compare_sample_ptrs(B, X.data_ptr(), count, pos.data_ptr(), lap.data_ptr(), stream=st.cuda_stream)

    def pairs(with_val):
        check(native.compare_pairs_rc(count, B, pos.data_ptr(), 0, 0, 0, 0.05, val.data_ptr() if with_val else 0,
                                      bits.data_ptr(), st.cuda_stream))

    def groups():
        check(native.compare_groups_rc(B, bits.data_ptr(), group.data_ptr(), info.data_ptr(), st.cuda_stream))

    t = {'sample': timed(sample, reps, st), 'pairs_val_and_bits': timed(lambda: pairs(True), reps, st),
         'pairs_bits_only': timed(lambda: pairs(False), reps, st), 'groups': timed(groups, reps, st)}
    pval = torch.empty((native.ATO_COMPARE_PATH_NCH, B, B), device=dev, dtype=torch.float64)

    def path(with_val):
        check(native.compare_path_rc(count, B, pos.data_ptr(), 0, 0, 0, 0.05, pval.data_ptr() if with_val else 0,
                                     bits.data_ptr(), st.cuda_stream))

    t['path_val_and_bits'] = timed(lambda: path(True), reps, st, inner=path_inner)
    t['path_bits_only'] = timed(lambda: path(False), reps, st, inner=path_inner)
    pref = torch.empty_like(pval)
    large = path_inner != INNER
    done = torch_path(pos, pref, first_only=large)
    t['torch_path_broadcast'] = timed(lambda: torch_path(pos, pref, first_only=large), 1, st, inner=1)
    t['torch_path_broadcast'] = {k: v * B / done for k, v in t['torch_path_broadcast'].items()}
    path(True)
    ref = torch.empty_like(val)
    t['torch_broadcast'] = timed(lambda: torch_pairs(pos, ref), min(reps, 3), st, inner=1)
    scale = float(ref[1].max())
    flops = 8.0 * count * B * (B + 64) / 2
    out = {'shape': name, 'batch': B, 'count': count, 'reps': reps, 'calls_per_event_pair': INNER, 'ms': t,
           'flops_model': flops, 'n_groups': int(torch.unique(group).numel()), 'sweeps': int(info[0]),
           'kernel_vs_torch_max_abs_diff_m': float((val[:2] - ref[:2]).abs().max()), 'largest_distance_m': scale,
           'at_equal_share': float((val[2] == ref[2]).double().mean())}
    for k in ('pairs_val_and_bits', 'pairs_bits_only'):
        out[f'{k}_TFps'] = flops / (t[k]['ms_median'] * 1e-3) / 1e12
        out[f'{k}_share_of_fp64_vector_peak'] = flops / (t[k]['ms_median'] * 1e-3) / PEAK
    pflops = 23.0 * count * (count - 1) * B * (B + 64)
    for k in ('path_val_and_bits', 'path_bits_only'):
        out[f'{k}_TFps'] = pflops / (t[k]['ms_median'] * 1e-3) / 1e12
        out[f'{k}_share_of_fp64_vector_peak'] = pflops / (t[k]['ms_median'] * 1e-3) / PEAK
    out.update({'path_flops_model': pflops, 'path_calls_per_event_pair': path_inner,
                'torch_path_rows_timed': done,
                'path_kernel_vs_torch_max_abs_diff_m': float((pval[[0, 1], :done] - pref[[0, 1], :done]).abs().max()),
                'torch_path_over_kernel': t['torch_path_broadcast']['ms_median'] / t['path_val_and_bits']['ms_median']})
    out['torch_over_kernel'] = t['torch_broadcast']['ms_median'] / t['pairs_val_and_bits']['ms_median']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = []
    for count in (64, 256):
        res.append(time_shape(f'race esp-parametric B=512 M={count}', 512, count, a.reps, 'race', use_quat=True))
        res.append(time_shape(f'fig8 dcm-parametric B=8192 M={count}', 8192, count, a.reps, 'fig8',
                              path_inner=PATH_INNER_LARGE, use_quat=True, use_dcm=True))
    for r in res:
        print(f"{r['shape']}: {r['n_groups']} groups in {r['sweeps']} sweeps; kernel against torch: "
              f"{r['kernel_vs_torch_max_abs_diff_m']:.2e} m of {r['largest_distance_m']:.1f} m, torch / kernel = "
              f"{r['torch_over_kernel']:.1f}")
        for k, v in r['ms'].items():
            extra = f", {r[k + '_TFps']:.2f} TF/s = {100 * r[k + '_share_of_fp64_vector_peak']:.1f} % of the fp64 " \
                    f"vector peak" if k + '_TFps' in r else ''
            if k == 'path_val_and_bits':
                print(f"    path kernel against torch: {r['path_kernel_vs_torch_max_abs_diff_m']:.2e} m, torch / kernel = "
                      f"{r['torch_path_over_kernel']:.1f} ({r['torch_path_rows_timed']} rows of the broadcast timed)")
            print(f"    {k}: {v['ms_median'] * 1e3:.1f} us median ({v['ms_min'] * 1e3:.1f} - {v['ms_max'] * 1e3:.1f})"
                  f"{extra}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
