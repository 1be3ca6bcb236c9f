#!/usr/bin/env python3
"""Time the mutual-information alignment (multipoint_amd.utils.alignment) on the GPU with device events, next to the numpy +
scipy restatement (tests/mi_restatement.py) on the host as the CPU baseline.

    python tools/bench_mi.py [--height 480 --width 640] [--pairs 8] [--cpu-evals 3] [--cpu-align 0] [--out profiles/mi_bench.json]

Reports, per bin count: microseconds per objective evaluation at E = 1 and at E = 4 * pairs evaluations per call, and per
histogram strategy where two are possible (the histogram entry point alone, which is what the strategies differ in); the wall
time of align_images over all pairs and bin sizes with the solver's iteration counts; the host's time per evaluation and,
with --cpu-align N, its Nelder-Mead on the first N problems.  There is no CPU fallback: without a GPU this fails."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
BINS = [16, 32, 64, 100, 256]


def pairs(B, H, W):
    import mi_restatement as R
    T_true = np.array([[0.97, 0.006, 6.0], [-0.005, 0.975, 4.0], [3e-6, -2e-6, 1.0]])
    opt, th, init = [], [], []
    for b in range(B):
        o = R.blob_image(100 + b, H, W, 400, 3.0, 14.0)
        w = R.warp_image(o, T_true, H, W)
        opt.append(o); th.append((4.0 * (w.astype(np.float64) - 0.45) ** 2).astype(np.float32))
        init.append(T_true + np.array([[0.002, 0, 1.6], [0, -0.002, -1.3], [0, 0, 0]]))
    return np.stack(opt), np.stack(th), np.stack(init)


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # microseconds per call


def timed(fns, warmup=3, windows=7, reps=5):
    """[min, median, max] microseconds per call of each function over `windows` windows of `reps` calls; the functions'
    windows alternate, so that they see the same machine."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(windows):
        for i, fn in enumerate(fns):
            t[i].append(window(fn, reps))
    return [[min(x), sorted(x)[len(x) // 2], max(x)] for x in t]


def histogram_entry(A, o, t, pair, bins, T, strategy):
    """mp_mi_joint_histogram alone, on buffers allocated once: no copy of the counts to the host, no Python slicing.  (The
    entry point itself uploads the evaluation list and synchronises the stream once behind it; that is part of the call.)"""
    from multipoint_amd import _lib
    c = A._Call(o, t, pair, bins)
    E = len(pair)
    Td = torch.from_numpy(np.ascontiguousarray(T.reshape(-1, 9))).to(c.dev)
    counts = torch.empty(sum(2 * n * n for n in bins), dtype=torch.int32, device=c.dev)
    minmax = torch.empty((E, 2), dtype=torch.float32, device=c.dev)
    pi, bi = A._ints(pair), A._ints(bins)
    keep = (c, Td, counts, minmax, pi, bi)

    def call():
        c.h.check(c.h.lib.mp_mi_joint_histogram(*c.head(), pi, bi, _lib.ptr(Td), E, strategy, _lib.ptr(counts),
                                                _lib.ptr(minmax), None, *c.tail()))
        return keep
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--pairs', type=int, default=8)
    ap.add_argument('--cpu-evals', type=int, default=3)
    ap.add_argument('--cpu-align', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mi.py measures on the GPU only')
    from multipoint_amd.utils import alignment as A
    import mi_restatement as R
    B, H, W = args.pairs, args.height, args.width
    opt, th, init = pairs(B, H, W)
    o, t = torch.from_numpy(opt).cuda()[:, None], torch.from_numpy(th).cuda()[:, None]
    res = {'device': torch.cuda.get_device_name(0), 'height': H, 'width': W, 'pairs': B, 'objective_us_per_eval': {},
           'histogram_us_per_eval': {}, 'timing': '[min, median, max] over 7 windows of 5 calls, device events around each window, '
           'the variants of a row alternating.  objective: whole Python calls (workspace allocation, list upload, the once-per-call '
           'thermal bin maps and the entry point\'s one stream synchronisation included).  histogram: the C entry alone on '
           'preallocated buffers (list upload, thermal maps and that synchronisation included; no copy of the counts)'}
    try:
        res['commit'] = subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, text=True).strip()
    except Exception:
        res['commit'] = None
    E = 4 * B
    jitter = np.array([[0, 0, 0.3], [0, 0, -0.2], [0, 0, 0]])
    many = np.stack([np.stack([init[b] + k * jitter for k in range(4)]) for b in range(B)])          # (B, 4, 3, 3)
    pair = [b for b in range(B) for _ in range(4)]
    for n in BINS:
        one, batch = timed([lambda: A.negative_mutual_information_batch(o[:1], t[:1], init[:1, None], n, normalized_mi=True),
                            lambda: A.negative_mutual_information_batch(o, t, many, n, normalized_mi=True)])
        res['objective_us_per_eval'][n] = {'E=1': one, 'E=%d' % E: [v / E for v in batch]}
        names = [('lds', 1), ('global', 2)] if n <= 64 else [('global', 2)]
        spread = timed([histogram_entry(A, o, t, pair, [n] * E, many, s) for _, s in names])
        res['histogram_us_per_eval'][n] = {name: [v / E for v in x] for (name, _), x in zip(names, spread)}
        print(n, res['objective_us_per_eval'][n], res['histogram_us_per_eval'][n], flush=True)
    params = {'alignment/bin_sizes': BINS, 'alignment/normalized_mi': True, 'alignment/smoothing_sigma': 0,
              'alignment/check/both/max_diff_mi': 0.5, 'alignment/accept_init': True, 'alignment/ranking_method': 'order'}
    A.align_images(o[:1], t[:1], init[:1], dict(params, **{'alignment/bin_sizes': [16]}))        # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    T, kinds, cands = A.align_images(o, t, init, params)
    torch.cuda.synchronize()
    res['align_images'] = {'wall_s': time.perf_counter() - t0, 'problems': B * len(BINS), 'types': kinds,
                           'nit': [[c.get('nit') for c in cs] for cs in cands], 'nfev': [[c.get('nfev') for c in cs] for cs in cands]}
    print('align_images', res['align_images']['wall_s'], kinds, flush=True)
    cpu = {}
    for n in BINS:
        t0 = time.perf_counter()
        for k in range(args.cpu_evals):
            R.negative_mi(init[0] + k * jitter, opt[0], th[0], init[0], n, False, True, 0)
        cpu[n] = (time.perf_counter() - t0) / max(args.cpu_evals, 1) * 1e6
    res['cpu_restatement_us_per_eval'] = cpu
    res['cpu_threads'] = os.environ.get('OMP_NUM_THREADS')
    if args.cpu_align > 0:
        t0 = time.perf_counter()
        stats = []
        for q in range(args.cpu_align):
            b, n = divmod(q, len(BINS))[0] % B, BINS[q % len(BINS)]
            r = R.nelder_mead(lambda x: R.negative_mi(x, opt[b], th[b], init[b], n, False, True, 0), init[b].ravel(), 1e-6, 1e-6)
            stats.append((n, r['nit'], r['nfev'], r['success']))
        res['cpu_nelder_mead'] = {'wall_s': time.perf_counter() - t0, 'problems': stats}
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
