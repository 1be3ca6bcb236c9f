#!/usr/bin/env python3
"""Time the image pyramid (csrc/pyramid.hip) and the staged mutual-information alignment built on it
(multipoint_amd.utils.alignment.align_images_mutual_information) on the GPU.

    python tools/bench_mi_pyramid.py [--height 240 --width 320] [--pairs 16] [--out profiles/mi_pyramid_bench.json]

Blur: microseconds per frame of mp_gaussian_blur at 512 x 640, B = 16, k = 5, with and without decimation (the C entry on
preallocated buffers, device events around windows of calls), next to the bytes it has to move -- read 4 H W, write 4 H W or
H W per frame -- and the rate that is.
Staged alignment: the same `--pairs` pairs, displaced by about 10.5 px at 96 x 128 and in proportion at other sizes, through
today's single-stage align_images and through the staged procedure with one and two pyramid levels: wall time, objective
launches enqueued (`rounds`), the solver's iterations in the full-resolution stage, and the four-corner error reached.
There is no CPU fallback: without a GPU this fails."""
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
from bench_mi import timed          # noqa: E402  (tools/ is this script's directory)

BINS = [16, 32, 64]


def pairs(B, H, W):
    import mi_restatement as R
    s = W / 128.0
    T_true = np.array([[0.94, 0.012, 6.0 * s], [-0.01, 0.95, 4.0 * s], [1.5e-5 / s, -1e-5 / s, 1.0]])
    opt, th, init = [], [], []
    for b in range(B):
        o = R.blob_image(200 + b, H, W, 150, 2.0 * s, 6.0 * s)
        w = R.warp_image(o, T_true, H, W)
        opt.append(o); th.append((4.0 * (w.astype(np.float64) - 0.45) ** 2).astype(np.float32))
        init.append(T_true + np.array([[0.004, 0, 8.0 * s], [0, -0.003, -6.4 * s], [0, 0, 0]]))
    return np.stack(opt), np.stack(th), np.stack(init), T_true


def blur_entry(x, k, decimate):
    from multipoint_amd import _lib
    B, H, W = x.shape
    out = torch.empty((B, (H + 1) // 2, (W + 1) // 2) if decimate else (B, H, W), dtype=torch.float32, device=x.device)
    h = _lib.get_handle(x.device)
    stream = _lib.stream_ptr(x.device)

    def call():
        h.check(h.lib.mp_gaussian_blur(h.ptr, _lib.ptr(x), B, H, W, k, int(decimate), _lib.ptr(out), stream))
        return out
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=240)
    ap.add_argument('--width', type=int, default=320)
    ap.add_argument('--pairs', type=int, default=16)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_mi_pyramid.py measures on the GPU only')
    from multipoint_amd.utils import alignment as A
    import mi_restatement as R
    res = {'device': torch.cuda.get_device_name(0)}
    try:
        res['commit'] = subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, text=True).strip()
    except Exception:
        res['commit'] = None

    # ---- the blur ----
    Bb, Hb, Wb, k = 16, 512, 640, 5
    x = torch.rand((Bb, Hb, Wb), dtype=torch.float32, device='cuda')
    full, half = timed([blur_entry(x, k, False), blur_entry(x, k, True)], warmup=5, windows=9, reps=50)
    res['blur'] = {'frames': Bb, 'height': Hb, 'width': Wb, 'ksize': k,
                   'timing': '[min, median, max] over 9 windows of 50 calls, device events around each window, the two variants '
                             'alternating; the C entry on preallocated buffers'}
    for name, t, out_bytes in (('full', full, 4 * Hb * Wb), ('decimated', half, 4 * ((Hb + 1) // 2) * ((Wb + 1) // 2))):
        floor = 4 * Hb * Wb + out_bytes
        res['blur'][name] = {'us_per_frame': [v / Bb for v in t], 'floor_bytes_per_frame': floor,
                             'GB_per_s_at_median': floor * Bb / (t[1] * 1e-6) / 1e9}
        print('blur', name, res['blur'][name], flush=True)

    # ---- the staged alignment ----
    B, H, W = args.pairs, args.height, args.width
    opt, th, init, T_true = pairs(B, H, W)
    o, t = torch.from_numpy(opt).cuda(), torch.from_numpy(th).cuda()
    base = {'alignment/bin_sizes': BINS, 'alignment/normalized_mi': True, 'alignment/smoothing_sigma': 0,
            'alignment/check/both/max_diff_mi': 0.5, 'alignment/accept_init': True, 'alignment/ranking_method': 'sum',
            'alignment/filter_size': 5}
    A.align_images_mutual_information(o[:1], t[:1], init[:1], dict(base, use_image_pyramid=True, **{
        'alignment/bin_sizes': [16], 'alignment/n_pyramid_levels': 2}))                     # warm-up
    torch.cuda.synchronize()
    e0 = [R.corner_error(init[b], T_true, H, W) for b in range(B)]
    res['alignment'] = {'pairs': B, 'height': H, 'width': W, 'bin_sizes': BINS, 'initial_error_px': float(np.mean(e0)),
                        'timing': 'one run each, host clock around the call and a device synchronise'}
    for name, levels in (('single_stage', 0), ('one_level', 1), ('two_levels', 2)):
        stats = {}
        params = dict(base, use_image_pyramid=levels > 0, **{'alignment/n_pyramid_levels': max(levels, 1)})
        t0 = time.perf_counter()
        if levels == 0:
            Ts, kinds, cands = A.align_images(o, t, init, params, stats=stats)
            stage_types = None
        else:
            out = A.align_images_mutual_information(o, t, init, params, stats=stats)
            Ts, kinds, cands = [r[1] for r in out], [r[2] for r in out], [r[3] for r in out]
            stage_types = [[(s['name'], s['type']) for s in r[4]] for r in out]
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        err = [R.corner_error(Ts[b], T_true, H, W) if Ts[b] is not None else None for b in range(B)]
        nit = [[c['nit'] for c in cs if 'nit' in c] for cs in cands]                 # the full-resolution stage's solver runs
        res['alignment'][name] = {'wall_s': wall, 'rounds': stats.get('rounds', 0), 'error_px': err, 'types': kinds,
                                  'final_stage_nit': nit, 'final_stage_nit_mean': float(np.mean([v for r in nit for v in r] or [0])),
                                  'stages': stage_types}
        print(name, 'wall %.2f s, rounds %d, mean error %.3f px, mean final-stage iterations %.0f' % (
            wall, stats.get('rounds', 0), float(np.mean([e for e in err if e is not None])),
            res['alignment'][name]['final_stage_nit_mean']), flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
