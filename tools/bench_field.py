#!/usr/bin/env python3
"""Time the local alignment correction (multipoint_amd.utils.field) on the GPU with device events.

    python tools/bench_field.py [--height 480 --width 640] [--batch 32] [--window 32 --stride 16 --radius 8] [--rounds 3]
                                [--runs 20] [--out profiles/field_bench.json]

  fit.kernel      mp_field_fit alone on a resident lattice of measured displacements: one workgroup per pair
  warp.kernel     mp_field_warp alone on resident frames and fields, with the validity mask
  correct.call    correct_locally as a user calls it: rounds + 1 measurements, `rounds` fits and warps, every read-back
Each figure is the median (min, max) of the timed calls after 3 warm-up calls, microseconds per CALL on the whole batch;
*_per_pair divides by the batch.  warp_bytes: 4 B read and 5 B written per pixel, what the warp must move; its rate is a
whole-kernel figure.  Frames are seeded noise, smoothed, the optical side sampled through a smooth planted displacement of up to
2 px and the thermal side contrast inverted; the share of corrected pairs and the medians before and after are recorded as a
sanity check.  There is no target and nothing to compare with: the figures are only recorded.  There is no CPU fallback."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--window', type=int, default=32)
    ap.add_argument('--stride', type=int, default=16)
    ap.add_argument('--radius', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_field.py measures on the GPU only')
    from multipoint_amd import _lib
    from multipoint_amd.utils import field as U
    from multipoint_amd.utils import residual as R
    B, H, W = args.batch, args.height, args.width
    g = torch.Generator(device='cuda').manual_seed(5)
    base = torch.rand((B, 1, H, W), generator=g, device='cuda')
    base = torch.nn.functional.avg_pool2d(base, 5, stride=1, padding=2)[:, 0]            # (set-up only: not what is timed)
    base = ((base - base.amin()) / (base.amax() - base.amin())).contiguous()
    thermal = (1.0 - base).contiguous()
    # the planted displacement on a coarse lattice of its own: optical[q] = base[q - g(q)]
    plant = np.zeros((B, 4, 5, 2))
    yy, xx = np.mgrid[0:4, 0:5]
    for b in range(B):
        plant[b, ..., 0] = -(1.0 + 0.8 * np.sin(xx + 0.2 * b) - 0.15 * yy)
        plant[b, ..., 1] = -(-0.4 * yy + 0.6 * np.cos(0.7 * xx + 0.1 * b))
    optical = U.warp_by_field(base, plant, (0.0, 0.0, float(max(H - 1, W - 1)) / 3.0), extrapolate='linear').contiguous()
    kw = dict(window=args.window, stride=args.stride, radius=args.radius)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); out = fn(); b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3, out

    def stats(ts):
        ts = sorted(ts)
        return {'min': ts[0], 'median': ts[len(ts) // 2], 'max': ts[-1], 'n': len(ts)}

    f = R.residual_field(optical, thermal, **kw)
    geometry = U.field_geometry(f)
    gy, gx = f['rho'].shape[1:]
    h = _lib.get_handle(optical.device)
    d = torch.from_numpy(f['d']).cuda()
    w = torch.from_numpy(U.field_weights(f)).cuda()
    size = _lib.c_ll()
    h.check(h.lib.mp_field_fit_workspace(B, gy, gx, ctypes.byref(size)))
    ws = torch.empty(size.value // 8, dtype=torch.float64, device='cuda')
    out_u = torch.empty((B, gy, gx, 2), dtype=torch.float64, device='cuda')
    out_i = torch.empty((B, 4), dtype=torch.int32, device='cuda')
    out_r = torch.empty((B,), dtype=torch.float64, device='cuda')
    dst = torch.empty((B, H, W), dtype=torch.float32, device='cuda')
    valid = torch.empty((B, H, W), dtype=torch.uint8, device='cuda')
    stream = _lib.stream_ptr(optical.device)

    def fit():
        h.check(h.lib.mp_field_fit(h.ptr, _lib.ptr(d), _lib.ptr(w), B, gy, gx, 0.25, 0.0, 0, 1e-12, 4 * gy * gx + 64, _lib.ptr(ws),
                                   size.value, _lib.ptr(out_u), _lib.ptr(out_i), _lib.ptr(out_r), None, stream))

    def warp():
        h.check(h.lib.mp_field_warp(h.ptr, _lib.ptr(optical), B, H, W, _lib.ptr(out_u), gy, gx, geometry[0], geometry[1], geometry[2],
                                    1, None, B, H, W, _lib.ptr(dst), _lib.ptr(valid), stream))

    def call():
        return U.correct_locally(optical, thermal, rounds=args.rounds, **kw)
    for _ in range(3):
        fit(); warp(); call()
    tf, tw, tc = [], [], []
    for i in range(args.runs):
        tf.append(timed(fit)[0])
        tw.append(timed(warp)[0])
        dt, res = timed(call)
        tc.append(dt)
        print('run %d: fit %.0f us, warp %.0f us, correct_locally %.0f us' % (i, tf[-1], tw[-1], tc[-1]), file=sys.stderr, flush=True)
    info = out_i.cpu().numpy()
    kf, kw_, kc = stats(tf), stats(tw), stats(tc)
    warp_bytes = B * H * W * 9
    out = {'device': torch.cuda.get_device_name(0), 'frame': [H, W], 'batch': B, 'window': args.window, 'stride': args.stride,
           'radius': args.radius, 'rounds': args.rounds, 'lattice': [gy, gx],
           'timing': 'median (min, max) of the timed calls after 3 warm-up calls, device events around each call, microseconds per '
                     'CALL on the whole batch; measured on one box; no target, recorded only',
           'fit_us': kf, 'fit_us_per_pair': kf['median'] / B, 'fit_iterations': [int(info[:, 1].min()), int(info[:, 1].max())],
           'warp_us': kw_, 'warp_us_per_pair': kw_['median'] / B, 'warp_bytes': int(warp_bytes),
           'warp_gbytes_per_s': warp_bytes / kw_['median'] * 1e-3,
           'correct_us': kc, 'correct_us_per_pair': kc['median'] / B,
           'applied_share': float(np.mean(res['applied'])),
           'median_mag_first': float(np.nanmedian([s['median_mag'] for s in res['summaries'][0]])),
           'median_mag_final': float(np.nanmedian([s['median_mag'] for s in res['summaries'][-1]]))}
    try:
        out['commit'] = subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, text=True,
                                                stderr=subprocess.DEVNULL).strip()
    except Exception:
        out['commit'] = None
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(out, fh, indent=1)


if __name__ == '__main__':
    main()
