#!/usr/bin/env python3
"""Time the frame preparation (multipoint_amd.utils.frames, csrc/frames.hip) on the GPU with device events, per stage and per
pair, next to the bytes each stage has to move.

    python tools/bench_frames.py [--optical 1200 1600] [--thermal 512 640] [--batch 16] [--runs 30] [--out profiles/frames_bench.json]

Stages: undistort + rotate (the 16-bit thermal frame, rotation fused), undistort of the 8-bit optical frame, resize of the optical
frame to the thermal height, the thermal rescale, and the whole prepare_frames.  Each figure is the median of --runs timed calls
after warm-up, in microseconds per PAIR, whole Python calls with output and workspace allocation included.  bytes_model counts
what a stage must read and write once, from the shapes; `floor_us` is that over 4 TB/s and `ratio_to_floor` the measured median
over it.  There is no CPU fallback: without a GPU this fails."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
FLOOR_BYTES_PER_US = 4e12 / 1e6


def median_us(fn, runs, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    t.sort()
    return {'min': t[0], 'median': t[len(t) // 2], 'max': t[-1]}


def bytes_model(Ho, Wo, Ht, Wt, oh, ow):
    """bytes per pair each stage reads and writes once"""
    return {'undistort + rotate thermal': 2 * Ht * Wt + 2 * Ht * Wt,
            'undistort optical': 3 * Ho * Wo + 3 * Ho * Wo,
            'resize optical': 3 * Ho * Wo + 3 * oh * ow,
            # two reads for the exact order statistics (the frame does not fit the LDS), one for the output pass; clipped
            # uint16, fp32 and saved uint16 written
            'thermal rescale': 3 * 2 * Ht * Wt + (2 + 4 + 2) * Ht * Wt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--optical', type=int, nargs=2, default=[1200, 1600])
    ap.add_argument('--thermal', type=int, nargs=2, default=[512, 640])
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--runs', type=int, default=30)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_frames.py measures on the GPU only')
    from multipoint_amd.utils import frames as F
    import frames_restatement as R
    (Ho, Wo), (Ht, Wt), B = args.optical, args.thermal, args.batch
    rng = np.random.RandomState(0)
    base_o, base_t = R.smooth_bgr8(1, Ho, Wo), R.thermal_u16(2, Ht, Wt)
    optical = torch.from_numpy(np.stack([np.roll(base_o, 7 * b, 1) for b in range(B)])).cuda()
    thermal = np.stack([(base_t.astype(np.int64) + rng.randint(-40, 40, base_t.shape) + 50 * b).clip(0, 65535).astype(np.uint16)
                        for b in range(B)])
    thermal = torch.from_numpy(thermal.view(np.int16)).cuda().view(torch.uint16)
    calibration = R.calibration_of([('optical', R.DISTORTIONS[1]), ('thermal', R.DISTORTIONS[2])], (Ho, Wo), (Ht, Wt))
    params = {'undistort_images': True, 'image/undistort_alpha': 0.0, 'image/thermal/rotate': True,
              'image/optical/downscale': True, 'image/thermal/rescale_outlier_rejection': True}
    Ko, Do = F.camera_from_calibration(calibration, 'optical')
    Kt, Dt = F.camera_from_calibration(calibration, 'thermal')
    Kon, Ktn = F.optimal_new_camera_matrix(Ko, Do, (Wo, Ho), 0.0), F.optimal_new_camera_matrix(Kt, Dt, (Wt, Ht), 0.0)
    oh, ow = Ht, int(Wo * (float(Ht) / Ho))
    stages = {'undistort + rotate thermal': lambda: F.undistort(thermal, Kt, Dt, Ktn, rotate180=True),
              'undistort optical': lambda: F.undistort(optical, Ko, Do, Kon),
              'resize optical': lambda: F.resize_bgr8(optical, (oh, ow)),
              'thermal rescale': lambda: F.thermal_rescale(thermal),
              'prepare_frames': lambda: F.prepare_frames(optical, thermal, params, calibration)}
    model = bytes_model(Ho, Wo, Ht, Wt, oh, ow)
    model['prepare_frames'] = sum(model.values())
    res = {'device': torch.cuda.get_device_name(0), 'optical': [Ho, Wo], 'thermal': [Ht, Wt], 'resized': [oh, ow], 'batch': B,
           'runs': args.runs, 'timing': 'median (min, max) of `runs` calls after 5 warm-up calls, device events around each call, '
           'microseconds per PAIR; whole Python calls, output and workspace allocation included',
           'floor': 'bytes_model / 4 TB/s', 'per_pair': {}}
    try:
        res['commit'] = subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, text=True).strip()
    except Exception:
        res['commit'] = None
    for name, fn in stages.items():
        t = {k: v / B for k, v in median_us(fn, args.runs).items()}
        floor = model[name] / FLOOR_BYTES_PER_US
        res['per_pair'][name] = {'us': t, 'bytes_model': model[name], 'floor_us': floor, 'ratio_to_floor': t['median'] / floor,
                                 'achieved_TB_per_s': model[name] / t['median'] / 1e6}
        print(name, json.dumps(res['per_pair'][name]), flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
