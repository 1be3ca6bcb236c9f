#!/usr/bin/env python3
"""Photometric augmentation (mp_photometric_augment) for 64 images of 240x320 with the primitives and parameters of the
reference's training config (configs/config_multipoint_training.yaml), random order: the device time of one batch in
each noise mode (hipEvents on the stream around the launch, after warm-up; median of --reps), and the host time of
drawing the 64 plans in each mode (for 'host' noise: the two 240x320 float64 fields per image) and of uploading the
host-mode fields.

    python tools/bench_photometric.py [--reps 30] [--json out.json]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multipoint_amd.datasets import augmentation as A  # noqa: E402

DEV = torch.device('cuda:0')
TRAIN = {'primitives': ['random_brightness', 'random_contrast', 'additive_speckle_noise', 'additive_gaussian_noise',
                        'additive_shade', 'motion_blur'],
         'params': {'random_brightness': {'max_abs_change': 0.15}, 'random_contrast': {'strength_range': [0.3, 1.8]},
                    'additive_gaussian_noise': {'stddev_range': [0, 0.06]},
                    'additive_speckle_noise': {'prob_range': [0, 0.0035]},
                    'additive_shade': {'transparency_range': [-0.5, 0.8], 'kernel_size_range': [50, 100]},
                    'motion_blur': {'max_kernel_size': 3}},
         'random_order': True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    B, H, W = args.batch, 240, 320
    imgs = torch.from_numpy(np.random.default_rng(0).random((B, 1, H, W), dtype=np.float32)).to(DEV)
    out = torch.empty_like(imgs)
    res = {'batch': B, 'height': H, 'width': W, 'reps': args.reps}
    for noise in ('host', 'device'):
        random.seed(0); np.random.seed(0)
        t0 = time.perf_counter()
        plans = [A.draw_photometric_plan((H, W), dict(TRAIN, noise=noise)) for _ in range(B)]
        t_draw = time.perf_counter() - t0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prep = A.prepare_photometric(plans, H, W, DEV)
        torch.cuda.synchronize()
        t_prep = time.perf_counter() - t0
        for _ in range(args.warmup):
            A.launch_photometric(prep, imgs, out)
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            A.launch_photometric(prep, imgs, out)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        res[noise] = {'device_ms_median': float(np.median(ms)), 'device_ms_min': float(np.min(ms)),
                      'host_draw_ms': t_draw * 1e3, 'prepare_upload_ms': t_prep * 1e3}
        print('%-6s noise: device %.3f ms / batch (median of %d, min %.3f); host plan draws %.1f ms; prepare + field '
              'upload %.1f ms' % (noise, np.median(ms), args.reps, np.min(ms), t_draw * 1e3, t_prep * 1e3), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
