#!/usr/bin/env python3
"""Time the RIFT baseline (multipoint_amd.models.ClassicDetectors, method RIFT) on the GPU with device events, per
stage and per image, next to the LGHD orientation stage from the same session: the same forward transform and 24 half-transformed
complex planes, plus one extra row pass over six of them.

    python tools/bench_rift.py [--height 512 --width 640] [--batches 16] [--runs 20] [--out profiles/rift_bench.json]

Stages: phase congruency (forward FFT, 24 filtered inverse column passes, the amplitude pass, six exact medians, the row pass that
leaves M, m and the maximum index map), detect (range, 8-bit image, FAST score, non-maximum suppression + prob), keypoint lists,
describe.  Each figure is the median of --runs timed calls after warm-up, in microseconds per image.  The bytes the
phase-congruency stage has to move are counted from the shapes (bytes_model).  There is no CPU fallback: without a GPU this fails."""
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


def median_us(fn, runs, warmup=3):
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


def bytes_model(H, W):
    """bytes per image the phase-congruency stage moves, from the shapes"""
    px = H * W
    return {'forward (u8 in, spectrum out, in, out)': px + 3 * 8 * px,
            'inverse columns (spectrum + 24 filter planes in, 24 complex planes out)': 8 * px + 24 * 4 * px + 24 * 8 * px,
            'amplitude rows (6 complex planes in, 6 real planes out)': 6 * 8 * px + 6 * 4 * px,
            'medians (6 real planes, 4 digit passes and at most one more)': 5 * 6 * 4 * px,
            'moment rows (24 complex planes in, M, m and the index map out)': 24 * 8 * px + 2 * 4 * px + px}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=512)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--batches', type=int, nargs='+', default=[16])
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--patch-size', type=int, default=96)
    ap.add_argument('--fast-threshold', type=int, default=13)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_rift.py measures on the GPU only')
    from multipoint_amd.models import ClassicDetectors, classic_detectors as C
    from multipoint_amd.utils import utils as U
    import lghd_restatement as R
    H, W = args.height, args.width
    net = ClassicDetectors({'method': 'RIFT', 'patch_size': args.patch_size, 'fast_threshold': args.fast_threshold}).cuda().eval()
    bank = net.filter_bank(H, W, net.device)
    model = bytes_model(H, W)
    res = {'device': torch.cuda.get_device_name(0), 'height': H, 'width': W, 'runs': args.runs, 'patch_size': args.patch_size,
           'fast_threshold': args.fast_threshold, 'bytes_model': model, 'bytes_per_image': sum(model.values()),
           'hbm_floor_us_at_4TBps': sum(model.values()) / 4e12 * 1e6,
           'timing': 'median (min, max) of `runs` calls after 3 warm-up calls, device events around each call, microseconds per '
                     'IMAGE; whole Python calls, output and workspace allocation included', 'per_image_us': {}}
    try:
        res['commit'] = subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, text=True).strip()
    except Exception:
        res['commit'] = None
    for B in args.batches:
        images = torch.from_numpy(np.stack([R.smooth_image(b, H, W) if b % 2 else R.noise_image(b, H, W) for b in range(B)]))
        images = images[:, None].cuda()
        u8 = C.quantize(images).reshape(B, H, W)
        M, _, mim, _ = C.phase_congruency(u8, bank)
        _, _, _, prob = C.rift_detect(M, args.fast_threshold, args.patch_size)
        kp, _, cnt = U.extract_keypoints(prob, 0.015, capacity=4096)
        stages = {'phase congruency': lambda: C.phase_congruency(u8, bank),
                  'lghd orientation (yardstick)': lambda: C.orientation_maps(u8, bank),
                  'detect': lambda: C.rift_detect(M, args.fast_threshold, args.patch_size),
                  'keypoint lists': lambda: U.extract_keypoints(prob, 0.015, capacity=4096),
                  'describe': lambda: C.rift_describe(mim, kp, cnt, args.patch_size),
                  'forward (phase congruency + detect)': lambda: net({'image': images})}
        row = {k: {s: v / B for s, v in median_us(fn, args.runs).items()} for k, fn in stages.items()}
        row['keypoints per image'] = float(cnt.float().clamp(max=4096).mean())
        res['per_image_us'][B] = row
        print(B, json.dumps(row), flush=True)
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
