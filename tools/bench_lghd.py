#!/usr/bin/env python3
"""Time the LGHD baseline (multipoint_amd.models.ClassicDetectors) on the GPU with device events, per stage and per image, next to
the numpy restatement (tests/lghd_restatement.py) on the host for scale.

    python tools/bench_lghd.py [--height 512 --width 640] [--batches 1 16] [--runs 20] [--cpu-runs 1] [--out profiles/lghd_bench.json]

Stages: quantise, FAST (score + non-maximum suppression + prob), orientation maps (forward FFT, 24 filtered inverse FFTs, arg-max),
keypoint lists (the existing threshold extraction), describe.  Each figure is the median of --runs timed calls after warm-up, in
microseconds per image.  The bytes the orientation stage has to move are counted from the shapes (bytes_model); the achieved rate
of its kernels comes from a kernel trace of this script (`--trace-only`: the stage alone, a few times, for a profiler run of its
own).  There is no CPU fallback: without a GPU this fails."""
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
    """bytes per image the orientation stage moves, from the shapes"""
    px = H * W
    return {'forward (u8 in, spectrum out, in, out)': px + 3 * 8 * px,
            'inverse columns (spectrum + 24 filter planes in, 24 complex planes out)': 8 * px + 24 * 4 * px + 24 * 8 * px,
            'inverse rows (24 complex planes in, 4 index planes out)': 24 * 8 * px + 4 * px}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=512)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 16])
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--cpu-runs', type=int, default=1)
    ap.add_argument('--trace-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_lghd.py measures on the GPU only')
    from multipoint_amd.models import ClassicDetectors, classic_detectors as C
    from multipoint_amd.utils import utils as U
    import lghd_restatement as R
    H, W = args.height, args.width
    net = ClassicDetectors({'method': 'LGHD'}).cuda().eval()
    bank = net.filter_bank(H, W, net.device)
    if args.trace_only:
        u8 = C.quantize(torch.from_numpy(np.stack([R.noise_image(b, H, W) for b in range(4)])).cuda())
        for _ in range(5):
            C.orientation_maps(u8, bank)
        torch.cuda.synchronize()
        return
    res = {'device': torch.cuda.get_device_name(0), 'height': H, 'width': W, 'runs': args.runs, 'bytes_model': bytes_model(H, W),
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
        _, _, prob = C.fast_detect(u8)
        ori = C.orientation_maps(u8, bank)
        kp, _, cnt = U.extract_keypoints(prob, 0.5, capacity=4096)
        stages = {'quantise': lambda: C.quantize(images), 'fast': lambda: C.fast_detect(u8),
                  'orientation': lambda: C.orientation_maps(u8, bank),
                  'keypoint lists': lambda: U.extract_keypoints(prob, 0.5, capacity=4096),
                  'describe': lambda: C.describe(ori, kp, cnt)}
        if B > 1:
            stages['forward (all but lists + describe)'] = lambda: net({'image': images})
        row = {k: {s: v / B for s, v in median_us(fn, args.runs).items()} for k, fn in stages.items()}
        row['keypoints per image'] = float(cnt.float().mean())
        res['per_image_us'][B] = row
        print(B, json.dumps(row), flush=True)
    cpu = {}
    u8 = R.quantize(R.noise_image(0, H, W))
    for name, fn in (('filter bank (once per frame size)', lambda: R.filter_bank(H, W)),):
        t0 = time.perf_counter(); bank64 = fn(); cpu[name] = (time.perf_counter() - t0) * 1e6
    t = []
    for _ in range(max(args.cpu_runs, 1)):
        t0 = time.perf_counter()
        kp, desc, _ = R.detect_and_compute(u8, bank64)
        t.append((time.perf_counter() - t0) * 1e6)
    cpu['detect_and_compute per image'] = sorted(t)[len(t) // 2]
    cpu['keypoints'] = len(kp)
    cpu['threads'] = os.environ.get('OMP_NUM_THREADS')
    res['cpu_restatement_us'] = cpu
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
