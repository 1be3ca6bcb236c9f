#!/usr/bin/env python3
"""Time the SIFT baseline (multipoint_amd.models.classic_detectors, `implementation: restated`) on the GPU with device events:
one forward (detect + describe) and its stages, per image.

    python tools/bench_sift.py [--height 480 --width 640] [--batch 32] [--runs 20] [--out profiles/sift_bench.json]

Stages: scale space (Gaussian + difference pyramids), detect (candidates, refinement + orientation, selection; on the pyramids
already in the workspace), describe, scatter.  `forward` is the model's whole call, quantisation and allocations included.  Each
figure is the median (min, max) of --runs timed calls after 3 warm-up calls, in microseconds per image.  Frames are the seeded
structured images of tests/sift_cases.py.  There is no CPU fallback: without a GPU this fails."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sift.py measures on the GPU only')
    from multipoint_amd.models import ClassicDetectors, classic_detectors as S
    import sift_cases as C
    H, W, B = args.height, args.width, args.batch
    images = torch.from_numpy(np.stack([C.structured_image(H, W, seed=b) for b in range(B)]))[:, None].cuda()
    net = ClassicDetectors({'method': 'SIFT', 'implementation': 'restated'}).cuda().eval()
    u8 = S.quantize(images).reshape(B, H, W)
    ws = S.SiftWorkspace(B, H, W, S.sift_capacity(H, W), u8.device)
    kp, count, flags, _ = S.sift_detect(u8, workspace=ws)
    cand, ncand = ws.candidates()
    _, nlist = ws.oriented()
    stages = {'forward': lambda: net({'image': images}),
              'scale space': lambda: S.sift_scale_space(u8, workspace=ws),
              'detect': lambda: S.sift_detect(None, workspace=ws),
              'describe': lambda: S.sift_describe(ws, kp, count),
              'scatter': lambda: S.sift_scatter(kp, count, H, W)}
    res = {'device': torch.cuda.get_device_name(0), 'height': H, 'width': W, 'batch': B, 'runs': args.runs,
           'timing': 'median (min, max) of `runs` calls after 3 warm-up calls, device events around each call, microseconds per '
                     'IMAGE; whole Python calls, output allocation included',
           'workspace_bytes': ws.nbytes, 'capacity': ws.capacity,
           'per_image': {'candidates': float(ncand.float().mean()), 'oriented keypoints': float(nlist.float().mean()),
                         'kept keypoints': float(count.float().mean()), 'flags': int(flags.max())}}
    try:
        res['commit'] = subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        res['commit'] = None
    res['per_image_us'] = {k: {s: v / B for s, v in median_us(fn, args.runs).items()} for k, fn in stages.items()}
    print(json.dumps(res))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
