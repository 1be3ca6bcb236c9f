#!/usr/bin/env python3
"""Time the result views (multipoint_amd.utils.drawing, csrc/draw.hip) on the GPU with device events, next to the bytes each
one has to move.

    python tools/bench_drawing.py [--shape 480 640] [--batch 32] [--marks 1000] [--runs 30] [--out profiles/drawing_bench.json]

Entries: gray_to_rgb of `batch` frames; draw_keypoints of `marks` rings per frame on canvases that exist; draw_pair_results of
`batch` pairs with `marks` matches each (two grey conversions, the owner map cleared, filled and resolved).  Each figure is the
median of --runs timed calls after warm-up, in microseconds per call, whole Python calls with output allocation included.
bytes_model counts what an entry must read and write once, from the shapes; `floor_us` is that over 4 TB/s.  There is no CPU
fallback: without a GPU this fails."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=2, default=[480, 640])
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--marks', type=int, default=1000)
    ap.add_argument('--runs', type=int, default=30)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_drawing.py measures on the GPU only')
    from multipoint_amd.pipeline import PairPipeline, PairResults
    from multipoint_amd.utils import drawing as D
    (H, W), B, K = args.shape, args.batch, args.marks
    rng = np.random.default_rng(0)
    dev = torch.device('cuda', torch.cuda.current_device())
    frames = torch.from_numpy(rng.random((B, 1, H, W), dtype=np.float32)).to(dev)
    other = torch.from_numpy(rng.random((B, 1, H, W), dtype=np.float32)).to(dev)
    kp = torch.from_numpy(np.stack([rng.integers(0, H, (2 * B, K)), rng.integers(0, W, (2 * B, K))], -1).astype(np.int32)).to(dev)
    counts = torch.full((2 * B,), K, dtype=torch.int32, device=dev)
    canvas = D.gray_to_rgb(frames)
    res = PairResults(kp, None, counts, None, torch.from_numpy(np.stack([rng.permutation(K) for _ in range(B)]).astype(np.int32)).to(dev),
                      None, None, H, W)
    images = PairPipeline.interleave(frames, other)
    px = B * H * W
    entries = {'gray_to_rgb': (lambda: D.gray_to_rgb(frames), 4 * px + 3 * px),
               'draw_keypoints': (lambda: D.draw_keypoints(canvas, kp[:B], counts[:B], radius=4), 8 * B * K),
               # two grey conversions into the (H, 2 W) canvas, the owner map written (memset), read and the canvas touched
               'draw_pair_results': (lambda: D.draw_pair_results(res, images), 2 * (4 * px + 3 * px) + 2 * 4 * 2 * px)}
    out = {'device': torch.cuda.get_device_name(0), 'shape': [H, W], 'batch': B, 'marks': K, 'runs': args.runs,
           'timing': 'median (min, max) of `runs` calls after 5 warm-up calls, device events around each call, microseconds per '
           'call; whole Python calls, output allocation included', 'floor': 'bytes_model / 4 TB/s', 'per_call': {}}
    try:
        out['commit'] = subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, text=True).strip()
    except Exception:
        out['commit'] = None
    for name, (fn, model) in entries.items():
        t = median_us(fn, args.runs)
        out['per_call'][name] = {'us': t, 'bytes_model': model, 'floor_us': model / FLOOR_BYTES_PER_US}
        print(name, json.dumps(out['per_call'][name]), flush=True)
    print(json.dumps(out))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
