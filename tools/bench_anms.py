#!/usr/bin/env python3
"""Time the spatially uniform top-k (adaptive non-maximal suppression) on the GPU with device events.

    python tools/bench_anms.py [--pairs 32] [--topk 1000] [--runs 20] [--out profiles/anms_bench.json]

  detect.score / detect.anms   utils.detect_keypoints on the heat maps of bench.py's own workload (the forward of its 2 x pairs
                               480 x 640 images, nms 4, threshold 0.015, top-k 1000), in the score mode and in the anms mode, the
                               fixed 8 NMS rounds of the pipeline; the same maps, the same session
  radii[n]                     mp_suppression_radii alone on 64 lists of n random candidates each (about 2 000, 8 000, 32 000)
Each figure is the median (min, max) of the timed calls after 3 warm-up calls, microseconds per CALL on the whole batch.
pair_steps: candidates squared, summed over the images -- what the all-pairs kernel compares.  There is no target and nothing to
compare with but the score mode's time of the same run: the figures are only recorded.  No CPU fallback: without a GPU this fails."""
import argparse
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
    ap.add_argument('--pairs', type=int, default=32)
    ap.add_argument('--topk', type=int, default=1000)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--robust', type=float, default=1.0)
    ap.add_argument('--candidates', type=int, nargs='*', default=[2000, 8000, 32000])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_anms.py measures on the GPU only')
    import bench
    import multipoint_amd.models as models
    import multipoint_amd.utils as U
    from multipoint_amd.datasets.synthetic_weights import SHIPPED_MODEL_CONFIG, make_weights
    dev = torch.device('cuda:0')
    pred = bench.PRED_CFG
    cfg = dict(SHIPPED_MODEL_CONFIG)
    net = models.MultiPoint(cfg); net.load_state_dict(make_weights(0, cfg)); net.to(dev); net.eval()
    images = bench.make_batch(list(range(args.pairs)), dev, bench.H, bench.W)
    with torch.no_grad():
        prob = net({'image': images, 'is_optical': (torch.arange(2 * args.pairs) % 2 == 0).reshape(-1, 1)})['prob']
    torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); out = fn(); b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3, out

    def stats(ts):
        ts = sorted(ts)
        return {'min': ts[0], 'median': ts[len(ts) // 2], 'max': ts[-1], 'n': len(ts)}

    def measure(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts, out = [], None
        for _ in range(args.runs):
            t, out = timed(fn)
            ts.append(t)
        return stats(ts), out

    kw = dict(keep_top_k=args.topk, capacity=args.topk, max_rounds=8)

    def score():
        return U.detect_keypoints(prob, pred['nms'], pred['detection_threshold'], **kw)

    def anms():
        return U.detect_keypoints(prob, pred['nms'], pred['detection_threshold'], topk_mode='anms', anms_robust=args.robust, **kw)

    # alternate the two modes so that neither owns a warmer machine
    ts, ta = [], []
    for _ in range(3):
        score(); anms()
    torch.cuda.synchronize()
    for i in range(args.runs):
        ts.append(timed(score)[0])
        ta.append(timed(anms)[0])
        print('run %d: score %.0f us, anms %.0f us' % (i, ts[-1], ta[-1]), file=sys.stderr, flush=True)
    survivors = U.detect_keypoints(prob, pred['nms'], pred['detection_threshold'], capacity=bench.H * bench.W // 4)[2].cpu().numpy()
    res = {'device': torch.cuda.get_device_name(0), 'frame': [bench.H, bench.W], 'images': 2 * args.pairs, 'topk': args.topk,
           'robust': args.robust,
           'timing': 'median (min, max) of the timed calls after 3 warm-up calls, device events around each call, microseconds per '
                     'CALL on the whole batch; measured on one box, in one session',
           'survivors_per_image': {'min': int(survivors.min()), 'median': float(np.median(survivors)), 'max': int(survivors.max())},
           'detect_pair_steps': int((survivors.astype(np.int64) ** 2).sum()),
           'detect_score_us': stats(ts), 'detect_anms_us': stats(ta),
           'detect_anms_minus_score_us': stats(ta)['median'] - stats(ts)['median'], 'radii': []}
    from multipoint_amd import _lib
    h = _lib.get_handle(dev)
    g = torch.Generator(device='cuda').manual_seed(3)
    B = 64
    for n in args.candidates:
        kp = torch.randint(0, 4096, (B, n, 2), generator=g, device=dev, dtype=torch.int32)
        sc = torch.rand((B, n), generator=g, device=dev) * 0.9 + 0.05
        cnt = torch.full((B,), n, dtype=torch.int32, device=dev)
        r2 = torch.empty((B, n), dtype=torch.int32, device=dev)

        def radii():
            h.check(h.lib.mp_suppression_radii(h.ptr, _lib.ptr(kp), _lib.ptr(sc), _lib.ptr(cnt), B, n, args.robust, _lib.ptr(r2),
                                               _lib.stream_ptr(dev)))
        st, _ = measure(radii)
        steps = B * n * n
        res['radii'].append({'lists': B, 'candidates': n, 'us': st, 'pair_steps': steps, 'gpair_steps_per_s': steps / st['median'] * 1e-3,
                             'undominated': int((r2 == -1).sum())})
        print('radii n=%d: %.0f us' % (n, st['median']), file=sys.stderr, flush=True)
    try:
        res['commit'] = subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, text=True,
                                                stderr=subprocess.DEVNULL).strip()
    except Exception:
        res['commit'] = None
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
