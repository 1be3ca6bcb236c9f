"""Developer tool (GPU box): time of the similarity / affine estimates next to the homography's on the same lists.

    python tools/bench_transform.py [--calls 200] [--repeats 5] [--out FILE]

32 planted pairs that share one similarity, 1000 keypoints each of which 90 % are matched, 30 % outliers, T = 2000 hypotheses:
    pair      mp_find_transform on the 32 lists (RANSAC + refit), per model; 'homography' is mp_find_homography
    pooled    mp_find_transform_pooled on their ~29 000 pooled matches as one group; 'homography' is mp_find_homography_pooled
    refine    mp_refine_transform / _pooled (10 rounds; the homography's is its Levenberg-Marquardt polish)
After a warm-up every candidate is timed with device events around `--calls` back-to-back calls; the candidates ALTERNATE
inside each of the `--repeats` windows, so that a drift of the machine reaches all of them alike.  Prints one JSON line (min,
median, max microseconds per call) and writes it to --out if given."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import multipoint_amd.utils as U  # noqa: E402
import pooled_cases as C  # noqa: E402
import transform_cases as TC  # noqa: E402

P, K, T, OUTLIERS, HW, THR = 32, 1000, 2000, 0.3, (480, 640), 3.0
MODELS = ('homography', 'similarity', 'affine')


def window(f, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        f()
    e1.record(); e1.synchronize()
    return 1000.0 * e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_transform.py needs the GPU: a time taken elsewhere says nothing')
    rng = np.random.default_rng(0)
    hm = TC.random_model(rng, 'similarity')
    kp, cnt, midx, _ = C.planted_pairs(rng, P, K, *HW, OUTLIERS, sizes=[K] * P, shared=hm)
    res = C.to_results(kp, cnt, midx, *HW)
    pooled = U.pool_matches(res)
    cand, quality = {}, {}
    for m in MODELS:
        Hp, _, np_ = U.find_transform(res, m, THR, max_iters=T, seed=0)
        Hg, _, ng = U.find_transform_pooled(pooled, m, THR, max_iters=T, seed=0)
        cand['pair/' + m] = lambda m=m: U.find_transform(res, m, THR, max_iters=T, seed=0)
        cand['pooled/' + m] = lambda m=m: U.find_transform_pooled(pooled, m, THR, max_iters=T, seed=0)
        cand['refine_pair/' + m] = lambda m=m, Hp=Hp: U.refine_transform(res, Hp, m, THR, rounds=10)
        cand['refine_pooled/' + m] = lambda m=m, Hg=Hg: U.refine_transform_pooled(pooled, Hg, m, THR, rounds=10)
        quality[m] = {'pair_inliers_min': int(np_.min()), 'pooled_inliers': int(ng[0]),
                      'pooled_corner_error_px': round(float(C.corner_error(Hg[0].cpu().numpy(), hm, *HW)), 4)}
    for f in cand.values():                            # warm-up: code objects, allocator
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in cand}
    for _ in range(args.repeats):
        for k, f in cand.items():                      # alternating: every candidate once per window
            us[k].append(window(f, args.calls))
    rec = {'pairs': P, 'keypoints_per_pair': K, 'matches_pooled': int(pooled.pts.shape[0]), 'hypotheses': T,
           'outlier_fraction': OUTLIERS, 'calls': args.calls, 'repeats': args.repeats, 'quality': quality,
           'us_per_call_min_median_max': {k: [round(sorted(v)[0], 1), round(sorted(v)[len(v) // 2], 1), round(sorted(v)[-1], 1)]
                                          for k, v in us.items()}}
    line = json.dumps(rec, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'wt') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
