#!/usr/bin/env python3
"""Where pooling finds a peak that single pairs miss: the float64 restatement of the Fourier-Mellin registration
(tests/registration_restatement.py; no GPU) on sparse or noisy planted pairs, each pair alone and pooled in groups.

    python tools/register_pooling_study.py [--shapes 40] [--sigma 0.05] [--pairs 12]

The pairs are those of tests/registration_cases.py (72 x 96 thermal frames, 4 degrees, scale 0.78, shift (-6, 9)) with --shapes
shapes per scene and Gaussian noise of --sigma added to both frames (clipped to [0, 1]).  Prints the corner error of every single
pair, then of the pooled estimate of every 4 pairs and of all.  DESIGN.md 3.20 quotes the figures."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', type=int, default=40)
    ap.add_argument('--sigma', type=float, default=0.05)
    ap.add_argument('--pairs', type=int, default=12)
    args = ap.parse_args()
    import registration_cases as C
    import registration_restatement as R
    C.SHAPES = args.shapes
    cfg = ((72, 96), 4.0, 0.78, (-6.0, 9.0))
    rng = np.random.RandomState(5)
    optical, thermal = [], []
    for seed in range(300, 300 + args.pairs):
        o, t, T = C.make_pair(seed, *cfg)
        optical.append(np.clip(o + rng.randn(*o.shape) * args.sigma, 0, 1).astype(np.float32))
        thermal.append(np.clip(t + rng.randn(*t.shape) * args.sigma, 0, 1).astype(np.float32))
    optical, thermal = np.stack(optical), np.stack(thermal)
    e = R.estimate(optical, thermal)
    errs = [C.corner_error(e['T'][g], T) for g in range(args.pairs)]
    print('shapes %d sigma %g' % (args.shapes, args.sigma))
    print('single pairs within 1 px: %d of %d; corner errors %s' % (sum(x <= 1.0 for x in errs), args.pairs,
                                                                     ' '.join('%.1f' % x for x in errs)))
    for n in sorted({min(4, args.pairs), args.pairs}):
        for k in range(0, args.pairs - n + 1, n):
            e = R.estimate(optical[k:k + n], thermal[k:k + n], [0, n])
            p1, p2 = e['pk1'][0], e['pk2'][0]
            print('pooled, pairs %d..%d: corner error %.2f px, ratios %.2f %.2f, branch %d' % (
                k, k + n - 1, C.corner_error(e['T'][0], T), p1['peak'] / p1['second'], p2['peak'] / p2['second'], e['branch'][0]))


if __name__ == '__main__':
    main()
