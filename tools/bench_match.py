"""Developer tool (GPU box): time of the ratio-test matcher against the routes it replaces or is built from.

    python tools/bench_match.py [--calls 200] [--repeats 3] [--out FILE.json]

Seeded unit descriptors with planted correspondences, D = 64, two sizes: 32 pairs x 1000 rows (a benchmark batch at
topk 1000) and 4 pairs x 4096 rows (the shipped `topk: 0` capacity).  Per size, after a warm-up, three candidates are
timed with device events around `--calls` back-to-back calls each, alternating, `--repeats` times:
    nearest   mp_match_nearest, ratio 0.9 (one direction, two nearest, ratio test fused into its epilogue launch)
    knn2      mp_match_knn2 + the ratio test on its [P][K][2] output as device tensor operations
    mutual    mp_match_mutual_nn (both directions)
Prints one JSON line per size: microseconds per call as [min, median, max] over the repeats, and how many query rows
the two ratio-test routes decide differently (their distances are rounded differently: MFMA dot product against a sum
of squared differences)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multipoint_amd.utils import knn2_pairs, match_pairs, nearest_pairs  # noqa: E402

RATIO = 0.9


def make_inputs(P, K, D, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.nn.functional.normalize(torch.randn(P, K, D, generator=g), dim=2)
    B = torch.nn.functional.normalize(torch.randn(P, K, D, generator=g), dim=2)
    n = (2 * K) // 3                                   # planted: noisy copies of rows of A at permuted positions of B
    for p in range(P):
        pos = torch.randperm(K, generator=g)[:n]; src = torch.randperm(K, generator=g)[:n]
        s = 0.9 * (0.2 + 1.8 * torch.rand(n, 1, generator=g))
        B[p, pos] = torch.nn.functional.normalize(A[p, src] + s * torch.randn(n, D, generator=g) / D ** 0.5, dim=1)
    cnt = torch.full((P,), K, dtype=torch.int32)
    return A.cuda(), cnt.cuda(), B.cuda(), cnt.clone().cuda()


def ratio_on_knn2(A, nA, B, nB):
    idx, dist = knn2_pairs(A, nA, B, nB)
    keep = (idx[..., 1] >= 0) & (dist[..., 0].double() < RATIO * dist[..., 1].double())
    return torch.where(keep, idx[..., 0], torch.full_like(idx[..., 0], -1)), keep.sum(1, dtype=torch.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_match.py needs the GPU: a time taken elsewhere says nothing')
    lines = []
    for P, K, D in ((32, 1000, 64), (4, 4096, 64)):
        A, nA, B, nB = make_inputs(P, K, D, 1000 + K)
        cand = {'nearest': lambda: nearest_pairs(A, nA, B, nB, ratio=RATIO),
                'knn2': lambda: ratio_on_knn2(A, nA, B, nB),
                'mutual': lambda: match_pairs(A, nA, B, nB)}
        for f in cand.values():                        # warm-up: code objects, workspace, allocator
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        near = nearest_pairs(A, nA, B, nB, ratio=RATIO)[0]
        differ = int(((near >= 0) != (ratio_on_knn2(A, nA, B, nB)[0] >= 0)).sum())
        us = {k: [] for k in cand}
        for _ in range(args.repeats):
            for name, f in cand.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    f()
                e1.record(); e1.synchronize()
                us[name].append(1000.0 * e0.elapsed_time(e1) / args.calls)
        rec = {'pairs': P, 'rows': K, 'D': D, 'calls': args.calls, 'repeats': args.repeats,
               'ratio_kept': int((near >= 0).sum()), 'ratio_decisions_differing_from_knn2': differ,
               'us_per_call_min_median_max': {k: [round(sorted(v)[0], 2), round(sorted(v)[len(v) // 2], 2),
                                                   round(sorted(v)[-1], 2)] for k, v in us.items()}}
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(lines, fh, indent=1)


if __name__ == '__main__':
    main()
