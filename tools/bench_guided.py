"""Developer tool (GPU box): what the guided matcher costs over the plain mutual one, and the times of the per-pair homography
estimate and its polish.

    python tools/bench_guided.py [--calls 200] [--repeats 3] [--out FILE.json]

Seeded unit descriptors with planted correspondences (tools/bench_match.py's construction), D = 256, two sizes: 32 pairs x
1000 rows and 4 pairs x 4096 rows.  Keypoints are scattered uniformly over a 480 x 640 frame; a planted row of B sits within
one pixel of its partner's position, the estimate is the identity.  Per size, after a warm-up, the candidates are timed with
device events around `--calls` back-to-back calls each, alternating, `--repeats` times:
    mutual      mp_match_mutual_nn
    guided_r6   mp_match_guided, radius 6   (a row has about 0.4 / 1.5 gated candidates at 1000 / 4096 rows)
    guided_r48  mp_match_guided, radius 48  (about 24 / 97)
    find        mp_find_homography on the radius-6 list, threshold 3 px, the default hypothesis count (lists of at most 3200 rows)
    polish      mp_refine_homography on the same list and find's estimate
Prints one JSON line per size: microseconds per call as [min, median, max] over the repeats and the ratio of the guided
medians to the mutual median of the same run."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multipoint_amd.pipeline import PairResults  # noqa: E402
from multipoint_amd.utils import find_homography, guided_pairs, match_pairs, refine_homography  # noqa: E402
from multipoint_amd.utils.evaluation import MAX_RANSAC_MATCHES  # noqa: E402

FRAME = (480, 640)


def make_inputs(P, K, D, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.nn.functional.normalize(torch.randn(P, K, D, generator=g), dim=2)
    B = torch.nn.functional.normalize(torch.randn(P, K, D, generator=g), dim=2)

    def scatter():
        return torch.stack([torch.randint(0, FRAME[0], (P, K), generator=g), torch.randint(0, FRAME[1], (P, K), generator=g)], 2)
    kpA, kpB = scatter(), scatter()
    n = (2 * K) // 3                                   # planted: noisy copies of rows of A at permuted positions of B
    for p in range(P):
        pos = torch.randperm(K, generator=g)[:n]; src = torch.randperm(K, generator=g)[:n]
        s = 0.9 * (0.2 + 1.8 * torch.rand(n, 1, generator=g))
        B[p, pos] = torch.nn.functional.normalize(A[p, src] + s * torch.randn(n, D, generator=g) / D ** 0.5, dim=1)
        jitter = torch.randint(-1, 2, (n, 2), generator=g)
        kpB[p, pos] = (kpA[p, src] + jitter).clamp_(min=0).minimum(torch.tensor(FRAME) - 1)
    # the interleaved lists of a PairResults: slot 2p = A, 2p + 1 = B
    desc = torch.stack([A, B], 1).reshape(2 * P, K, D).contiguous().cuda()
    kp = torch.stack([kpA, kpB], 1).reshape(2 * P, K, 2).to(torch.int32).contiguous().cuda()
    cnt = torch.full((2 * P,), K, dtype=torch.int32).cuda()
    return desc, kp, cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_guided.py needs the GPU: a time taken elsewhere says nothing')
    lines = []
    for P, K, D in ((32, 1000, 256), (4, 4096, 256)):
        desc, kp, cnt = make_inputs(P, K, D, 1000 + K)
        lay = dict(pair_stride=2 * K * D, count_stride=2)
        eye = torch.eye(3, dtype=torch.float64).repeat(P, 1, 1).cuda()

        def guided(radius):
            return guided_pairs(desc, cnt, desc[1:], cnt[1:], kp, kp[1:], eye, radius, **lay)
        cand = {'mutual': lambda: match_pairs(desc, cnt, desc[1:], cnt[1:], **lay),
                'guided_r6': lambda: guided(6.0), 'guided_r48': lambda: guided(48.0)}
        counts = {k: int(f()[2].sum()) for k, f in cand.items()}
        if K <= MAX_RANSAC_MATCHES:
            mi, md, mc = guided(6.0)
            res = PairResults(kp, None, cnt, desc, mi, md, mc, *FRAME, 'guided')
            est = find_homography(res, 3.0)[0]
            cand['find'] = lambda: find_homography(res, 3.0)
            cand['polish'] = lambda: refine_homography(res, est, 3.0)
            counts['polish_inliers'] = int(cand['polish']()[2].sum())
        for f in cand.values():                        # warm-up: code objects, workspace, allocator
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        us = {k: [] for k in cand}
        for _ in range(args.repeats):
            for name, f in cand.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    f()
                e1.record(); e1.synchronize()
                us[name].append(1000.0 * e0.elapsed_time(e1) / args.calls)
        stat = {k: [round(sorted(v)[0], 2), round(sorted(v)[len(v) // 2], 2), round(sorted(v)[-1], 2)] for k, v in us.items()}
        rec = {'pairs': P, 'rows': K, 'D': D, 'calls': args.calls, 'repeats': args.repeats, 'matches': counts,
               'us_per_call_min_median_max': stat,
               'ratio_to_mutual': {k: round(stat[k][1] / stat['mutual'][1], 3) for k in ('guided_r6', 'guided_r48')}}
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(lines, fh, indent=1)


if __name__ == '__main__':
    main()
