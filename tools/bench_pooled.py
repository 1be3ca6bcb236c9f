"""Developer tool (GPU box): time of the pooled homography estimate.

    python tools/bench_pooled.py [--calls 20] [--repeats 3] [--oracle-iters 100] [--out profiles/pooled_homography.json]

256 planted pairs that share one homography, 1000 keypoints each of which 90 % are matched (N ~ 230 000 pooled matches),
30 % outliers, T = 2000 hypotheses.  After a warm-up the three steps are timed with device events around `--calls`
back-to-back calls each, `--repeats` times:
    pool      mp_pool_matches (count, scan, ordered write) -- without the one host read of N that utils.pool_matches adds
    find      mp_find_homography_pooled (score T x N, select, refit)
    polish    mp_refine_homography_pooled
For context the oracle's CPU restatement of the same algorithm (oracle.ransac_homography, numpy) is timed on the host for
`--oracle-iters` hypotheses and scaled to T.  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import multipoint_amd.utils as U  # noqa: E402
import pooled_cases as C  # noqa: E402

P, K, T, OUTLIERS, HW = 256, 1000, 2000, 0.3, (480, 640)


def timed(f, calls, repeats):
    us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            f()
        e1.record(); e1.synchronize()
        us.append(1000.0 * e0.elapsed_time(e1) / calls)
    us.sort()
    return [round(us[0], 1), round(us[len(us) // 2], 1), round(us[-1], 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--oracle-iters', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pooled_homography.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_pooled.py needs the GPU: a time taken elsewhere says nothing')
    rng = np.random.default_rng(0)
    hm = C.random_homography(rng)
    kp, cnt, midx, _ = C.planted_pairs(rng, P, K, *HW, OUTLIERS, sizes=[K] * P, shared=hm)
    res = C.to_results(kp, cnt, midx, *HW)
    pooled = U.pool_matches(res)
    N = pooled.pts.shape[0]
    Hm, mask, nin = U.find_homography_pooled(pooled, 3.0, max_iters=T, seed=0)
    cand = {'pool': lambda: pool_only(res),
            'find': lambda: U.find_homography_pooled(pooled, 3.0, max_iters=T, seed=0),
            'polish': lambda: U.refine_homography_pooled(pooled, Hm, 3.0)}
    for f in cand.values():                            # warm-up: code objects, allocator
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    us = {k: timed(f, args.calls, args.repeats) for k, f in cand.items()}
    pts = pooled.pts.cpu().numpy()
    from oracle import mp_oracle
    t0 = time.perf_counter()
    mp_oracle.ransac_homography(pts[:, :2], pts[:, 2:], 3.0, args.oracle_iters, 0, 0)
    oracle_s = time.perf_counter() - t0
    R, _, rn, cost = U.refine_homography_pooled(pooled, Hm, 3.0)
    rec = {'pairs': P, 'keypoints_per_pair': K, 'matches_pooled': int(N), 'hypotheses': T, 'outlier_fraction': OUTLIERS,
           'calls': args.calls, 'repeats': args.repeats, 'inliers': int(nin[0]),
           'corner_error_px': {'refit': round(float(C.corner_error(Hm[0].cpu().numpy(), hm, *HW)), 4),
                               'polished': round(float(C.corner_error(R[0].cpu().numpy(), hm, *HW)), 4)},
           'us_per_call_min_median_max': us,
           'oracle_host': {'hypotheses': args.oracle_iters, 'seconds': round(oracle_s, 2),
                           'seconds_scaled_to_T': round(oracle_s * T / args.oracle_iters, 1)}}
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(rec, fh, indent=1)


_pool_buffers = {}


def pool_only(res):
    """mp_pool_matches into buffers allocated once: the launches alone, without the read of N."""
    import ctypes
    from multipoint_amd import _lib
    dev = res.kp_yx.device
    Pn, Kn = res.num_pairs, res.kp_yx.shape[1]
    b = _pool_buffers
    if not b:
        h = _lib.get_handle(dev)
        n = ctypes.c_longlong()
        h.check(h.lib.mp_pooled_workspace_bytes(Pn, 1, 1, ctypes.byref(n)))
        b.update(h=h, pts=torch.empty((Pn * Kn, 4), device=dev), q=torch.empty(Pn * Kn, dtype=torch.int32, device=dev),
                 po=torch.empty(Pn + 1, dtype=torch.int32, device=dev), go=torch.empty(2, dtype=torch.int32, device=dev),
                 ws=torch.empty(max(n.value, 16), dtype=torch.uint8, device=dev))
    h = b['h']
    h.check(h.lib.mp_pool_matches(h.ptr, _lib.ptr(res.kp_yx), _lib.ptr(res.kp_count), _lib.ptr(res.match_idx), None, Pn, Kn, 1,
                                  _lib.ptr(b['pts']), _lib.ptr(b['q']), Pn * Kn, _lib.ptr(b['po']), _lib.ptr(b['go']),
                                  _lib.ptr(b['ws']), b['ws'].numel(), _lib.stream_ptr(dev)))


if __name__ == '__main__':
    main()
