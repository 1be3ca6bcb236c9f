"""GPU: the matchers at descriptor width 384 (the LGHD baseline's) against a float64 brute force on unit rows: mutual nearest
neighbours, the one-way and ratio modes, the guided matcher and the scalar route of get_matches.  Indices must agree wherever
the float64 best-to-second gap exceeds 1e-5, distances within 1e-6.  K = 70 is no multiple of the 32-row tiles, one pair has an
empty list on either side."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
D, K = 384, 70
PAIRS = [(70, 45), (33, 64), (37, 0), (0, 20), (1, 1)]           # (rows of A, rows of B)
GAP, DTOL = 1e-5, 1e-6


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _pair(case):
    """Unit Gaussian rows; two thirds of the shorter list are noisy copies of rows of the other one (the generator of
    tests/test_gpu_match_modes.py with the noise floor raised from 0.18 to 0.54), so nearest distances spread from about 0.5
    to 1.4.  The floor follows from the number format, not from the kernel: d = sqrt(2 - 2 t) turns an error e of the dot
    product t into e / d, and ANY fp32 accumulation of 384 products in ascending k leaves e up to about 5e-7 where the partial
    sums approach 1 (2^-24 per addition, 384 additions); 1e-6 on d is therefore only meaningful for d >= 0.5.
    test_inputs_admit_the_distance_bound checks that with a plain numpy fp32 accumulation."""
    N, M = PAIRS[case]
    rng = np.random.default_rng(384 + case)
    A = _unit(rng.standard_normal((N, D))) if N else np.zeros((0, D), np.float32)
    B = _unit(rng.standard_normal((M, D))) if M else np.zeros((0, D), np.float32)
    n_pl = (2 * min(N, M)) // 3
    if n_pl:
        pos = rng.permutation(M)[:n_pl]; src = rng.permutation(N)[:n_pl]
        s = 0.9 * rng.uniform(0.6, 2.0, (n_pl, 1))
        B[pos] = _unit(A[src].astype(np.float64) + s * rng.standard_normal((n_pl, D)) / np.sqrt(D))
    return A, B


def _brute(A, B, allowed=None):
    """float64: (dist [N, M], best [N], second [N], decided [N]: the best-to-second gap exceeds GAP); `allowed` masks candidates"""
    d = np.sqrt(2.0 - 2.0 * np.clip(A.astype(np.float64) @ B.astype(np.float64).T, -1.0, 1.0))
    if allowed is not None:
        d = np.where(allowed, d, np.inf)
    N, M = d.shape
    order = np.argsort(d, axis=1, kind='stable')
    best = order[:, 0] if M else np.full(N, -1)
    second = order[:, 1] if M > 1 else np.full(N, -1)
    rows = np.arange(N)
    gap = d[rows, second] - d[rows, best] if M > 1 else np.full(N, np.inf)
    gap = np.where(np.isnan(gap), np.inf, gap)                     # (inf - inf: fewer than two candidates)
    return d, best, second, gap > GAP


@pytest.fixture(scope='module')
def data():
    prs = [_pair(c) for c in range(len(PAIRS))]
    P = len(prs)
    a = np.zeros((P, K, D), np.float32); b = np.zeros((P, K, D), np.float32)
    na = np.zeros(P, np.int32); nb = np.zeros(P, np.int32)
    for p, (A, B) in enumerate(prs):
        a[p, :len(A)] = A; b[p, :len(B)] = B; na[p], nb[p] = len(A), len(B)
    dev = [torch.from_numpy(x).to(DEV) for x in (a, na, b, nb)]
    return prs, dev


def test_inputs_admit_the_distance_bound(data):
    """A condition on the inputs, no kernel involved: sqrt(2 - 2 t) with t accumulated in fp32 in ascending k by numpy lies within
    DTOL of the float64 distance for every pair of rows."""
    prs, _ = data
    for A, B in prs:
        if not len(A) or not len(B):
            continue
        acc = np.zeros((len(A), len(B)), np.float32)
        for k in range(D):
            acc = acc + A[:, k:k + 1] * B[:, k][None, :]
        assert acc.dtype == np.float32
        d32 = np.sqrt(np.float32(2) - np.float32(2) * np.clip(acc, -1, 1))
        err = np.abs(d32 - _brute(A, B)[0]).max()
        print('%d x %d: numpy fp32 distances within %.3g of float64' % (len(A), len(B), err))
        assert err <= DTOL


def _check_mutual(prs, midx, mdist, mcnt, allowed=None, threshold=None):
    for p, (A, B) in enumerate(prs):
        N, M = len(A), len(B)
        assert (midx[p, N:] == -1).all() and (mdist[p, N:] == 0).all()
        if N == 0 or M == 0:
            assert mcnt[p] == 0 and (midx[p] == -1).all()
            continue
        al = None if allowed is None else allowed[p]
        d, best, _, dec_r = _brute(A, B, al)
        dT, bestT, _, dec_c = _brute(B, A, None if al is None else al.T)
        has = np.isfinite(d[np.arange(N), best])
        # row i is decided when its own arg-min and the arg-min of its best column are
        decided = dec_r & (~has | dec_c[np.where(has, best, 0)])
        want = np.where(has & (bestT[np.where(has, best, 0)] == np.arange(N)), best, -1)
        if threshold is not None:
            dd = d[np.arange(N), np.where(has, best, 0)]
            want = np.where(dd < threshold, want, -1)
            decided &= np.abs(dd - threshold) > GAP
        got = midx[p, :N]
        print('pair %d (%d x %d): %d of %d rows decided, %d matches' % (p, N, M, decided.sum(), N, (got >= 0).sum()))
        assert decided.mean() >= 0.9
        assert np.array_equal(got[decided], want[decided])
        hit = got >= 0
        err = np.abs(mdist[p, :N][hit] - d[np.arange(N)[hit], got[hit]])
        print('    max |distance - float64| = %.3g' % err.max(initial=0))
        assert err.max(initial=0) <= DTOL
        assert (mdist[p, :N][~hit] == 0).all()
        assert mcnt[p] == hit.sum()


def test_mutual_nearest_neighbours(data):
    from multipoint_amd.utils.matching import match_pairs
    prs, (a, na, b, nb) = data
    out = [o.cpu().numpy() for o in match_pairs(a, na, b, nb)]
    _check_mutual(prs, *out)
    again = [o.cpu().numpy() for o in match_pairs(a, na, b, nb)]
    assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(out, again))
    thr = [o.cpu().numpy() for o in match_pairs(a, na, b, nb, threshold=0.9)]
    _check_mutual(prs, *thr, threshold=0.9)


def test_mutual_on_interleaved_lists(data):
    """the layout PairPipeline matches in place: slot 2p against slot 2p + 1"""
    from multipoint_amd.utils.matching import match_pairs
    prs, (a, na, b, nb) = data
    P = len(prs)
    t = torch.stack((a, b), 1).reshape(2 * P, K, D).contiguous()
    c = torch.stack((na, nb), 1).reshape(2 * P).contiguous()
    out = [o.cpu().numpy() for o in match_pairs(t, c, t[1:], c[1:], pair_stride=2 * K * D, count_stride=2)]
    want = [o.cpu().numpy() for o in match_pairs(a, na, b, nb)]
    assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(out, want))


def test_one_way_and_ratio(data):
    from multipoint_amd.utils.matching import nearest_pairs
    prs, (a, na, b, nb) = data
    near = [o.cpu().numpy() for o in nearest_pairs(a, na, b, nb, return_second=True)]
    rat = [o.cpu().numpy() for o in nearest_pairs(a, na, b, nb, ratio=0.9)]
    for p, (A, B) in enumerate(prs):
        N, M = len(A), len(B)
        midx, mdist, mcnt, sidx, sdist = (x[p] for x in near)
        ridx, rdist, rcnt = (x[p] for x in rat)
        assert (midx[N:] == -1).all() and (ridx[N:] == -1).all() and (sidx[N:] == -1).all()
        if N == 0 or M == 0:
            assert mcnt == 0 and rcnt == 0 and (midx == -1).all() and (ridx == -1).all()
            continue
        d, best, second, decided = _brute(A, B)
        rows = np.arange(N)
        assert mcnt == N and np.array_equal(midx[:N][decided], best[decided])
        assert np.abs(mdist[:N] - d[rows, midx[:N]]).max() <= DTOL
        if M == 1:
            assert (sidx[:N] == -1).all() and rcnt == 0
            continue
        third = np.sort(d, axis=1)[:, 2] if M > 2 else np.full(N, np.inf)
        dec2 = decided & (third - d[rows, second] > GAP)
        assert np.array_equal(sidx[:N][dec2], second[dec2])
        assert np.abs(sdist[:N] - d[rows, sidx[:N]]).max() <= DTOL
        keep = d[rows, best] < 0.9 * d[rows, second]
        clear = np.abs(d[rows, best] - 0.9 * d[rows, second]) > GAP
        print('pair %d: ratio test keeps %d of %d, %d clear of the boundary' % (p, keep.sum(), N, clear.sum()))
        assert clear.mean() >= 0.9
        assert np.array_equal((ridx[:N] >= 0)[clear], keep[clear])
        k = clear & keep & decided
        assert np.array_equal(ridx[:N][k], best[k])
        assert np.abs(rdist[:N][ridx[:N] >= 0] - d[rows, ridx[:N]][ridx[:N] >= 0]).max(initial=0) <= DTOL


def test_guided(data):
    """mutual nearest neighbours inside a gate: keypoints on a grid, identity homography, radius 6 pixels"""
    from multipoint_amd.utils.matching import guided_pairs
    prs, (a, na, b, nb) = data
    P = len(prs)
    rng = np.random.default_rng(7)
    kpa = rng.integers(0, 40, (P, K, 2)).astype(np.int32); kpb = rng.integers(0, 40, (P, K, 2)).astype(np.int32)
    hom = np.tile(np.eye(3), (P, 1, 1))
    radius = 12.0
    out = [o.cpu().numpy() for o in guided_pairs(a, na, b, nb, torch.from_numpy(kpa).to(DEV), torch.from_numpy(kpb).to(DEV), hom,
                                                 radius)]
    allowed = []
    for p, (A, B) in enumerate(prs):
        pa = kpa[p, :len(A)].astype(np.float64); pb = kpb[p, :len(B)].astype(np.float64)
        allowed.append(((pa[:, None, :] - pb[None, :, :]) ** 2).sum(-1) <= radius * radius)      # integers: exact in fp32 too
    _check_mutual(prs, *out, allowed=allowed)
    assert 0 < out[2][0] < 45


def test_scalar_route(data):
    """utils.get_matches without crossCheck (mp_match_knn2: true L2 distances in LDS) and thresholdmatcher at width 384"""
    from multipoint_amd.utils.matching import get_matches
    prs, _ = data
    for p in (0, 1, 2):
        A, B = prs[p]
        N, M = len(A), len(B)
        got = get_matches(A, B, 'bfmatcher', False, crossCheck=False)
        if M == 0:
            assert got == []
            continue
        d, best, _, decided = _brute(A, B)
        assert [m.queryIdx for m in got] == list(range(N))
        tr = np.array([m.trainIdx for m in got]); ds = np.array([m.distance for m in got])
        assert np.array_equal(tr[decided], best[decided])
        # || a - b || of unit rows is the same distance; fp32 rows are unit within 6e-8, which the 1e-6 covers
        assert np.abs(ds - d[np.arange(N), tr]).max() <= DTOL
        thr = get_matches(A, B, 'thresholdmatcher', False, threshold=0.8)
        near = np.abs(d - 0.8) <= GAP
        want = {(i, j) for i, j in np.argwhere(d < 0.8) if not near[i, j]}
        have = {(m.queryIdx, m.trainIdx) for m in thr if not near[m.queryIdx, m.trainIdx]}
        assert have == want and len(want) > 5
        cross = get_matches(A, B, 'bfmatcher', False, crossCheck=True)
        assert len(cross) > 10 and all(abs(m.distance - d[m.queryIdx, m.trainIdx]) <= DTOL for m in cross)
