"""GPU (MI355X): the pooled homography estimate (mp_pool_matches, mp_find_homography_pooled, mp_refine_homography_pooled)
against the per-pair kernels it shares its device functions with, against the oracle's CPU restatement of the algorithm
(oracle.ransac_homography with pair_index := group index) and against planted models."""
import ctypes

import numpy as np
import pytest
import torch

import pooled_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HW = (480, 640)


def _tol(Ho):
    return 1e-6 * max(1.0, np.abs(Ho).max())


def _pooled(a, b, sizes=None):
    """A PooledMatches of the caller's own points: groups of `sizes` rows (default: one group)."""
    import multipoint_amd.utils as U
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate([a, b], 1), dtype=np.float32)).reshape(-1, 4).to(DEV)
    go = np.concatenate([[0], np.cumsum([len(a)] if sizes is None else sizes)]).astype(np.int32)
    return U.PooledMatches(pts, None, None, torch.from_numpy(go).to(DEV))


# ----------------------------------------------------------------------------------------------------------------------
# pooling
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P,K,groups', [(3, 300, None), (5, 257, [0, 0, 2, 2, 5]), (300, 7, 'runs'), (2, 1000, [0, 1])])
def test_pool_matches_against_numpy(P, K, groups):
    """pts / query_index / pair_offsets / group_offsets against the numpy restatement: ragged lists, unmatched rows, partner
    indices beyond the thermal list, more pairs than one scan step (300 > 256), list lengths off the 256-thread step, groups
    without a pair (ids 1, 3, 4 of the second case)."""
    import multipoint_amd.utils as U
    rng = np.random.default_rng(P * 1000 + K)
    sizes = rng.integers(0, K + 1, P)
    kp, cnt, midx, _ = C.planted_pairs(rng, P, K, *HW, 0.2, sizes=sizes)
    cnt[1::2] = np.maximum(cnt[1::2] - rng.integers(0, 3, P), 0)          # some partner indices now lie beyond the thermal list
    if groups == 'runs':
        groups = np.sort(rng.integers(0, 40, P))
    got = U.pool_matches(C.to_results(kp, cnt, midx, *HW, device=DEV), groups)
    pts, qidx, po, go = C.pool_host(kp, cnt, midx, groups)
    assert np.array_equal(got.pair_offsets.cpu().numpy(), po) and np.array_equal(got.group_offsets.cpu().numpy(), go)
    assert got.pts.shape == pts.shape and np.array_equal(got.pts.cpu().numpy(), pts)
    assert np.array_equal(got.query_index.cpu().numpy(), qidx)


# ----------------------------------------------------------------------------------------------------------------------
# pooled against per-pair: the parent's kernel is the yardstick
# ----------------------------------------------------------------------------------------------------------------------
EDGE_K, EDGE_T, EDGE_COUNTS = 3200, 257, (4, 5, 255, 256, 257, 3200)
# data seed of the K = EDGE_K case, picked on the CPU with the oracle alone as CASE_SEEDS was: the first seed from 0 at which
# every pair's usable matches are pooled_cases.well_posed for (thr 3, T = EDGE_T, seed 7, pair index).  Outliers are drawn at
# 30 % in every pair; well_posed asks for min(N, 8) inliers, so seeds 0 and 1, which leave the 5-match pair an outlier and a
# consensus set of 4, were passed over.  At seed 2 the winners have 4, 5, 176, 163, 187 and 2211 inliers.
EDGE_SEED = 2


def edge_pairs(seed=EDGE_SEED):
    """6 pairs at the per-pair limit K = 3200 whose numbers of usable matches are EDGE_COUNTS: the edges of the ordered
    compaction and of the 256-stride loops of the refit and the polish.  A pair has up to 300 keypoints more than usable matches,
    all matched at first; the surplus, chosen at random, is then unmatched, so the survivors are spread with holes over more
    than one step of 256 queries (but for the last pair, where every one of the 3200 queries survives)."""
    rng = np.random.default_rng(seed)
    sizes = [min(c + 300, EDGE_K) for c in EDGE_COUNTS]
    kp, cnt, midx, planted = C.planted_pairs(rng, len(sizes), EDGE_K, *HW, 0.3, sizes=sizes, matched_frac=1.1)
    for p, (n, c) in enumerate(zip(sizes, EDGE_COUNTS)):
        midx[p, rng.permutation(n)[:n - c]] = -1
    return kp, cnt, midx, planted


@pytest.mark.parametrize('K', [200, 1000, EDGE_K])
def test_pooled_equals_per_pair(K):
    """groups = arange(P): every group holds one pair, so sample4(seed, g, t, n) draws what the per-pair kernel draws.  n_inliers
    and the scattered mask must be equal, H within the device/oracle tolerance of the project, and the same for the polish.
    K = 200, 1000: 3 pairs of equal size, T = 512.  K = EDGE_K: the 6 pairs of edge_pairs, T = 257.
    Largest differences seen on an MI355X (printed below): 0 in all three cases, find and polish.  One kernel template
    (mp_homography.h) stands behind both routes, so H and the polished H must also be the same BYTES."""
    import multipoint_amd.utils as U
    thr = 3.0
    if K == EDGE_K:
        P, T = len(EDGE_COUNTS), EDGE_T
        kp, cnt, midx, _ = edge_pairs()
    else:
        P, T = 3, 512
        kp, cnt, midx, _ = C.planted_pairs(np.random.default_rng(K), P, K, *HW, 0.3)
    res = C.to_results(kp, cnt, midx, *HW, device=DEV)
    H1, m1, n1 = U.find_homography(res, thr, max_iters=T, seed=7)
    pooled = U.pool_matches(res, np.arange(P))
    H2, m2, n2 = U.find_homography_pooled(pooled, thr, max_iters=T, seed=7)
    qi, po = pooled.query_index.cpu().numpy(), pooled.pair_offsets.cpu().numpy()
    H1n, H2n = H1.cpu().numpy(), H2.cpu().numpy()
    print('find: max |H_pooled - H_pair| = %g' % np.abs(H1n - H2n).max())
    assert (n1.cpu().numpy() >= 4).all() and np.array_equal(n1.cpu().numpy(), n2.cpu().numpy())
    assert np.array_equal(C.scatter_mask(m2.cpu().numpy(), qi, po, P, K), m1.cpu().numpy())
    for p in range(P):
        assert np.abs(H1n[p] - H2n[p]).max() <= _tol(H1n[p])
    assert H1n.tobytes() == H2n.tobytes()
    R1, rm1, rn1, c1 = U.refine_homography(res, H1, thr)
    R2, rm2, rn2, c2 = U.refine_homography_pooled(pooled, H2, thr)
    R1n, R2n = R1.cpu().numpy(), R2.cpu().numpy()
    print('polish: max |H_pooled - H_pair| = %g, max |cost_pooled - cost_pair| = %g'
          % (np.abs(R1n - R2n).max(), np.abs(c1.cpu().numpy() - c2.cpu().numpy()).max()))
    assert np.array_equal(rn1.cpu().numpy(), rn2.cpu().numpy())
    assert np.array_equal(C.scatter_mask(rm2.cpu().numpy(), qi, po, P, K), rm1.cpu().numpy())
    for p in range(P):
        assert np.abs(R1n[p] - R2n[p]).max() <= _tol(R1n[p])
    assert R1n.tobytes() == R2n.tobytes()
    c1n, c2n = c1.cpu().numpy(), c2.cpu().numpy()
    assert (c2n[:, 1] <= c2n[:, 0]).all() and np.allclose(c1n, c2n, rtol=1e-9, atol=1e-9)


# ----------------------------------------------------------------------------------------------------------------------
# pooled against the oracle
# ----------------------------------------------------------------------------------------------------------------------
def _group_sizes():
    import multipoint_amd.utils as U
    c = U.pooled_chunk()[0]
    return [4, 5, 255, 256, 257, c - 1, c, c + 1, 3 * c + 7, 3201]


def _check_against_oracle(oracle, a, b, sizes, T, thr, seed):
    import multipoint_amd.utils as U
    Hm, mask, nin = U.find_homography_pooled(_pooled(a, b, sizes), thr, max_iters=T, seed=seed)
    Hm, mask, nin = Hm.cpu().numpy(), mask.cpu().numpy().astype(bool), nin.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(sizes)])
    worst = 0.0
    for g in range(len(sizes)):
        s, e = off[g], off[g + 1]
        Ho, mo = oracle.ransac_homography(a[s:e], b[s:e], thr, T, seed, g)
        if Ho is None:
            assert nin[g] == 0 and not mask[s:e].any() and (Hm[g] == 0).all()
            continue
        assert nin[g] == mo.sum() == mask[s:e].sum() and np.array_equal(mask[s:e], mo)
        worst = max(worst, np.abs(Hm[g] - Ho).max() / _tol(Ho))
        assert np.abs(Hm[g] - Ho).max() <= _tol(Ho)
    return worst


# data seeds of the (N index, T) cases, picked on the CPU with the oracle alone: the first offset from 0 at which the data is
# pooled_cases.well_posed (the winning consensus set has at least min(N, 8) members and a refit conditioned as
# pooled_cases.dlt_gap asks).  Offset 0 where a case is not listed; most listed ones have T = 1, where the only hypothesis drawn
# often holds an outlier and its few chance inliers do not determine a homography.
CASE_SEEDS = {(1, 1): 19, (1, 255): 7, (1, 256): 6, (1, 257): 5, (2, 1): 1, (3, 1): 1, (4, 1): 6, (5, 1): 7, (6, 1): 5, (7, 1): 1,
              (8, 1): 3, (9, 1): 3}


@pytest.mark.parametrize('T', [1, 255, 256, 257])
@pytest.mark.parametrize('n_index', range(10))
def test_pooled_matches_oracle(oracle, n_index, T):
    """Every group size at which the scoring kernel changes path (one thread step, one staged chunk, several chunks, the
    per-pair limit + 1) times every hypothesis count around one block of 256.  Integer coordinates: masks exactly equal, H
    within 1e-6 max(1, |H|)."""
    N = _group_sizes()[n_index]
    rng = np.random.default_rng(CASE_SEEDS.get((n_index, T), 0) + 1000 * n_index + T)
    a, b, _, _ = C.planted_points(rng, N, *HW, 0.3)
    worst = _check_against_oracle(oracle, a, b, [N], T, 3.0, 11)
    print('N = %d, T = %d: |H - H_oracle| / tolerance = %.3g' % (N, T, worst))


@pytest.mark.parametrize('T', [1, 257])
def test_pooled_three_groups_one_empty_one_too_small(oracle, T):
    """G = 3: a group of 3 points (fewer than sample4 can draw from: it must leave, not hang), an empty group, a group of 700."""
    rng = np.random.default_rng(33)                                        # (well_posed for both T, checked on the CPU)
    sizes = [3, 0, 700]
    a, b, _, _ = C.planted_points(rng, sum(sizes), *HW, 0.3)
    import multipoint_amd.utils as U
    Hm, mask, nin = U.find_homography_pooled(_pooled(a, b, sizes), 3.0, max_iters=T, seed=11)
    assert nin.tolist()[:2] == [0, 0] and (Hm[:2] == 0).all() and not mask[:3].any() and int(nin[2]) >= 4
    _check_against_oracle(oracle, a, b, sizes, T, 3.0, 11)
    R, rmask, rn, cost = U.refine_homography_pooled(_pooled(a, b, sizes), Hm, 3.0)
    assert rn.tolist()[:2] == [0, 0] and (R[:2] == 0).all() and not rmask[:3].any() and (cost[:2] == 0).all()
    # (the polish runs on the inliers of the estimate it is given, the REFITTED model: not the winning sample's consensus set)
    assert int(rn[2]) == int(rmask[3:].sum()) >= 4 and float(cost[2, 1]) <= float(cost[2, 0])


def test_pooled_large_group(oracle):
    """N = 200 003 (off every step of the kernels, 196 staged chunks over 64 splits), T = 512, 40 % outliers."""
    rng = np.random.default_rng(2)
    a, b, bad, hm = C.planted_points(rng, 200003, *HW, 0.4)
    worst = _check_against_oracle(oracle, a, b, [len(a)], 512, 3.0, 3)
    print('N = 200003: |H - H_oracle| / tolerance = %.3g' % worst)


def test_pooled_degenerate_inputs():
    """Collinear points: no 4-point sample is solvable, so no hypothesis votes -- zero matrix, no inliers, an untouched-zero
    mask, as test_find_homography_degenerate_inputs expects of the per-pair kernel."""
    import multipoint_amd.utils as U
    x = np.arange(10, dtype=np.float64)
    line = np.stack([x, np.zeros(10)], 1)
    Hm, mask, nin = U.find_homography_pooled(_pooled(line, line), 3.0, max_iters=256)
    assert nin.tolist() == [0] and not mask.any() and (Hm == 0).all()
    Hp, mp = U.find_homography_pooled_points(line, line, 3.0, max_iters=256, device=DEV)
    assert Hp is None and mp.shape == (10,) and not mp.any()
    Hp, mp = U.find_homography_pooled_points(line[:3], line[:3], device=DEV)
    assert Hp is None and mp.shape == (3,)
    R, rmask, rn, cost = U.refine_homography_pooled(_pooled(line, line), Hm, 3.0)
    assert rn.tolist() == [0] and not rmask.any() and (R == 0).all()


def test_c_abi_refusals():
    """MP_EINVAL with a message, before any launch: N >= 2^24, G out of range, max_iters out of range, a workspace that is too
    small, pts off its 16-byte alignment."""
    from multipoint_amd import _lib
    h = _lib.get_handle(torch.device(DEV))
    pts = torch.zeros((64, 4), dtype=torch.float32, device=DEV); go = torch.tensor([0, 16], dtype=torch.int32, device=DEV)
    Hm = torch.zeros(9, dtype=torch.float64, device=DEV); mask = torch.zeros(64, dtype=torch.uint8, device=DEV)
    nin = torch.zeros(1, dtype=torch.int32, device=DEV); ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)

    def find(p=pts, N=16, G=1, thr=3.0, T=256, wsb=ws.numel()):
        return h.lib.mp_find_homography_pooled(h.ptr, ctypes.c_void_p(p.data_ptr()), _lib.ptr(go), N, G, thr, T, 0, _lib.ptr(Hm),
                                               _lib.ptr(mask), _lib.ptr(nin), _lib.ptr(ws), wsb, _lib.stream_ptr(torch.device(DEV)))
    assert find() == 0
    for kw, word in ((dict(N=1 << 24), '2^24'), (dict(G=0), 'G'), (dict(G=65536), 'G'), (dict(T=0), 'max_iters'),
                     (dict(T=(1 << 20) + 1), 'max_iters'), (dict(thr=0.0), 'threshold'), (dict(wsb=512), 'workspace'),
                     (dict(p=pts.reshape(-1)[1:]), 'aligned')):
        assert find(**kw) == -1
        assert word in h.lib.mp_last_error(h.ptr).decode()
    n = ctypes.c_longlong()
    assert h.lib.mp_pooled_workspace_bytes(4, 1, 1 << 21, ctypes.byref(n)) == -1
    assert h.lib.mp_pooled_workspace_bytes(4, 2, 300, ctypes.byref(n)) == 0 and n.value >= 2 * 300 * 4 + 2 * 8


# ----------------------------------------------------------------------------------------------------------------------
# float32 sub-pixel points
# ----------------------------------------------------------------------------------------------------------------------
SUBPIXEL_SEED = 0


def test_pooled_points_subpixel(oracle):
    """find_homography_pooled_points on N = 5000 float32 sub-pixel correspondences.  With sub-pixel coordinates an error can
    sit on the threshold, where the device (fused multiply-adds) and the oracle (numpy) may round to different sides: the mask
    may differ only at correspondences whose error under the oracle's winning 4-point model lies within 1e-6 px of the
    threshold.  SUBPIXEL_SEED was picked on the CPU so that there is none (asserted first: at most 2)."""
    import multipoint_amd.utils as U
    rng = np.random.default_rng(SUBPIXEL_SEED)
    thr, T, seed = 3.0, 2000, 5
    a, b, bad, hm = C.planted_points(rng, 5000, *HW, 0.3, integer=False)
    a, b = a.astype(np.float32), b.astype(np.float32)
    Ho, mo = oracle.ransac_homography(a, b, thr, T, seed, 0)
    near = C.threshold_margin(C.winning_model(oracle, a, b, thr, T, seed, 0), a, b, thr) <= 1e-6
    assert Ho is not None and near.sum() <= 2
    Hm, mask = U.find_homography_pooled_points(a, b, thr, max_iters=T, seed=seed, device=DEV)
    assert Hm is not None and mask.shape == (5000,)
    diff = mask.astype(bool) != mo
    assert not (diff & ~near).any()
    print('sub-pixel: %d correspondences within 1e-6 px of the threshold, %d mask bytes differ, |H - H_oracle| / tolerance = %.3g'
          % (near.sum(), diff.sum(), np.abs(Hm - Ho).max() / _tol(Ho)))
    assert np.abs(Hm - Ho).max() <= _tol(Ho)
    assert C.corner_error(Hm, hm, *HW) < 0.5


# ----------------------------------------------------------------------------------------------------------------------
# pooling does what no single pair can
# ----------------------------------------------------------------------------------------------------------------------
SPARSE_SEED = 0


def sparse_pairs(seed=None):
    """40 pairs that share one homography, 3 matches each, a quarter of them outliers."""
    rng = np.random.default_rng(SPARSE_SEED if seed is None else seed)
    hm = C.random_homography(rng)
    kp, cnt, midx, planted = C.planted_pairs(rng, 40, 8, *HW, 0.25, sizes=[3] * 40, shared=hm, matched_frac=1.1)
    return kp, cnt, midx, planted, hm


def test_pooling_succeeds_where_every_pair_fails():
    """3 matches are fewer than a homography needs, so find_homography gives a zero matrix for every pair; the 120 pooled
    matches give the planted model (corners within 1 px) with every clean match an inlier.  SPARSE_SEED was checked on the CPU
    with the oracle."""
    import multipoint_amd.utils as U
    kp, cnt, midx, planted, hm = sparse_pairs()
    res = C.to_results(kp, cnt, midx, *HW, device=DEV)
    H1, m1, n1 = U.find_homography(res, 3.0)
    assert (H1 == 0).all() and not m1.any() and not n1.any()
    est = U.estimate_shared_homography(res, reproj_threshold=3.0)
    assert est.H.shape == (1, 3, 3) and est.pooled.pts.shape == (120, 4)
    assert C.corner_error(est.H[0].cpu().numpy(), hm, *HW) < 1.0
    bad = np.concatenate([planted[p][1] for p in range(40)])                # (every keypoint is matched: query order = list order)
    mask = est.mask.cpu().numpy().astype(bool)
    assert mask[~bad].all() and int(est.n_inliers[0]) == mask.sum()
    assert float(est.cost[0, 1]) <= float(est.cost[0, 0])


# ----------------------------------------------------------------------------------------------------------------------
# determinism and order
# ----------------------------------------------------------------------------------------------------------------------
def test_pooled_runs_are_bit_identical():
    import multipoint_amd.utils as U
    rng = np.random.default_rng(9)
    kp, cnt, midx, _ = C.planted_pairs(rng, 6, 900, *HW, 0.4)
    res = C.to_results(kp, cnt, midx, *HW, device=DEV)
    runs = [U.estimate_shared_homography(res, [0, 0, 0, 1, 1, 1], max_iters=700, seed=1) for _ in range(2)]
    for x, y in zip(runs[0][:4], runs[1][:4]):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert (runs[0].n_inliers.cpu().numpy() > 100).all()


def test_permuting_the_pairs_of_a_group_permutes_the_mask():
    """The samples are drawn by row index, so another order of the pairs draws other hypotheses and H need not be equal.  For
    the consensus set to be the same whatever is drawn, the clean matches here follow an integer translation EXACTLY (no noise,
    nothing to round): every all-clean sample gives that model to fp64 rounding, so its inliers are all clean matches plus the
    same few chance hits; with 30 % outliers 512 hypotheses hold an all-clean sample with probability 1 - 1e-60."""
    import multipoint_amd.utils as U
    rng = np.random.default_rng(4)
    P, K = 5, 120
    hm = np.array([[1.0, 0, 7], [0, 1, -4], [0, 0, 1]])
    kp, cnt, midx, planted = C.planted_pairs(rng, P, K, *HW, 0.0, sizes=rng.integers(60, K + 1, P), shared=hm)
    for p in range(P):                                                     # noise-free clean matches, far-away outliers
        n = cnt[2 * p]
        q = np.nonzero(midx[p, :n] >= 0)[0]
        kp[2 * p + 1, midx[p, q]] = kp[2 * p, q] + np.array([-4, 7])
        bad = q[rng.random(len(q)) < 0.3]
        kp[2 * p + 1, midx[p, bad]] += rng.integers(40, 200, (len(bad), 2)).astype(np.int32)
    order = rng.permutation(P)
    e1 = U.estimate_shared_homography(C.to_results(kp, cnt, midx, *HW, device=DEV), max_iters=512, polish=False)
    kp2 = kp.reshape(P, 2, K, 2)[order].reshape(2 * P, K, 2); cnt2 = cnt.reshape(P, 2)[order].reshape(-1)
    e2 = U.estimate_shared_homography(C.to_results(kp2, cnt2, midx[order], *HW, device=DEV), max_iters=512, polish=False)
    assert int(e1.n_inliers[0]) == int(e2.n_inliers[0]) >= 4
    m1 = C.scatter_mask(e1.mask.cpu().numpy(), e1.pooled.query_index.cpu().numpy(), e1.pooled.pair_offsets.cpu().numpy(), P, K)
    m2 = C.scatter_mask(e2.mask.cpu().numpy(), e2.pooled.query_index.cpu().numpy(), e2.pooled.pair_offsets.cpu().numpy(), P, K)
    assert np.array_equal(m2, m1[order])
    assert C.corner_error(e1.H[0].cpu().numpy(), hm, *HW) < 1e-6 and C.corner_error(e2.H[0].cpu().numpy(), hm, *HW) < 1e-6
