"""GPU (MI355X): the similarity and affine estimators (mp_find_transform*, mp_refine_transform*) on the three routes -- per-pair
integer lists, per-pair sub-pixel lists, pooled groups -- against the numpy restatement of tests/transform_restatement.py,
against each other, against planted models and against the homography entries they forward to."""
import ctypes

import numpy as np
import pytest
import torch

import pooled_cases as C
import transform_cases as T
import transform_restatement as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HW = T.HW
THR = 3.0


def _res(kp, cnt, midx, sub=None):
    from multipoint_amd.pipeline import PairResults
    P, K = midx.shape
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)                     # noqa: E731
    return PairResults(t(kp), None, t(cnt), None, t(midx), torch.zeros((P, K), device=DEV), None, *HW,
                       kp_sub=None if sub is None else t(np.asarray(sub, np.float32)))


def _points_res(a, b):
    """One pair that holds the correspondences a[i] -> b[i] (x, y): integer arrays as pixel lists, float arrays as sub-pixel ones."""
    a, b = np.asarray(a), np.asarray(b)
    n = len(a)
    kp = np.stack([a[:, ::-1], b[:, ::-1]]).astype(np.int32)
    sub = np.stack([a[:, ::-1], b[:, ::-1]]).astype(np.float32) if a.dtype.kind == 'f' or b.dtype.kind == 'f' else None
    return _res(kp, np.array([n, n], np.int32), np.arange(n, dtype=np.int32).reshape(1, n), sub)


def _pooled(a, b, sizes=None):
    import multipoint_amd.utils as U
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate([a, b], 1), dtype=np.float32)).reshape(-1, 4).to(DEV)
    go = np.concatenate([[0], np.cumsum([len(a)] if sizes is None else sizes)]).astype(np.int32)
    return U.PooledMatches(pts, None, None, torch.from_numpy(go).to(DEV))


def _np(*tensors):
    return [x.cpu().numpy() for x in tensors]


def _check_find(model, a, b, index, T_, seed, Hd, maskd, nd, what):
    """One pair / group of a device result against the restatement.  maskd: the device mask over the correspondences in list order.
    Returns |H - H_restated| / tolerance (0 without a model)."""
    Ho, mo, m6 = R.ransac_transform(a, b, model, THR, T_, seed, index, full=True)
    assert nd == maskd.sum(), what
    if Ho is None:
        assert nd == 0 and not maskd.any() and (Hd == 0).all(), what
        return 0.0
    near = T.near_threshold(m6, a, b, THR)
    diff = maskd.astype(bool) != mo
    assert not (diff & ~near).any(), what
    assert np.isfinite(Hd).all() and tuple(Hd[2]) == (0.0, 0.0, 1.0), what
    if model == 'similarity':
        assert Hd[0, 0] == Hd[1, 1] and Hd[0, 1] == -Hd[1, 0], what
    if diff.any():                                       # (another set, another refit: nothing more to compare)
        return 0.0
    assert np.abs(Hd - Ho).max() <= T.tol(Ho), what
    return np.abs(Hd - Ho).max() / T.tol(Ho)


def _check_refine(model, a, b, Hin, rounds, Hd, maskd, nd, costd, what):
    marked = []
    Ho, mo, no, co, _ = R.refine_transform(a, b, model, Hin, THR, rounds, marked=marked)
    assert nd == maskd.sum() and np.isfinite(Hd).all() and np.isfinite(costd).all() and costd[1] <= costd[0], what
    if any(T.near_threshold(m, a, b, THR).any() for m in marked):
        return
    assert np.array_equal(maskd.astype(bool), mo) and nd == no, what
    assert np.abs(Hd - Ho).max() <= T.tol(Ho), what
    assert np.allclose(costd, co, rtol=1e-9, atol=1e-9), what


# ----------------------------------------------------------------------------------------------------------------------
# per-pair route against the restatement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sweep():
    """The sweep's pairs per (model, outlier share), built once and left unchanged."""
    out = {}
    for mi, model in enumerate(T.MODELS):
        for oi, outliers in enumerate(T.SWEEP_OUTLIERS):
            kp, cnt, midx, _ = T.sweep_pairs(model, outliers, seed=100 * mi + oi)
            out[model, outliers] = (kp, cnt, midx, T.pair_lists(kp, cnt, midx))
    return out


@pytest.mark.parametrize('outliers', T.SWEEP_OUTLIERS)
@pytest.mark.parametrize('T_', T.SWEEP_T)
@pytest.mark.parametrize('model', T.MODELS)
def test_find_and_refine_match_the_restatement(sweep, model, T_, outliers):
    """Seven pairs at K = 3200 (the LDS limit) with S - 1, S, S + 1, 255, 256, 257 and 3200 usable matches, hypothesis counts
    around one block of 256: H within 1e-6 max(1, |H|), the mask equal except within 1e-6 px of the threshold under the
    winning sample's model, n_inliers the mask's sum; then ten rounds of refinement from the device's estimate."""
    import multipoint_amd.utils as U
    kp, cnt, midx, lists = sweep[model, outliers]
    res = _res(kp, cnt, midx)
    seed = 7
    H, mask, nin = _np(*U.find_transform(res, model, THR, max_iters=T_, seed=seed))
    Hr, rmask, rn, cost = _np(*U.refine_transform(res, H, model, THR, rounds=10))
    counts = T.sweep_counts(model)
    worst = 0.0
    for p, (a, b, q) in enumerate(lists):
        what = '%s T %d outliers %g pair %d (%d matches)' % (model, T_, outliers, p, counts[p])
        assert len(a) == counts[p]
        other = np.ones(mask.shape[1], bool); other[q] = False
        assert not mask[p, other].any() and not rmask[p, other].any(), what
        worst = max(worst, _check_find(model, a, b, p, T_, seed, H[p], mask[p, q], nin[p], what))
        if counts[p] < T.SAMPLE[model] + 1:
            assert nin[p] == 0, what
        _check_refine(model, a, b, H[p], 10, Hr[p], rmask[p, q], rn[p], cost[p], what)
    print('%s T %d outliers %g: inliers %s, refined %s, worst |H - H_restated| / tolerance %.3g'
          % (model, T_, outliers, nin.tolist(), rn.tolist(), worst))
    if T_ >= 255 and outliers <= 0.5:
        assert (nin[3:] >= 100).all()                                 # (every pair with 255 matches or more has a model)


# ----------------------------------------------------------------------------------------------------------------------
# pooled route
# ----------------------------------------------------------------------------------------------------------------------
def _pooled_sizes():
    import multipoint_amd.utils as U
    c, s = U.pooled_chunk()
    return [c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1, s * c - 1, s * c, s * c + 1]


@pytest.mark.parametrize('n_index', range(9))
@pytest.mark.parametrize('model', T.MODELS)
def test_pooled_matches_the_restatement(model, n_index):
    """One group of a size around the staged chunk, two chunks (where a second split starts) and the most splits of a launch
    (beyond it a workgroup walks more than one chunk); T = 257: the second hypothesis block has one live thread."""
    import multipoint_amd.utils as U
    N = _pooled_sizes()[n_index]
    rng = np.random.default_rng(1000 * n_index + len(model))
    a, b, _, _ = C.planted_points(rng, N, *HW, 0.5, hm=T.random_model(rng, model))
    pooled = _pooled(a, b)
    H, mask, nin = _np(*U.find_transform_pooled(pooled, model, THR, max_iters=257, seed=11))
    worst = _check_find(model, a, b, 0, 257, 11, H[0], mask, nin[0], '%s N %d' % (model, N))
    Hr, rmask, rn, cost = _np(*U.refine_transform_pooled(pooled, H, model, THR, rounds=10))
    _check_refine(model, a, b, H[0], 10, Hr[0], rmask, rn[0], cost[0], '%s N %d refine' % (model, N))
    print('%s N %d: %d inliers, refined %d, |H - H_restated| / tolerance %.3g' % (model, N, nin[0], rn[0], worst))
    assert nin[0] > 0.4 * N


@pytest.mark.parametrize('T_', [1, 257])
@pytest.mark.parametrize('model', T.MODELS)
def test_pooled_three_groups_one_empty_one_below_the_minimum(model, T_):
    import multipoint_amd.utils as U
    S = T.SAMPLE[model]
    sizes = [S - 1, 0, 700]
    rng = np.random.default_rng(33)
    a, b, _, _ = C.planted_points(rng, sum(sizes), *HW, 0.3, hm=T.random_model(rng, model))
    pooled = _pooled(a, b, sizes)
    H, mask, nin = _np(*U.find_transform_pooled(pooled, model, THR, max_iters=T_, seed=11))
    assert nin[:2].tolist() == [0, 0] and (H[:2] == 0).all() and not mask[:S - 1].any()
    _check_find(model, a[S - 1:], b[S - 1:], 2, T_, 11, H[2], mask[S - 1:], nin[2], '%s T %d' % (model, T_))
    if T_ == 257:
        assert nin[2] > 400
    Hr, rmask, rn, cost = _np(*U.refine_transform_pooled(pooled, H, model, THR))
    assert rn[:2].tolist() == [0, 0] and (Hr[:2] == 0).all() and not rmask[:S - 1].any() and (cost[:2] == 0).all()
    _check_refine(model, a[S - 1:], b[S - 1:], H[2], 10, Hr[2], rmask[S - 1:], rn[2], cost[2], '%s T %d refine' % (model, T_))


@pytest.mark.parametrize('model', T.MODELS)
def test_pooled_with_one_group_per_pair_equals_per_pair(sweep, model):
    """groups = arange(P): the sampling draws what the per-pair kernel draws, the refit and the refinement are one kernel
    template on two point views."""
    import multipoint_amd.utils as U
    kp, cnt, midx, _ = sweep[model, 0.5]
    P, K = midx.shape
    res = _res(kp, cnt, midx)
    H1, m1, n1 = _np(*U.find_transform(res, model, THR, max_iters=257, seed=7))
    pooled = U.pool_matches(res, np.arange(P))
    H2, m2, n2 = _np(*U.find_transform_pooled(pooled, model, THR, max_iters=257, seed=7))
    qi, po = _np(pooled.query_index, pooled.pair_offsets)
    assert np.array_equal(n1, n2) and (n1[3:] >= 100).all() and not n1[:2].any()
    assert np.array_equal(C.scatter_mask(m2, qi, po, P, K), m1)
    for p in range(P):
        assert np.abs(H1[p] - H2[p]).max() <= T.tol(H1[p])
    R1, rm1, rn1, c1 = _np(*U.refine_transform(res, H1, model, THR))
    R2, rm2, rn2, c2 = _np(*U.refine_transform_pooled(pooled, H1, model, THR))
    print('%s: max |H_pooled - H_pair| find %g, refine %g' % (model, np.abs(H1 - H2).max(), np.abs(R1 - R2).max()))
    assert np.array_equal(rn1, rn2) and np.array_equal(C.scatter_mask(rm2, qi, po, P, K), rm1)
    for p in range(P):
        assert np.abs(R1[p] - R2[p]).max() <= T.tol(R1[p])
    assert np.allclose(c1, c2, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize('model', T.MODELS)
def test_permuting_the_pairs_of_a_group_permutes_the_mask(model):
    """As test_gpu_pooled_homography's: the clean matches follow an integer translation exactly (a similarity and an affine
    transform), the outliers lie far away, so every all-clean sample has the same consensus set whatever rows it is drawn from."""
    import multipoint_amd.utils as U
    rng = np.random.default_rng(4)
    P, K = 5, 120
    hm = np.array([[1.0, 0, 7], [0, 1, -4], [0, 0, 1]])
    kp, cnt, midx, _ = C.planted_pairs(rng, P, K, *HW, 0.0, sizes=rng.integers(60, K + 1, P), shared=hm)
    for p in range(P):
        n = cnt[2 * p]
        q = np.nonzero(midx[p, :n] >= 0)[0]
        kp[2 * p + 1, midx[p, q]] = kp[2 * p, q] + np.array([-4, 7])
        bad = q[rng.random(len(q)) < 0.3]
        kp[2 * p + 1, midx[p, bad]] += rng.integers(40, 200, (len(bad), 2)).astype(np.int32)
    order = rng.permutation(P)
    e1 = U.estimate_shared_transform(_res(kp, cnt, midx), model=model, max_iters=512, polish=False)
    kp2 = kp.reshape(P, 2, K, 2)[order].reshape(2 * P, K, 2); cnt2 = cnt.reshape(P, 2)[order].reshape(-1)
    e2 = U.estimate_shared_transform(_res(kp2, cnt2, midx[order]), model=model, max_iters=512, polish=False)
    assert int(e1.n_inliers[0]) == int(e2.n_inliers[0]) >= 4 and e1.cost is None
    m1 = C.scatter_mask(*_np(e1.mask, e1.pooled.query_index, e1.pooled.pair_offsets), P, K)
    m2 = C.scatter_mask(*_np(e2.mask, e2.pooled.query_index, e2.pooled.pair_offsets), P, K)
    assert np.array_equal(m2, m1[order])
    assert C.corner_error(e1.H[0].cpu().numpy(), hm, *HW) < 1e-6 and C.corner_error(e2.H[0].cpu().numpy(), hm, *HW) < 1e-6


# ----------------------------------------------------------------------------------------------------------------------
# degenerate input
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', T.MODELS)
def test_degenerate_inputs_give_zeros_and_no_nan(model):
    import multipoint_amd.utils as U
    n = 12
    x = np.arange(n, dtype=np.int64)
    cases = {'coincident': (np.full((n, 2), 5), np.stack([x, 2 * x], 1))}
    if model == 'affine':
        cases['collinear'] = (np.stack([x, 3 * x], 1), np.stack([x, 3 * x], 1))
    for name, (a, b) in cases.items():
        for pts in ((a, b), (a.astype(np.float32), b.astype(np.float32))):                # integer and float route
            res = _points_res(*pts)
            H, mask, nin = _np(*U.find_transform(res, model, THR, max_iters=256))
            assert not H.any() and not mask.any() and not nin.any(), name
            Hr, rmask, rn, cost = _np(*U.refine_transform(res, H, model, THR))
            assert not Hr.any() and not rmask.any() and not rn.any() and not cost.any(), name
            Hp, mp = U.find_transform_points(*pts, model, THR, max_iters=256, device=DEV)
            assert Hp is None and mp.shape == (n,) and not mp.any(), name
        pooled = _pooled(a, b)
        H, mask, nin = _np(*U.find_transform_pooled(pooled, model, THR, max_iters=256))
        assert not H.any() and not mask.any() and not nin.any(), name
        # a refinement handed a model of such data cannot refit it: the model stays, nothing is NaN
        Hr, rmask, rn, cost = _np(*U.refine_transform_pooled(_pooled(a, a), np.eye(3)[None], model, THR))
        assert np.array_equal(Hr[0], np.eye(3)) and rmask.all() and rn[0] == n and not cost.any(), name
    # every match unusable: no partner, or a partner index beyond the thermal list
    kp, cnt, midx, _ = C.planted_pairs(np.random.default_rng(0), 2, 50, *HW, 0.2)
    midx[0] = -1
    midx[1, :] = 49; cnt[3] = 40
    res = _res(kp, cnt, midx)
    H, mask, nin = _np(*U.find_transform(res, model, THR, max_iters=64))
    assert not H.any() and not mask.any() and not nin.any()
    Hr, rmask, rn, cost = _np(*U.refine_transform(res, np.eye(3)[None].repeat(2, 0), model, THR))
    assert not Hr.any() and not rmask.any() and not rn.any() and not cost.any()
    est = U.estimate_shared_transform(res, model=model, max_iters=64)
    assert est.pooled.pts.shape[0] == 0 and not est.H.cpu().numpy().any() and not est.n_inliers.cpu().numpy().any()


# ----------------------------------------------------------------------------------------------------------------------
# float against integer route
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', T.MODELS)
def test_whole_number_float_lists_give_the_integer_bits(sweep, model):
    import multipoint_amd.utils as U
    kp, cnt, midx, _ = sweep[model, 0.5]
    ri, rf = _res(kp, cnt, midx), _res(kp, cnt, midx, sub=kp.astype(np.float32))
    fi, ff = U.find_transform(ri, model, THR, max_iters=300, seed=3), U.find_transform(rf, model, THR, max_iters=300, seed=3)
    for x, y in zip(fi, ff):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert int(fi[2][-1]) > 1000
    for x, y in zip(U.refine_transform(ri, fi[0], model, THR), U.refine_transform(rf, ff[0], model, THR)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


@pytest.mark.parametrize('model', T.MODELS)
def test_fractional_points_recover_the_model_closer_than_rounded_ones(model):
    import multipoint_amd.utils as U
    rng = np.random.default_rng(8)
    hm = T.random_model(rng, model)
    a, b, _, _ = C.planted_points(rng, 400, *HW, 0.3, hm=hm, noise=0.0, integer=False)
    a, b = a.astype(np.float32), b.astype(np.float32)
    Hf, mf = U.find_transform_points(a, b, model, THR, max_iters=512, seed=1, device=DEV)
    Hi, mi = U.find_transform_points(np.rint(a).astype(np.int64), np.rint(b).astype(np.int64), model, THR, max_iters=512, seed=1,
                                     device=DEV)
    ef, ei = C.corner_error(Hf, hm, *HW), C.corner_error(Hi, hm, *HW)
    print('%s: corner error %.3g px from fractional points, %.3g px from rounded ones' % (model, ef, ei))
    assert mf.sum() >= 250 and mi.sum() >= 250
    assert ef < 1e-3 and ef < 0.1 * ei


# ----------------------------------------------------------------------------------------------------------------------
# refinement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', T.MODELS)
def test_refinement_properties(model):
    import multipoint_amd.utils as U
    rng = np.random.default_rng(2)
    # clean data, a start 2 px off at every corner: back to the planted model
    a, b = T.exact_points(rng, 600, model)
    start = T.EXACT_MODELS[model].copy(); start[0, 2] += 2.0
    for res in (_points_res(a.astype(np.int64), b.astype(np.float32)), None):
        if res is None:
            refine = lambda H, rounds: _np(*U.refine_transform_pooled(_pooled(a, b), H, model, THR, rounds))      # noqa: E731
        else:
            refine = lambda H, rounds, res=res: _np(*U.refine_transform(res, H, model, THR, rounds))            # noqa: E731
        H0, m0, n0, c0 = refine(start[None], 0)
        assert np.array_equal(H0[0], start) and m0.all() and n0[0] == 600 and c0[0, 0] == c0[0, 1] == pytest.approx(2400.0)
        H1, m1, n1, c1 = refine(start[None], 10)
        err = C.corner_error(H1[0], T.EXACT_MODELS[model], *HW)
        print('%s: from 2 px to %.3g px, cost %.6g -> %.3g' % (model, err, c1[0, 0], c1[0, 1]))
        assert err < 1e-6 and n1[0] == 600 and c1[0, 1] <= c1[0, 0] and c1[0, 0] == pytest.approx(2400.0)
        H2, m2, n2, c2 = refine(H1, 1)                                 # a fixed point: one more round changes nothing
        assert H2.tobytes() == H1.tobytes() and np.array_equal(m2, m1) and n2[0] == n1[0] and c2[0, 0] == c2[0, 1]
    # noisy data with outliers, several pairs: the cost never rises, rounds = 0 returns the input with its own mask, the result
    # of enough rounds is a fixed point
    kp, cnt, midx, _ = C.planted_pairs(rng, 4, 500, *HW, 0.5, shared=T.random_model(rng, model))
    res = _res(kp, cnt, midx)
    H, mask, nin = U.find_transform(res, model, THR, max_iters=300, seed=2)
    H0, m0, n0, c0 = _np(*U.refine_transform(res, H, model, THR, rounds=0))
    assert H0.tobytes() == H.cpu().numpy().tobytes() and (c0[:, 0] == c0[:, 1]).all() and (n0 == m0.sum(1)).all()
    lists = T.pair_lists(kp, cnt, midx)
    for p, (pa, pb, q) in enumerate(lists):                           # its own mask: the matches within THR of the input
        m6 = H0[p].reshape(9)[:6]
        want = R.error2(m6, *map(R._f32, (pa, pb))) <= THR * THR
        near = T.near_threshold(m6, pa, pb, THR)
        assert not ((m0[p, q].astype(bool) != want) & ~near).any()
    # from a start 2.5 / 1.5 px off, where about half of the inliers are beyond the threshold: the set grows over the rounds
    # (on the CPU: two refits, back to the consensus set of the estimate; no error within 2e-4 px of the threshold)
    start = H0.copy(); start[:, 0, 2] += 2.5; start[:, 1, 2] -= 1.5
    Hs, ms, ns, cs = _np(*U.refine_transform(res, start, model, THR, rounds=0))
    H1, m1, n1, c1 = _np(*U.refine_transform(res, start, model, THR, rounds=50))
    print('%s: inliers of the start %s, after the rounds %s, of the estimate %s' % (model, ns.tolist(), n1.tolist(), nin.tolist()))
    assert (c1[:, 1] <= c1[:, 0]).all() and (n1 == m1.sum(1)).all() and (n1 > ns).all() and (ns >= 10).all()
    for p, (pa, pb, q) in enumerate(lists):
        _check_refine(model, pa, pb, start[p], 50, H1[p], m1[p, q], n1[p], c1[p], '%s pair %d' % (model, p))
    H2, m2, n2, c2 = _np(*U.refine_transform(res, H1, model, THR, rounds=1))
    assert H2.tobytes() == H1.tobytes() and np.array_equal(m2, m1) and np.array_equal(n2, n1) and (c2[:, 0] == c2[:, 1]).all()


# ----------------------------------------------------------------------------------------------------------------------
# forwarding, determinism
# ----------------------------------------------------------------------------------------------------------------------
def test_model_homography_is_the_existing_entries_bit_for_bit():
    import multipoint_amd.utils as U
    kp, cnt, midx, _ = C.planted_pairs(np.random.default_rng(5), 3, 700, *HW, 0.3)
    sub = kp.astype(np.float32) + np.random.default_rng(6).uniform(-0.4, 0.4, kp.shape).astype(np.float32)

    def same(xs, ys):
        assert len(xs) == len(ys)
        for x, y in zip(xs, ys):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    for res in (_res(kp, cnt, midx), _res(kp, cnt, midx, sub=sub)):
        want = U.find_homography(res, THR, max_iters=400, seed=9)
        same(U.find_transform(res, 'homography', THR, max_iters=400, seed=9), want)
        assert (want[2] >= 100).all()
        same(U.refine_transform(res, want[0], 'homography', THR, rounds=7), U.refine_homography(res, want[0], THR, iters=7))
        same(U.refine_alignment(res, THR, rounds=0, model='homography')[1:], U.refine_alignment(res, THR, rounds=0)[1:])
    pooled = U.pool_matches(_res(kp, cnt, midx), [0, 0, 1])
    want = U.find_homography_pooled(pooled, THR, max_iters=400, seed=9)
    same(U.find_transform_pooled(pooled, 'homography', THR, max_iters=400, seed=9), want)
    same(U.refine_transform_pooled(pooled, want[0], 'homography', THR, rounds=7), U.refine_homography_pooled(pooled, want[0], THR, iters=7))
    e1, e2 = U.estimate_shared_transform(_res(kp, cnt, midx), [0, 0, 1], 'homography', seed=2), U.estimate_shared_homography(
        _res(kp, cnt, midx), [0, 0, 1], seed=2)
    same(e1[:4], e2[:4])


@pytest.mark.parametrize('model', T.MODELS)
def test_runs_are_bit_identical(model):
    import multipoint_amd.utils as U
    kp, cnt, midx, _ = C.planted_pairs(np.random.default_rng(9), 6, 900, *HW, 0.5, shared=T.random_model(np.random.default_rng(1), model))
    sub = kp.astype(np.float32) + np.random.default_rng(6).uniform(-0.4, 0.4, kp.shape).astype(np.float32)

    def run():
        out = []
        for res in (_res(kp, cnt, midx), _res(kp, cnt, midx, sub=sub)):                   # the integer and the float entries
            f = U.find_transform(res, model, THR, max_iters=700, seed=1)
            out += list(f) + list(U.refine_transform(res, f[0], model, THR))
        e = U.estimate_shared_transform(_res(kp, cnt, midx), [0, 0, 0, 1, 1, 1], model, max_iters=700, seed=1)   # the pooled ones
        f = U.find_transform_pooled(e.pooled, model, THR, max_iters=700, seed=1)
        return out + list(e[:4]) + list(f)
    r1, r2 = run(), run()
    for x, y in zip(r1, r2):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    assert (r1[2].cpu().numpy() > 100).all() and (r1[-1].cpu().numpy() > 300).all()


# ----------------------------------------------------------------------------------------------------------------------
# what the models are for
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', sorted(T.FEW_SEEDS))
def test_few_inliers_similarity_recovers_the_transform(seed):
    """The seeds of tests/test_transform_host.py (6-8 correct matches of 40, where the restated 4-point homography is more than 3 px
    off or finds nothing): the kernels' similarity is within 1 px of the planted transform at the four corners."""
    import multipoint_amd.utils as U
    a, b, good, hm = T.few_inlier_points(seed)
    H, mask = U.find_transform_points(a, b, 'similarity', T.FEW_THR, max_iters=T.FEW_T, seed=T.FEW_RANSAC_SEED, device=DEV)
    assert H is not None
    err = C.corner_error(H, hm, *T.FEW_HW)
    print('seed %d: %d of %d planted inliers found, corner error %.3f px' % (seed, mask[good].sum(), good.sum(), err))
    assert err < 1.0
    Ho, mo = R.ransac_transform(a, b, 'similarity', T.FEW_THR, T.FEW_T, T.FEW_RANSAC_SEED, 0)
    assert np.array_equal(mask.astype(bool), mo) and np.abs(H - Ho).max() <= T.tol(Ho)
    angle, scale, dx, dy = U.decompose_similarity(H)
    want = U.decompose_similarity(hm)
    assert abs(angle - want[0]) < 0.02 and abs(scale - want[1]) < 0.02


def test_refine_alignment_with_a_similarity():
    """utils.refine_alignment(model='similarity') on a planted pair of tests/guided_restatement.py (160 x 130 keypoints, half of the
    smaller list true partners, half of those shadowed by a closer distractor that the mutual matcher prefers): the guided
    re-matching under the first similarity wins partners back, so the end has no fewer inliers than find_transform alone, and
    is the composition of its steps."""
    import guided_restatement as G
    import multipoint_amd.utils as U
    from multipoint_amd.pipeline import PairResults
    D = 64
    pr = G.make_pair(D, 0)
    K = G.K
    desc = np.zeros((2, K, D), np.float32); kp = np.zeros((2, K, 2), np.int32)
    n, m = len(pr['A']), len(pr['B'])
    desc[0, :n] = pr['A']; desc[1, :m] = pr['B']; kp[0, :n] = pr['kpA']; kp[1, :m] = pr['kpB']
    desc, kp = torch.from_numpy(desc).to(DEV), torch.from_numpy(kp).to(DEV)
    cnt = torch.tensor([n, m], dtype=torch.int32, device=DEV)
    mi, md, mc = U.match_pairs(desc, cnt, desc[1:], cnt[1:], pair_stride=2 * K * D, count_stride=2)
    res = PairResults(kp, None, cnt, desc, mi, md, mc, *G.FRAME)
    H0, m0, n0 = U.find_transform(res, 'similarity', THR)
    res2, H, mask, nin = U.refine_alignment(res, THR, model='similarity')
    print('similarity: %d inliers of %d matches -> %d inliers of %d matches' % (int(n0[0]), int(mc[0]), int(nin[0]), int(res2.match_count[0])))
    assert int(n0[0]) >= 10 and int(nin[0]) >= int(n0[0]) and res2.match_mode == 'guided'      # (on the CPU: 33 of 76 -> 68 of 73)
    Hn = H[0].cpu().numpy()
    assert Hn[0, 0] == Hn[1, 1] and Hn[0, 1] == -Hn[1, 0] and tuple(Hn[2]) == (0.0, 0.0, 1.0)
    print('corner distance to the planted homography (perspective terms of 1e-4, which no similarity has): %.2f px'
          % C.corner_error(Hn, pr['H'], *G.FRAME))
    # by hand
    gi, gd, gc = U.guided_pairs(desc, cnt, desc[1:], cnt[1:], kp, kp[1:], H0, 2 * THR, -1.0, pair_stride=2 * K * D, count_stride=2)
    hand = PairResults(kp, None, cnt, desc, gi, gd, gc, *G.FRAME, 'guided')
    H1, _, _ = U.find_transform(hand, 'similarity', THR)
    H2, mask2, nin2, _ = U.refine_transform(hand, H1, 'similarity', THR)
    assert torch.equal(res2.match_idx, gi) and torch.equal(H, H2) and torch.equal(mask, mask2) and torch.equal(nin, nin2)


# ----------------------------------------------------------------------------------------------------------------------
# C ABI
# ----------------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals():
    """MP_EINVAL with a message, before any launch."""
    from multipoint_amd import _lib
    dev = torch.device(DEV)
    h = _lib.get_handle(dev)
    P, K = 2, 64
    kp = torch.zeros((2 * P, K, 2), dtype=torch.int32, device=DEV); kpf = kp.float()
    cnt = torch.zeros(2 * P, dtype=torch.int32, device=DEV); midx = torch.full((P, K), -1, dtype=torch.int32, device=DEV)
    Hm = torch.zeros((P, 9), dtype=torch.float64, device=DEV); mask = torch.zeros((P, K), dtype=torch.uint8, device=DEV)
    nin = torch.zeros(P, dtype=torch.int32, device=DEV); cost = torch.zeros((P, 2), dtype=torch.float64, device=DEV)
    st = _lib.stream_ptr(dev)

    def margs(entry, model):                               # (the *_homography* entries take no model)
        return () if 'homography' in entry else (model,)

    def find(entry='mp_find_transform', k=kp, P=P, K=K, model=1, thr=3.0, T_=256, H=Hm):
        return getattr(h.lib, entry)(h.ptr, _lib.ptr(k), _lib.ptr(cnt), _lib.ptr(midx), P, K, *margs(entry, model), thr, T_, 0,
                                     _lib.ptr(H), _lib.ptr(mask), _lib.ptr(nin), st)

    def refine(entry='mp_refine_transform', k=kp, P=P, K=K, model=2, thr=3.0, rounds=3, H=Hm):
        return getattr(h.lib, entry)(h.ptr, _lib.ptr(k), _lib.ptr(cnt), _lib.ptr(midx), P, K, *margs(entry, model), thr, rounds,
                                     _lib.ptr(H), _lib.ptr(mask), _lib.ptr(nin), _lib.ptr(cost), st)
    bad = ((dict(model=3), 'model'), (dict(model=-1), 'model'), (dict(thr=0.0), 'threshold'), (dict(K=0), 'K'), (dict(K=3201), 'K'),
           (dict(P=0), 'P'), (dict(H=None), 'NULL'))
    for entry, k in (('mp_find_transform', kp), ('mp_find_transform_f', kpf)):
        assert find(entry, k) == 0 and find(entry, k, model=0) == 0 and find(entry, k, model=2) == 0
        for kw, word in bad + ((dict(T_=0), 'max_iters'), (dict(T_=(1 << 20) + 1), 'max_iters')):
            assert find(entry, k, **kw) == -1, kw
            msg = h.lib.mp_last_error(h.ptr).decode()
            assert word in msg and entry in msg, (kw, msg)
    for entry, k in (('mp_refine_transform', kp), ('mp_refine_transform_f', kpf)):
        assert refine(entry, k) == 0 and refine(entry, k, model=0) == 0 and refine(entry, k, model=1) == 0
        for kw, word in bad + ((dict(rounds=-1), 'rounds'), (dict(rounds=1001), 'rounds')):
            assert refine(entry, k, **kw) == -1, kw
            msg = h.lib.mp_last_error(h.ptr).decode()
            assert word in msg and entry in msg, (kw, msg)
    # the *_homography* entries are the same bodies at MP_MODEL_HOMOGRAPHY: the same tables without the model rows
    for entry, k in (('mp_find_homography', kp), ('mp_find_homography_f', kpf)):
        assert find(entry, k) == 0
        for kw, word in bad[2:] + ((dict(T_=0), 'max_iters'), (dict(T_=(1 << 20) + 1), 'max_iters')):
            assert find(entry, k, **kw) == -1, kw
            msg = h.lib.mp_last_error(h.ptr).decode()
            assert word in msg and entry in msg, (kw, msg)
    for entry, k in (('mp_refine_homography', kp), ('mp_refine_homography_f', kpf)):
        assert refine(entry, k) == 0
        for kw, word in bad[2:] + ((dict(rounds=-1), 'iters'), (dict(rounds=1001), 'iters')):
            assert refine(entry, k, **kw) == -1, kw
            msg = h.lib.mp_last_error(h.ptr).decode()
            assert word in msg and entry in msg, (kw, msg)
    # pooled
    pts = torch.zeros((64, 4), dtype=torch.float32, device=DEV); go = torch.tensor([0, 16], dtype=torch.int32, device=DEV)
    H1 = torch.zeros(9, dtype=torch.float64, device=DEV); pmask = torch.zeros(64, dtype=torch.uint8, device=DEV)
    n1 = torch.zeros(1, dtype=torch.int32, device=DEV); ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)

    def pfind(p=pts, N=16, G=1, model=1, thr=3.0, T_=256, wsb=ws.numel(), entry='mp_find_transform_pooled'):
        return getattr(h.lib, entry)(h.ptr, ctypes.c_void_p(p.data_ptr()), _lib.ptr(go), N, G, *margs(entry, model), thr, T_, 0,
                                     _lib.ptr(H1), _lib.ptr(pmask), _lib.ptr(n1), _lib.ptr(ws), wsb, st)

    def prefine(p=pts, N=16, G=1, model=2, thr=3.0, rounds=3, entry='mp_refine_transform_pooled'):
        return getattr(h.lib, entry)(h.ptr, ctypes.c_void_p(p.data_ptr()), _lib.ptr(go), N, G, *margs(entry, model), thr, rounds,
                                     _lib.ptr(H1), _lib.ptr(pmask), _lib.ptr(n1), None, st)
    assert pfind() == 0 and pfind(model=0) == 0 and pfind(model=2) == 0 and prefine() == 0 and prefine(model=0) == 0
    pbad = ((dict(model=7), 'model'), (dict(N=1 << 24), '2^24'), (dict(G=0), 'G'), (dict(G=65536), 'G'), (dict(thr=-1.0), 'threshold'),
            (dict(p=pts.reshape(-1)[1:]), 'aligned'))
    for kw, word in pbad + ((dict(T_=0), 'max_iters'), (dict(T_=(1 << 20) + 1), 'max_iters'), (dict(wsb=512), 'workspace')):
        assert pfind(**kw) == -1, kw
        assert word in h.lib.mp_last_error(h.ptr).decode(), kw
    for kw, word in pbad + ((dict(rounds=-1), 'rounds'), (dict(rounds=1001), 'rounds')):
        assert prefine(**kw) == -1, kw
        assert word in h.lib.mp_last_error(h.ptr).decode(), kw
    entry = 'mp_find_homography_pooled'
    assert pfind(entry=entry) == 0
    for kw, word in pbad[1:] + ((dict(T_=0), 'max_iters'), (dict(T_=(1 << 20) + 1), 'max_iters'), (dict(wsb=512), 'workspace')):
        assert pfind(entry=entry, **kw) == -1, kw
        msg = h.lib.mp_last_error(h.ptr).decode()
        assert word in msg and entry in msg, (kw, msg)
    entry = 'mp_refine_homography_pooled'
    assert prefine(entry=entry) == 0
    for kw, word in pbad[1:] + ((dict(rounds=-1), 'iters'), (dict(rounds=1001), 'iters')):
        assert prefine(entry=entry, **kw) == -1, kw
        msg = h.lib.mp_last_error(h.ptr).decode()
        assert word in msg and entry in msg, (kw, msg)
    torch.cuda.synchronize()
