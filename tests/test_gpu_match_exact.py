"""GPU (MI355X): the matchers (mp_match.h, match_mfma.hip, match_guided.hip, match_extra.hip) and the descriptor sampler
(sample_desc.hip) on exact-arithmetic inputs, compared BIT FOR BIT with integer truths (tests/exact_match_restatement.py; the
premise is checked on the CPU by tests/test_match_exact_host.py).

The rows have entries in {0, +-2^-k} and norm exactly 1, so every dot product is exact in fp32 whatever the order of the sums,
and most queries have tied nearest neighbours, in different half-waves, tiles and column shares.  Nothing is ambiguous: every
index, count and distance bit pattern is determined, every comparison is np.array_equal on int32 views, there is no tolerance
and no excluded query.  What that pins down: the lowest index wins every tie (across half-waves, tiles, column shares, merge2
and merge_shares), the `u < ub` / `u < ub2` pre-filters drop nothing, `d < threshold` is strict, the gate is `<= r^2`, a gated
row without a candidate yields no match, the clip gives exactly 0 and 2, and the scalar knn2 route and the MFMA route return
the same bits.  The one tolerance of the file is the sampler's at odd coordinates (real bilinear weights): DESC_ABS = 2^-23."""
import numpy as np
import pytest
import torch

import exact_match_restatement as E

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DESC_ABS = 2.0 ** -23            # one fp32 ulp of 1.0 (tests/test_gpu_exact.py)
LAYOUTS = ('separate', 'interleaved')
_ROWS = {}                       # D -> rows compared, for the report


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for D, n in sorted(_ROWS.items()):
        print('\n[exact matchers D %d] %d output rows compared bit for bit' % (D, n))


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x.astype(np.int64)


def _check(ctx, name, got, want, cov=None, D=None):
    """got == want bit for bit, or a message with the first differing rows and the coverage categories they belong to"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (ctx, name, got.shape, want.shape)
    if D is not None:
        _ROWS[D] = _ROWS.get(D, 0) + (got.shape[0] if got.ndim else 1)
    g, w = _bits(got), _bits(want.astype(got.dtype))
    if np.array_equal(g, w):
        return
    bad = np.nonzero((g != w).reshape(len(g), -1).any(1))[0] if g.ndim else np.array([0])
    first = []
    for i in bad[:6]:
        cat = E.categories_of(cov, int(i)) if cov is not None and i < len(cov['tied']) else ['beyond the count']
        first.append((int(i), got[i].tolist() if got.ndim else got.item(), want[i].tolist() if want.ndim else want.item(), cat))
    pytest.fail('%s %s: %d of %d rows differ; first (row, got, want, coverage): %s' % (ctx, name, len(bad), len(g), first))


def _twice(fn):
    """fn() -> tuple of tensors, launched twice: identical bytes; returns numpy arrays"""
    a = [o.cpu().numpy() for o in fn()]
    torch.cuda.synchronize()
    b = [o.cpu().numpy() for o in fn()]
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes(), 'two launches differ'
    return a


def _layout(pairs, K, D, layout, counts=None, keypoints=False, swap=False):
    """The pairs (dicts with A, B int32 rows and s[, kpA, kpB]) as one batch of capacity K in the separate ([P,K,D] x 2) or
    the interleaved layout (slot 2p = A, 2p + 1 = B; pair_stride, count_stride = 2).  counts: [(nA, nB)] to claim instead of
    the rows present.  Returns (args, kwargs) for match_pairs / nearest_pairs [/ guided_pairs, without H and radius]."""
    P = len(pairs)
    desc = np.zeros((2 * P, K, D), np.float32); cnt = np.zeros(2 * P, np.int32); kp = np.zeros((2 * P, K, 2), np.int32)
    for p, pr in enumerate(pairs):
        sides = [(pr['A'], pr.get('kpA')), (pr['B'], pr.get('kpB'))]
        if swap:
            sides = sides[::-1]
        for side, (rows, k) in enumerate(sides):
            desc[2 * p + side, :len(rows)] = E.as_f32(rows, pr['s'])
            cnt[2 * p + side] = len(rows) if counts is None else counts[p][side]
            if keypoints:
                kp[2 * p + side, :len(rows)] = k
    t = torch.from_numpy(desc).to(DEV); c = torch.from_numpy(cnt).to(DEV); k = torch.from_numpy(kp).to(DEV)
    if layout == 'separate':
        args = [t[0::2].contiguous(), c[0::2].contiguous(), t[1::2].contiguous(), c[1::2].contiguous()]
        if keypoints:
            args += [k[0::2].contiguous(), k[1::2].contiguous()]
        return args, {}
    args = [t, c, t[1:], c[1:]]
    if keypoints:
        args += [k, k[1:]]
    return args, dict(pair_stride=2 * K * D, count_stride=2)


def _pad(x, K, fill):
    out = np.full(K, fill, x.dtype)
    out[:len(x)] = x
    return out


def _nearest_truth(u, s, K, ratio):
    """(match_idx, match_dist, count, second_idx, second_dist), rows at or beyond the count -1 / 0"""
    N, M = u.shape
    nn = E.two_nearest(u)
    d = E.dist_f32(u, s) if M else np.zeros((N, 1), np.float32)
    rows = np.arange(N)
    has1, has2 = nn[:, 0] >= 0, nn[:, 1] >= 0
    d1 = np.where(has1, d[rows, np.maximum(nn[:, 0], 0)], np.float32(0)).astype(np.float32)
    d2 = np.where(has2, d[rows, np.maximum(nn[:, 1], 0)], np.float32(0)).astype(np.float32)
    keep = has1 if ratio is None else E.ratio_keep(d1, d2, has2, ratio)
    return (_pad(np.where(keep, nn[:, 0], -1), K, -1), _pad(np.where(keep, d1, np.float32(0)).astype(np.float32), K, 0),
            int(keep.sum()), _pad(nn[:, 1], K, -1), _pad(d2, K, 0))


def _mutual_truth(u, s, K, threshold, gate=None):
    m, d = E.mutual(u, s, threshold, gate)
    return _pad(m, K, -1), _pad(d, K, 0), int((m >= 0).sum())


# ---- the batched MFMA matchers ----

@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('D', E.WIDTHS)
def test_nearest_two(D, layout):
    """nearest_pairs(ratio=None, return_second=True): both indices, both distances and the counts"""
    from multipoint_amd.utils import nearest_pairs
    pairs = E.batch(D)
    args, kw = _layout(pairs, E.K, D, layout)
    out = _twice(lambda: nearest_pairs(*args, ratio=None, return_second=True, **kw))
    for p, pr in enumerate(pairs):
        ctx = 'D %d %s pair %d %s' % (D, layout, p, E.PAIRS[p])
        want = _nearest_truth(pr['u'], pr['s'], E.K, None)
        for name, g, w in zip(('match_idx', 'match_dist', 'match_count', 'second_idx', 'second_dist'), out, want):
            _check(ctx, name, g[p], w, pr['cov'], D)


@pytest.mark.parametrize('ratio', [0.9, 1.0])
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('D', E.WIDTHS)
def test_ratio(D, layout, ratio):
    """Lowe's test is strict: with ratio = 1.0 a query whose two nearest are equally far is refused"""
    from multipoint_amd.utils import nearest_pairs
    pairs = E.batch(D)
    args, kw = _layout(pairs, E.K, D, layout)
    out = _twice(lambda: nearest_pairs(*args, ratio=ratio, return_second=True, **kw))
    for p, pr in enumerate(pairs):
        ctx = 'D %d %s ratio %s pair %d %s' % (D, layout, ratio, p, E.PAIRS[p])
        want = _nearest_truth(pr['u'], pr['s'], E.K, ratio)
        for name, g, w in zip(('match_idx', 'match_dist', 'match_count', 'second_idx', 'second_dist'), out, want):
            _check(ctx, name, g[p], w, pr['cov'], D)
        if ratio == 1.0:
            near = _nearest_truth(pr['u'], pr['s'], E.K, None)
            tied = np.nonzero((near[3] >= 0) & (near[1] == near[4]))[0]
            assert (out[0][p][tied] == -1).all(), (ctx, 'equal first and second distances kept', tied[:6].tolist())


@pytest.mark.parametrize('threshold', [-1.0, 0.5, 1.0, 2.0])
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('D', E.WIDTHS)
def test_mutual(D, layout, threshold):
    """match_pairs: the integer mutual-NN truth; a pair at distance exactly `threshold` is absent; B against A gives the
    transposed set"""
    from multipoint_amd.utils import match_pairs
    pairs = E.batch(D)
    args, kw = _layout(pairs, E.K, D, layout)
    out = _twice(lambda: match_pairs(*args, threshold=threshold, **kw))
    sargs, skw = _layout(pairs, E.K, D, layout, swap=True)
    back = _twice(lambda: match_pairs(*sargs, threshold=threshold, **skw))
    for p, pr in enumerate(pairs):
        ctx = 'D %d %s threshold %s pair %d %s' % (D, layout, threshold, p, E.PAIRS[p])
        for name, g, w in zip(('match_idx', 'match_dist', 'match_count'), out, _mutual_truth(pr['u'], pr['s'], E.K, threshold)):
            _check(ctx, name, g[p], w, pr['cov'], D)
        for name, g, w in zip(('match_idx', 'match_dist', 'match_count'), back, _mutual_truth(pr['u'].T, pr['s'], E.K, threshold)):
            _check(ctx + ' B against A', name, g[p], w, None, D)
        fwd = {(int(i), int(j)) for i, j in enumerate(out[0][p]) if j >= 0}
        bwd = {(int(i), int(j)) for j, i in enumerate(back[0][p]) if i >= 0}
        assert fwd == bwd, (ctx, 'not the transposed set', sorted(fwd ^ bwd)[:6])
        if threshold >= 0:
            kept = out[1][p][out[0][p] >= 0]
            assert (kept < np.float32(threshold)).all(), (ctx, 'a pair at or beyond the threshold was kept')


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('D', E.WIDTHS)
def test_counts_beyond_the_capacity_are_clamped(D, layout):
    """one pair whose counts say 130 and 200 rows in a batch of capacity 96: the first 96 rows of each side"""
    from multipoint_amd.utils import match_pairs, nearest_pairs
    pr = E.clamp_pair(D)
    K = E.K_CLAMP
    args, kw = _layout([pr], K, D, layout, counts=[E.CLAMP_COUNTS])
    ctx = 'D %d %s clamp' % (D, layout)
    out = _twice(lambda: nearest_pairs(*args, ratio=None, return_second=True, **kw))
    for name, g, w in zip(('match_idx', 'match_dist', 'match_count', 'second_idx', 'second_dist'), out,
                          _nearest_truth(pr['u'], pr['s'], K, None)):
        _check(ctx, 'nearest ' + name, g[0], w, pr['cov'], D)
    out = _twice(lambda: nearest_pairs(*args, ratio=0.9, return_second=True, **kw))
    for name, g, w in zip(('match_idx', 'match_dist', 'match_count', 'second_idx', 'second_dist'), out,
                          _nearest_truth(pr['u'], pr['s'], K, 0.9)):
        _check(ctx, 'ratio ' + name, g[0], w, pr['cov'], D)
    for threshold in (-1.0, 0.5):
        out = _twice(lambda: match_pairs(*args, threshold=threshold, **kw))
        for name, g, w in zip(('match_idx', 'match_dist', 'match_count'), out, _mutual_truth(pr['u'], pr['s'], K, threshold)):
            _check(ctx, 'mutual %s %s' % (threshold, name), g[0], w, pr['cov'], D)


# ---- the guided matcher ----

@pytest.mark.parametrize('threshold', [-1.0, 0.5, 1.0])
@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('D', E.WIDTHS)
def test_guided(D, layout, threshold):
    """guided_pairs at radius 5 on keypoints exactly on, just outside and inside the gate, rows and columns without a
    candidate, the all-zero matrix and rows with w = 0: the gated integer truth"""
    from multipoint_amd.utils import guided_pairs
    pairs = E.gate_batch(D)
    args, kw = _layout(pairs, E.K, D, layout, keypoints=True)
    H = np.stack([pr['H'] for pr in pairs])
    out = _twice(lambda: guided_pairs(*args, H, float(E.RADIUS), threshold=threshold, **kw))
    for p, pr in enumerate(pairs):
        ctx = 'D %d %s guided threshold %s case %d %s' % (D, layout, threshold, p, E.GATE_CASES[p])
        want = _mutual_truth(pr['u'], pr['s'], E.K, threshold, pr['gate'])
        for name, g, w in zip(('match_idx', 'match_dist', 'match_count'), out, want):
            _check(ctx, name, g[p], w, pr['cov'], D)
        N, M = pr['u'].shape
        if N and M:
            # stated on their own: a row without a candidate has no match; every on-boundary partner was a candidate
            empty = ~pr['gate'].any(1)
            assert (out[0][p][:N][empty] == -1).all(), (ctx, 'a row without candidates was matched')
            got = out[0][p][:N]
            assert pr['gate'][np.nonzero(got >= 0)[0], got[got >= 0]].all(), (ctx, 'a match outside the gate')


@pytest.mark.parametrize('D', E.WIDTHS)
def test_guided_with_a_gate_that_covers_the_frame_is_match_pairs(D):
    from multipoint_amd.utils import guided_pairs, match_pairs
    pairs = E.gate_batch(D)
    args, kw = _layout(pairs, E.K, D, 'interleaved', keypoints=True)
    H = np.stack([np.eye(3) for _ in pairs])
    for threshold in (-1.0, 1.0):
        wide = _twice(lambda: guided_pairs(*args, H, 1.0e6, threshold=threshold, **kw))       # (keypoints lie within 2^14)
        plain = _twice(lambda: match_pairs(*args[:4], threshold=threshold, **kw))
        for name, g, w in zip(('match_idx', 'match_dist', 'match_count'), wide, plain):
            for p, pr in enumerate(pairs):
                _check('D %d wide gate threshold %s case %d' % (D, threshold, p), name, g[p], w[p], pr['cov'], D)


# ---- the per-pair routes of get_matches ----

def _dmatches(ms):
    return (np.array([m.queryIdx for m in ms], np.int64), np.array([m.trainIdx for m in ms], np.int64),
            np.array([m.distance for m in ms], np.float64).astype(np.float32))


@pytest.fixture(scope='module', params=range(len(E.SINGLES)), ids=['%dx%d_D%d' % (n, m, d) for d, n, m in E.SINGLES])
def one_pair(request):
    pr = E.single(request.param)
    return pr, E.as_f32(pr['A'], pr['s']), E.as_f32(pr['B'], pr['s']), 'single %s' % (E.SINGLES[request.param],)


def test_get_matches_one_way_and_ratio(one_pair):
    """'bfmatcher' without crossCheck and with knn_matches run the scalar knn2 kernel on squared L2 distances (exact here:
    |a - b|^2 = 2 - 2 a.b); the batched MFMA route must return the same bits, and both the truth"""
    from multipoint_amd.utils import get_matches, nearest_pairs, knn2_pairs
    pr, A, B, ctx = one_pair
    D = A.shape[1]
    N, M = pr['u'].shape
    K = max(N, M)
    idx, dist, cnt, sidx, sdist = _nearest_truth(pr['u'], pr['s'], K, None)
    q, t, d = _dmatches(get_matches(A, B, 'bfmatcher', crossCheck=False))
    _check(ctx, 'bfmatcher queryIdx', q, np.arange(N), None, D)
    _check(ctx, 'bfmatcher trainIdx', t, idx[:N], pr['cov'], D)
    _check(ctx, 'bfmatcher distance', d, dist[:N], pr['cov'], D)
    ridx, rdist, rcnt, _, _ = _nearest_truth(pr['u'], pr['s'], K, 0.9)
    q, t, d = _dmatches(get_matches(A, B, 'bfmatcher', knn_matches=True))
    keep = np.nonzero(ridx[:N] >= 0)[0]
    assert 0 < len(keep) < N
    _check(ctx, 'knn_matches queryIdx', q, keep, None, D)
    _check(ctx, 'knn_matches trainIdx', t, ridx[keep], None, D)
    _check(ctx, 'knn_matches distance', d, rdist[keep], None, D)
    # the two routes against each other on the same padded pair
    dA = torch.zeros((1, K, D), device=DEV); dA[0, :N] = torch.from_numpy(A)
    dB = torch.zeros((1, K, D), device=DEV); dB[0, :M] = torch.from_numpy(B)
    nA = torch.tensor([N], dtype=torch.int32, device=DEV); nB = torch.tensor([M], dtype=torch.int32, device=DEV)
    knn = _twice(lambda: knn2_pairs(dA, nA, dB, nB))
    mfma = _twice(lambda: nearest_pairs(dA, nA, dB, nB, ratio=None, return_second=True))
    _check(ctx, 'knn2 against MFMA nearest idx', knn[0][0, :, 0], mfma[0][0], pr['cov'], D)
    _check(ctx, 'knn2 against MFMA second idx', knn[0][0, :, 1], mfma[3][0], pr['cov'], D)
    _check(ctx, 'knn2 against MFMA nearest dist', knn[1][0, :, 0], mfma[1][0], pr['cov'], D)
    _check(ctx, 'knn2 against MFMA second dist', knn[1][0, :, 1], mfma[4][0], pr['cov'], D)
    _check(ctx, 'MFMA second idx', mfma[3][0], sidx, pr['cov'], D)
    _check(ctx, 'MFMA second dist', mfma[4][0], sdist, pr['cov'], D)
    assert int(mfma[2][0]) == cnt


def test_get_matches_nnmatcher(one_pair):
    from multipoint_amd.utils import get_matches
    pr, A, B, ctx = one_pair
    D = A.shape[1]
    for threshold in (1.0, 0.5):
        m, dist = E.mutual(pr['u'], pr['s'], threshold)
        keep = np.nonzero(m >= 0)[0]
        q, t, d = _dmatches(get_matches(A, B, 'nnmatcher', threshold=threshold))
        _check(ctx, 'nnmatcher %s queryIdx' % threshold, q, keep, None, D)
        _check(ctx, 'nnmatcher %s trainIdx' % threshold, t, m[keep], None, D)
        _check(ctx, 'nnmatcher %s distance' % threshold, d, dist[keep], None, D)


@pytest.mark.parametrize('threshold', [0.5, 1.0])
def test_get_matches_thresholdmatcher(one_pair, threshold):
    """the whole ordered list; 1000 x 1000 at 1.0 overflows the first capacity guess max(4 K, 1024) and is launched again"""
    from multipoint_amd.utils import get_matches
    pr, A, B, ctx = one_pair
    D = A.shape[1]
    ij, dist = E.threshold_list(pr['u'], pr['s'], threshold)
    if pr['u'].shape == (1000, 1000):
        assert len(ij) > max(4 * 1000, 1024)
    q, t, d = _dmatches(get_matches(A, B, 'thresholdmatcher', threshold=threshold))
    assert len(q) == len(ij), (ctx, threshold, len(q), len(ij))
    _check(ctx, 'thresholdmatcher %s queryIdx' % threshold, q, ij[:, 0], None, D)
    _check(ctx, 'thresholdmatcher %s trainIdx' % threshold, t, ij[:, 1], None, D)
    _check(ctx, 'thresholdmatcher %s distance' % threshold, d, dist, None, D)
    assert (d < np.float32(threshold)).all()


# ---- descriptor sampling on the same rows ----

SAMPLE_K = 128
EVEN = [(y, x) for y in range(0, 17, 2) for x in range(0, 17, 2)]         # 81: the coarse map's 9 x 9 pixels, borders included


def _sample_inputs(D, Hc, Wc, seed, zero_image=None):
    """B = 3 maps [Hc, Wc, D] of exact rows (one codebook), keypoints: EVEN first, then points with an odd coordinate;
    counts (K, 0, K + 5)"""
    rng = np.random.default_rng(seed)
    book = E.make_book(rng, D)
    maps = np.stack([E.exact_rows(rng, Hc * Wc, D, book)[0].reshape(Hc, Wc, D) for _ in range(3)])
    if zero_image is not None:
        maps[zero_image] = 0
    odd = [(y, x) for y in range(16) for x in range(16) if (y | x) & 1]
    kp = np.zeros((3, SAMPLE_K, 2), np.int32)
    for b in range(3):
        pick = rng.permutation(len(odd))[:SAMPLE_K - len(EVEN)]
        kp[b] = EVEN + [odd[i] for i in pick]
    cnt = np.array([SAMPLE_K, 0, SAMPLE_K + 5], np.int32)
    return maps, book['s'], kp, cnt


def _sample(maps, s, kp, cnt):
    from multipoint_amd.utils.utils import interpolate_descriptors_batched
    desc = torch.from_numpy(E.as_f32(maps, s)).permute(0, 3, 1, 2).to(DEV)          # (B, D, Hc, Wc) logical
    k = torch.from_numpy(kp).to(DEV); c = torch.from_numpy(cnt).to(DEV)
    return _twice(lambda: (interpolate_descriptors_batched(k, c, desc, 16, 16),))[0]


@pytest.mark.parametrize('D', [64, 128, 192, 256])
def test_sampling(D):
    """H = W = 16 over a 9 x 9 map: iy = y / 2 exactly in the kernel's own fp32 steps.  Even coordinates: the map's row bit
    for bit (weights 0 / 1, sum of squares exactly 1).  Odd coordinates: within DESC_ABS of float64."""
    maps, s, kp, cnt = _sample_inputs(D, 9, 9, 40 + D)
    out = _sample(maps, s, kp, cnt)
    assert out.shape == (3, SAMPLE_K, D) and np.isfinite(out).all()
    assert not out[1].any(), 'rows beyond the count (0) are not zero'
    ne = len(EVEN)
    for b in (0, 2):
        ctx = 'D %d image %d' % (D, b)
        want = np.stack([maps[b, y // 2, x // 2] for y, x in EVEN])
        _check(ctx, 'rows at even coordinates', out[b, :ne], E.as_f32(want, s))
        truth = E.sample_truth(maps[b], s, kp[b], 16, 16)
        err = np.abs(out[b].astype(np.float64) - truth)
        print('%s: max |out - float64| at odd coordinates %.3g' % (ctx, err[ne:].max()))
        worst = int(err.max(1).argmax())
        assert err.max() <= DESC_ABS, (ctx, 'keypoint', kp[b, worst].tolist(), float(err.max()))


@pytest.mark.parametrize('Hc,Wc', [(1, 9), (9, 1), (1, 1)])
def test_sampling_degenerate_maps(Hc, Wc):
    """a one-row (one-column) map gives that row (column) everywhere; an all-zero map gives zeros (the 1e-12 floor), not NaN"""
    D = 128
    maps, s, kp, cnt = _sample_inputs(D, Hc, Wc, 77 + Hc + 2 * Wc, zero_image=2)
    out = _sample(maps, s, kp, cnt)
    assert np.isfinite(out).all()
    assert not out[1].any() and not out[2].any()
    exact = [n for n, (y, x) in enumerate(kp[0]) if (Hc == 1 or y % 2 == 0) and (Wc == 1 or x % 2 == 0)]
    assert len(exact) > len(EVEN) or (Hc, Wc) == (9, 9)
    want = np.stack([maps[0, 0 if Hc == 1 else kp[0, n, 0] // 2, 0 if Wc == 1 else kp[0, n, 1] // 2] for n in exact])
    _check('map %d x %d' % (Hc, Wc), 'rows on the map\'s pixels', out[0, exact], E.as_f32(want, s))
    truth = E.sample_truth(maps[0], s, kp[0], 16, 16)
    assert np.abs(out[0].astype(np.float64) - truth).max() <= DESC_ABS


@pytest.mark.parametrize('D', E.WIDTHS)
def test_sampled_rows_go_straight_into_the_matcher(D):
    """the chain the pipeline runs: rows sampled at even coordinates of two images, matched: the integer truth"""
    from multipoint_amd.utils import match_pairs
    from multipoint_amd.utils.utils import interpolate_descriptors_batched
    maps, s, kp, cnt = _sample_inputs(D, 9, 9, 40 + D)
    desc = torch.from_numpy(E.as_f32(maps, s)).permute(0, 3, 1, 2).to(DEV)
    out = interpolate_descriptors_batched(torch.from_numpy(kp).to(DEV), torch.from_numpy(cnt).to(DEV), desc, 16, 16)
    ne = len(EVEN)
    n = torch.tensor([ne], dtype=torch.int32, device=DEV)
    got = _twice(lambda: match_pairs(out[0:1], n, out[2:3], n))
    u = E.u_int(maps[0].reshape(ne, D), maps[2].reshape(ne, D), s)
    cov = E.coverage(u, ne)
    assert cov['tied'].sum() > 0
    for name, g, w in zip(('match_idx', 'match_dist', 'match_count'), got, _mutual_truth(u, s, SAMPLE_K, -1.0)):
        _check('D %d sampled chain' % D, name, g[0], w, cov, D)
