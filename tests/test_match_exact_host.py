"""CPU: the premise of tests/test_gpu_match_exact.py, checked on every input it uses (tests/exact_match_restatement.py).

The GPU tests demand bit equality with an integer truth.  That is only fair if ANY fp32 evaluation of the inputs returns that
truth, and only decisive if the inputs hold the ties, the on-threshold distances and the on-boundary keypoints the kernels'
rules are about.  These are conditions on the inputs: if a seed misses one, change the seed, not the condition."""
from fractions import Fraction

import numpy as np
import pytest

import exact_match_restatement as E


def _all_pairs():
    for D in E.WIDTHS:
        for c, p in enumerate(E.batch(D)):
            yield 'D %d pair %d %s' % (D, c, E.PAIRS[c]), D, p
        yield 'D %d clamp pair' % D, D, E.clamp_pair(D)
        for c, p in enumerate(E.gate_batch(D)):
            yield 'D %d gate case %d %s' % (D, c, E.GATE_CASES[c]), D, p
    for k, (D, N, M) in enumerate(E.SINGLES):
        yield 'single %d %s' % (k, E.SINGLES[k]), D, E.single(k)


def _dot_f32(a, b, order):
    """A . B^T accumulated in fp32, one channel at a time in `order`"""
    acc = np.zeros((len(a), len(b)), np.float32)
    for c in order:
        acc = (acc + a[:, c, None] * b[None, :, c]).astype(np.float32)
    return acc


def test_fp32_accumulation_in_any_order_is_the_integer_truth():
    rows = 0
    for ctx, D, p in _all_pairs():
        a, b, s = E.as_f32(p['A'], p['s']), E.as_f32(p['B'], p['s']), p['s']
        if len(a) == 0 or len(b) == 0:
            continue
        # the large single pairs: a 120 x 120 corner is the same arithmetic
        a, b, u = a[:120], b[:120], p['u'][:120, :120]
        for order in (np.arange(D), np.random.default_rng(D).permutation(D)):
            dot = _dot_f32(a, b, order)
            t = np.minimum(np.maximum(dot, np.float32(-1)), np.float32(1))
            got = np.float32(2) - np.float32(2) * t                              # the kernels' u, in fp32
            assert got.dtype == np.float32
            assert np.array_equal(got.astype(np.float64) * (s * s), u.astype(np.float64)), ctx
            # the scalar knn2 route: fp32 sum of squared differences
            e = a[:, None, :] - b[None, :, :]
            sq = np.zeros(e.shape[:2], np.float32)
            for c in order:
                sq = (sq + e[:, :, c] * e[:, :, c]).astype(np.float32)
            assert np.array_equal(sq.astype(np.float64) * (s * s), u.astype(np.float64)), ctx
        rows += len(a)
    assert rows > 0


def test_rows_have_norm_exactly_one():
    for ctx, D, p in _all_pairs():
        for r in (p['A'], p['B']):
            assert set(np.unique(r).tolist()) <= {-1, 0, 1}, ctx
            assert ((r.astype(np.int64) ** 2).sum(1) == p['s'] ** 2).all(), ctx
            f = E.as_f32(r, p['s'])
            assert np.array_equal(f.astype(np.float64) * p['s'], r.astype(np.float64)), ctx        # no rounding
            acc = np.zeros(len(f), np.float32)
            for c in range(D):
                acc = (acc + f[:, c] * f[:, c]).astype(np.float32)
            assert (acc == np.float32(1)).all(), ctx
        if D == 128:                                               # A and B share one zero pattern of 64 channels
            zero = ~np.isin(np.arange(D), p['book']['nz'])
            assert zero.sum() == 64 and not p['A'][:, zero].any() and not p['B'][:, zero].any(), ctx


def test_distance_is_strictly_monotone_in_u():
    """sorting by (u_int, index) is sorting by (fp32 distance bits, index): no two attained u share a distance"""
    for D in E.WIDTHS:
        s = E.scale_of(D)
        d = E.dist_f32(np.arange(0, 4 * s * s + 1, 4, dtype=np.int64), s)
        assert (np.diff(d.view(np.int32)) > 0).all()
        assert d[0] == 0 and d[-1] == 2
        # float64 sqrt rounded once more equals the correctly rounded fp32 sqrt of the (exact) fp32 u
        u32 = (np.arange(0, 4 * s * s + 1, 4) / (s * s)).astype(np.float32)
        for x, got in zip(u32[1:], d[1:]):
            r = Fraction(float(got)); lo = Fraction(float(np.nextafter(got, np.float32(-1)))); hi = Fraction(float(np.nextafter(got, np.float32(3))))
            assert ((r + lo) / 2) ** 2 <= Fraction(float(x)) <= ((r + hi) / 2) ** 2


@pytest.mark.parametrize('D', E.WIDTHS)
def test_coverage_is_nonzero_in_every_category(D):
    total = {}
    for p in E.batch(D):
        for k, v in p['cov'].items():
            total[k] = total.get(k, 0) + int(v.sum())
    print('D %d coverage over the batch: %s' % (D, total))
    assert all(v > 0 for v in total.values()), total
    assert set(total) == {'tied'} | {t + c for t in ('tie_', 'top2_') for c in E.CATEGORIES}


def test_single_pairs_cover_every_category():
    for k in range(len(E.SINGLES)):
        cov = E.single(k)['cov']
        assert all(int(v.sum()) > 0 for v in cov.values()), (k, {a: int(b.sum()) for a, b in cov.items()})


def test_large_pairs_are_mostly_tied():
    seen = 0
    for ctx, D, p in _all_pairs():
        N, M = p['u'].shape
        if N * M >= E.LARGE ** 2:
            seen += 1
            assert 2 * int(p['cov']['tied'].sum()) >= N, (ctx, int(p['cov']['tied'].sum()), N)
    assert seen >= 2 * len(E.WIDTHS) + len(E.SINGLES)


def test_planted_distances_exist_and_sit_on_the_thresholds():
    for ctx, D, p in _all_pairs():
        N, M = p['u'].shape
        pl, s = p['planted'], p['s']
        if N < 30 or M < 30:
            continue
        d = E.dist_f32(p['u'], s)
        match, dist = E.mutual(p['u'], s)
        assert d[pl['duplicate']] == 0 and d[pl['opposite']] == 2, ctx
        for name, want in (('half', 0.5), ('one', 1.0)):
            i, j = pl[name]
            assert d[i, j] == np.float32(want), ctx
            assert match[i] == j and dist[i] == np.float32(want), (ctx, name)          # a mutual match ON the threshold ...
            cut, _ = E.mutual(p['u'], s, threshold=want)
            assert cut[i] == -1, (ctx, name)                                           # ... which the strict test refuses
            assert (cut >= 0).sum() < (match >= 0).sum()
        i, j = pl['half']
        assert (p['u'][i] == p['u'][i, j]).sum() >= 2, ctx                             # the d = 0.5 partner is tied
    for D in E.WIDTHS:
        b = E.batch(D)
        p = b[E.PAIRS.index((3, 1))]                                                     # the mutual match at d = 2 exactly
        assert E.mutual(p['u'], p['s'])[0].tolist() == [0, -1, -1] and E.mutual(p['u'], p['s'], 2.0)[0].tolist() == [-1, -1, -1]
        p = b[E.PAIRS.index((5, 2))]
        assert E.two_nearest(p['u'])[0].tolist() == [0, 1] and E.dist_f32(p['u'], p['s'])[0].tolist() == [0.0, 2.0]


def test_ratio_one_refuses_equal_distances():
    for D in E.WIDTHS:
        equal = kept9 = kept1 = total = 0
        for p in E.batch(D):
            if p['u'].shape[0] == 0 or p['u'].shape[1] < 2:
                continue
            nn = E.two_nearest(p['u']); d = E.dist_f32(p['u'], p['s']); rows = np.arange(len(nn))
            d1, d2 = d[rows, nn[:, 0]], d[rows, nn[:, 1]]
            k1, k9 = E.ratio_keep(d1, d2, nn[:, 1] >= 0, 1.0), E.ratio_keep(d1, d2, nn[:, 1] >= 0, 0.9)
            assert not k1[d1 == d2].any() and k1[d1 < d2].all()
            equal += int((d1 == d2).sum()); kept9 += int(k9.sum()); kept1 += int(k1.sum()); total += len(rows)
        # the two ratios decide differently, neither keeps or drops all
        assert equal > 0 and 0 < kept9 < kept1 < total, (D, equal, kept9, kept1, total)


def test_gate_inputs():
    for D in E.WIDTHS:
        seen = set()
        for c, p in enumerate(E.gate_batch(D)):
            name, N, M = E.GATE_CASES[c]
            ctx = 'D %d gate case %d %s' % (D, c, name)
            gate = p['gate']
            X, Y, W = E.warp_int(name, p['kpA'])
            H = p['H']
            # the kernel's double arithmetic is exact and its fp32 positions are the rationals themselves
            for i in range(N):
                x, y = int(p['kpA'][i, 1]), int(p['kpA'][i, 0])
                w = H[2, 0] * x + H[2, 1] * y + H[2, 2]
                q = E.HOMOGRAPHIES[name][1]
                assert Fraction(w) == Fraction(int(W[i]), q), ctx
                if W[i] != 0:
                    for num, row in ((X[i], 0), (Y[i], 1)):
                        v = np.float32((H[row, 0] * x + H[row, 1] * y + H[row, 2]) / w)
                        assert Fraction(float(v)) == Fraction(int(num), int(W[i])), ctx
                        assert (2 * int(num)) % int(W[i]) == 0 and abs(v) < 2 ** 14, ctx      # half-integers: fp32 differences are exact
            assert np.abs(p['kpB']).max(initial=0) < 2 ** 14
            # the integer gate against exact rationals, offset by offset
            for j, i, (dx, dy) in p['offsets']:
                ex = Fraction(int(X[i]), int(W[i])) - int(p['kpB'][j, 1]); ey = Fraction(int(Y[i]), int(W[i])) - int(p['kpB'][j, 0])
                assert (ex, ey) == (-dx, -dy), ctx
                assert bool(gate[i, j]) == (dx * dx + dy * dy <= E.RADIUS ** 2), ctx
                seen.add((name, 'on' if (dx, dy) in E.ON_BOUNDARY else 'outside' if (dx, dy) in E.JUST_OUTSIDE else 'other'))
            if N and M:
                if name == 'zero':
                    assert not gate.any() and (W == 0).all(), ctx
                elif min(N, M) >= 30:
                    assert (~gate.any(1)).sum() > 0 and (~gate.any(0)).sum() > 0, ctx          # no-candidate rows and columns
                    assert gate.any(1).sum() > 0, ctx
                    # the gate changes the answer: some gated winner is not the ungated one
                    assert (E.mutual(p['u'], p['s'], gate=gate)[0] != E.mutual(p['u'], p['s'])[0]).any(), ctx
                if name == 'w_zero':
                    assert 0 < (W == 0).sum() < N and not gate[W == 0].any(), ctx
                if name == 'projective':
                    assert set(np.unique(W).tolist()) == {1, 2, 4}, ctx
        # some gated mutual match sits ON the thresholds 0.5 and 1.0 (guided_mutual_kernel's `d < threshold` is strict)
        for want in (0.5, 1.0):
            cut = 0
            for p in E.gate_batch(D):
                m, d = E.mutual(p['u'], p['s'], gate=p['gate'])
                cut += int(((m >= 0) & (d == np.float32(want))).sum())
            assert cut > 0, (D, want)
        for name in ('identity', 'shift', 'half', 'projective', 'w_zero'):
            assert (name, 'on') in seen and (name, 'outside') in seen, (D, name, sorted(seen))
    assert (3, 4) in E.ON_BOUNDARY and (5, 0) in E.ON_BOUNDARY and (4, 4) in E.JUST_OUTSIDE and E.RADIUS == 5


def test_sample_truth_at_even_coordinates_is_the_map_row():
    rng = np.random.default_rng(3)
    for D in (64, 128, 192, 256):
        rows, s = E.exact_rows(rng, 81, D)
        m = rows.reshape(9, 9, D)
        kp = np.array([(y, x) for y in range(0, 17, 2) for x in range(0, 17, 2)])
        out = E.sample_truth(m, s, kp, 16, 16)
        assert np.array_equal(out, m.reshape(81, D) / s)
        assert ((rows.astype(np.int64) ** 2).sum(1) == s * s).all()
