"""Warp, adaptation and descriptor-sampling kernels, host side (no GPU): the premises of tests/test_gpu_sampling_shapes.py.

  * tests/sampling_restatement.py (numpy float64, written from the comments of homog_adapt.hip and sample_desc.hip) agrees with
    the oracle's restatement of the reference -- kornia's warp in float32 normalised coordinates within the tolerances
    tests/test_gpu_ha.py documents for that difference, cv2's valid mask bit for bit, the reflect-padded Gaussian filter, the
    reference's adaptation loop (with an identity "network") and its descriptor interpolation, the committed sampling.npz;
  * the cases of tests/sampling_cases.py stand on both sides of every tile edge, and on every one of them at most 1 % of the
    pixels are near a rounding tie or carry a bound that says nothing -- none at all under the exact matrices;
  * every deliberately wrong restatement of R.MUTANTS is told apart from the true one by more than the bound on at least one
    committed case (on the discrete outputs: in a pixel that is neither near a tie nor vacuous).

`pytest -s` prints the near-tie and vacuous counts of every case."""
import os

import numpy as np
import pytest
import torch

import sampling_cases as C
import sampling_restatement as R
from oracle import ha_oracle as HA

CAP = 0.01
_WARP = {}


def warp_result(case, mode, pad, mutant=None):
    key = (case['name'], mode, pad, mutant)
    if key not in _WARP:
        _WARP[key] = R.warp(case['src'], case['hom'], case['dsize'], mode, pad, mutant)
    return _WARP[key]


WARP_CASES = C.warp_cases()
WARP_RUNS = [(c, m, p) for c in WARP_CASES for m, p in C.WARP_VARIANTS if p in c['paddings']]
ACC_CASES = C.accumulate_cases()
DESC_CASES = C.desc_cases()


# ---- the cases stand on both sides of every tile edge ----
def test_frames_cover_both_sides_of_every_tile_edge():
    def both_sides(values, edge):
        return min(values) < edge and edge in values and max(values) > edge
    assert both_sides([W for _, W in C.FRAMES], 64) and both_sides([H for H, _ in C.FRAMES], 4)
    assert any(W > 128 for _, W in C.FRAMES) and any(H > 8 for H, _ in C.FRAMES)           # more than two blocks each way
    assert both_sides([W for _, W in C.MASK_FRAMES], 32) and both_sides([H for H, _ in C.MASK_FRAMES], 32)
    assert any(W > 64 for _, W in C.MASK_FRAMES) and max(C.MASK_RADII) == 16 and min(C.MASK_RADII) == 0
    for k in C.FILTER_SIZES:
        r = (k - 1) // 2
        fr = C.filter_frames(k)
        assert (r + 1, 64) in fr and all(H > r and W > r for H, W in fr)
        assert ((5, r + 1) if r < 5 else (r + 1, r + 1)) in fr                  # the smallest legal width at every k
        assert r >= 4 or (both_sides([W for _, W in fr], 64) and both_sides([H for H, _ in fr], 4))
    assert max(C.FILTER_SIZES) == 31 and min(C.FILTER_SIZES) == 1
    # descriptor rows: 4 waves per block, B*K on both sides of a multiple of 4; every D the kernel takes
    assert {(B * K) % 4 for B, K in C.DESC_BK} >= {0, 1} and {c['desc'].shape[3] for c in DESC_CASES} == {64, 128, 192, 256, 320, 384}
    assert {(c['desc'].shape[1] == 1, c['desc'].shape[2] == 1) for c in DESC_CASES} >= {(True, False), (False, True), (False, False)}
    for c in DESC_CASES:
        K = c['kp'].shape[1]
        assert c['kp'].shape[0] * K <= 128 and all(int(n) in (0, 1, K - 1, K, K + 3) for n in c['count'])
    counts = {(int(n) > c['kp'].shape[1], int(n) == 0) for c in DESC_CASES for n in c['count']}
    assert (True, False) in counts and (False, True) in counts
    assert {tuple(s[1:]) for s in C.POINTWISE_SHAPES} and sorted(int(np.prod(s)) for s in C.POINTWISE_SHAPES) == [1, 255, 256, 257]
    for c in WARP_CASES:
        assert c['src'].shape[0] <= 7 and len(c['hom']) <= 7 and c['dsize'][0] <= 50 and c['dsize'][1] <= 200
        assert c['exact'] == all(R.is_exact_matrix(m) for m in c['hom']), c['name']
    sizes = {(c['src'].shape[0], len(c['hom'])) for c in WARP_CASES}
    assert (3, 7) in sizes and (7, 7) in sizes
    rel = {(np.sign(c['dsize'][0] - c['src'].shape[1]), np.sign(c['dsize'][1] - c['src'].shape[2])) for c in WARP_CASES}
    assert rel >= {(-1, -1), (0, 0), (1, 1)}


# ---- caps: conditions on the reference alone ----
@pytest.mark.parametrize('case', WARP_CASES, ids=lambda c: c['name'])
def test_warp_case_caps(case):
    for mode, pad in C.WARP_VARIANTS:
        if pad not in case['paddings']:
            continue
        r = warp_result(case, mode, pad)
        tie, vac = int(r['tie'].sum()), int(r['vacuous'].sum())
        print('warp %-26s %-8s %-10s near-tie %3d vacuous %3d of %d' % (case['name'], mode, pad, tie, vac, r['want'].size))
        assert tie <= CAP * r['want'].size and vac <= CAP * r['want'].size, (case['name'], mode, pad, tie, vac)
        if case['exact']:
            assert tie == 0 and vac == 0
        assert np.isfinite(r['want']).all()
    if 'proj' in case['name'] and case['dsize'][1] > 8:
        assert (~R.project(case['hom'][-1], *case['dsize'])[4]).sum() == case['dsize'][0]       # the column at infinity


def _acc(case, mutant=None):
    return R.accumulate(case['pa'], case['pb'], case['mask'], case['hom'], case['B'], case['agg'], case['prob0'], case['count0'],
                        mutant)


@pytest.mark.parametrize('case', ACC_CASES, ids=lambda c: c['name'])
def test_accumulate_case_caps(case):
    r = _acc(case)
    tie = int(r['tie'].sum())
    vac = int((r['bound'] > R.VACUOUS_FRACTION * np.abs(r['prob']).max()).sum())
    print('accumulate %-22s near-tie %3d vacuous %3d of %d' % (case['name'], tie, vac, r['prob'].size))
    assert tie <= CAP * r['prob'].size and vac <= CAP * r['prob'].size
    assert np.array_equal(r['count'], np.rint(r['count'])) and (r['count_lo'] <= r['count']).all() and (r['count'] <= r['count_hi']).all()
    assert (r['count'] != case['count0']).any() or case['W'] < 9
    if case['W'] > 8 and any(np.array_equal(m, C.Z0_MATRIX) for m in case['hom']):
        assert case['mask'][:, 0, 0].all()


# ---- the restatement against the oracle ----
DYADIC_FRAME = (5, 65)               # H - 1 = 4, W - 1 = 64: the oracle's float32 normalised coordinates are exact there
ORACLE_NEAREST_EXACT = [0, 1, 3, 4, 5]     # identity, integer shift, flips, outside shift; not the half shifts (ties in float32)


def _oracle_exact_set(case, mode, pad, got, want):
    """The exact-matrix set against the float32 oracle.  On the 5 x 65 frames the oracle's normalised coordinates are dyadic, so
    all seven matrices -- the half shifts that tie to even, the wholly-outside shift, the multiple reflections -- are compared
    without tolerance: equal in nearest mode and, on the one-pixel sources, in all four variants; bilinear on noise within the
    oracle's own float32 rounding of a value below 1 (2^-23), and within one float32 step of a coordinate of 1000 px under
    reflection.  On the other frames nearest is equal on the integer matrices; bilinear keeps the float32 tolerance
    test_gpu_ha.py documents (1e-5, growing by 2e-7 per pixel of the largest coordinate); the half shifts in nearest mode are
    ties for the float32 oracle there and are not compared."""
    diff = np.abs(got - want)
    name = (case['name'], mode, pad)
    if case['src'].shape[1:] == DYADIC_FRAME and tuple(case['dsize']) == DYADIC_FRAME:
        if mode == 'nearest' or case['name'].startswith('corner'):
            assert np.array_equal(got, want), name
        else:
            far = 1000.0 * 2.0 ** -23 if pad == 'reflection' else 0.0
            assert diff[[0, 1, 2, 3, 4, 6]].max() <= 2.0 ** -23 and diff[5].max() <= max(far, 2.0 ** -23), (name, diff.max())
        return
    if mode == 'nearest':
        assert np.array_equal(got[ORACLE_NEAREST_EXACT], want[ORACLE_NEAREST_EXACT]), name
        return
    size = max(case['src'].shape[1:] + tuple(case['dsize']))
    for n, m in enumerate(case['hom']):
        reach = max(size, np.abs(m[:2, 2]).max())
        assert diff[n].max() <= max(1e-5, 2e-7 * reach), (name, n, diff[n].max())


@pytest.mark.parametrize('case', [c for c in WARP_CASES if min(c['src'].shape[1:]) > 1 and min(c['dsize']) > 1 and c['name'] != 'far_5x65'],
                         ids=lambda c: c['name'])
def test_warp_against_oracle(case):
    """kornia evaluates the warp in float32 NORMALISED coordinates: ~1e-5 px off at 64x64, ~1e-4 px at 480x640 (test_gpu_ha.py).
    Exact matrices: _oracle_exact_set.  Sampled homographies: <= 2e-3 on bilinear samples of white noise up to 160 px and in
    proportion beyond (mean <= 2e-5), a bounded number of differing pixels for nearest.  Pixels the bound already calls vacuous
    or near a tie, and those projected further than 1000 px away (where float32 normalised coordinates lose the pixel), are left
    out."""
    n_out = len(case['hom'])
    src = torch.from_numpy(np.stack([case['src'][n % len(case['src'])] for n in range(n_out)]))[:, None]
    M = torch.from_numpy(np.linalg.inv(case['hom']).astype(np.float32))
    size = max(case['src'].shape[1:] + tuple(case['dsize']))
    tol = 2e-3 * max(1.0, size / 160.0)
    for mode, pad in C.WARP_VARIANTS:
        r = warp_result(case, mode, pad)
        want = HA.warp_perspective(src, M, case['dsize'], mode, pad)[:, 0].numpy().astype(np.float64)
        diff = np.abs(r['want'] - want)
        if case['exact']:
            _oracle_exact_set(case, mode, pad, r['want'], want)
            continue
        keep = ~r['tie'] & ~r['vacuous']
        for n in range(n_out):
            u, v, _, _, ok = R.project(case['hom'][n], *case['dsize'])
            with np.errstate(invalid='ignore'):
                keep[n] &= ok & (np.abs(u) < 1e3) & (np.abs(v) < 1e3)
        if mode == 'bilinear':
            assert diff[keep].max() <= tol and diff[keep].mean() <= 2e-5, (case['name'], pad, diff[keep].max())
        else:
            assert (diff[keep] != 0).sum() <= max(2, 2e-3 * keep.sum()), (case['name'], pad, int((diff[keep] != 0).sum()))


@pytest.mark.parametrize('H,W', C.MASK_FRAMES)
def test_valid_mask_against_oracle(H, W):
    for h in np.linalg.inv(C.mask_homographies(H, W)):
        inv = np.linalg.inv(h)
        for r in C.MASK_RADII + [3]:
            for border in (False, True):
                want = HA.compute_valid_mask((H, W), h, r, border)
                assert np.array_equal(R.valid_mask(inv, H, W, r, border)[0], want.astype(np.uint8)), (r, border)
    masks = R.valid_mask(C.mask_homographies(H, W), H, W, 1, True)
    assert masks.shape == (C.MASK_G, H, W) and len({m.tobytes() for m in masks}) >= (3 if H > 5 else 2)     # blockIdx.z matters


@pytest.mark.parametrize('k', C.FILTER_SIZES)
def test_filter_against_oracle(k):
    for H, W in C.filter_frames(k):
        x = C.filter_input(k, H, W)
        want = HA.smooth(torch.from_numpy(x)[:, None], k)[:, 0].numpy()
        w = C.filter_weights('gaussian', k)
        assert np.abs(w - HA.gaussian_weights(k)[0, 0].numpy()).max() <= 1e-7
        got, bound = R.gaussian_filter(x, w)
        assert (np.abs(got - want) <= 1e-6 + bound).all(), (k, H, W)       # the oracle sums k^2 float32 products itself
        assert bound.max() <= (k * k + 1) * R.U * 1.01 + 1e-30           # sum|in * w| <= max|in| * sum w
        # the table that is 1 at one off-centre position: the expected output is a reflected shift of the input
        dy, dx = C.one_hot_position(k)
        r = (k - 1) // 2
        got, _ = R.gaussian_filter(x, C.filter_weights('one_hot', k))
        yy, xx = np.abs(np.arange(H) + dy - r), np.arange(W) + dx - r
        xx = np.where(xx >= W, 2 * (W - 1) - xx, xx)
        assert np.array_equal(got, x[:, yy[:, None], xx[None, :]].astype(np.float64))


def _chain(images, homs, cfg, agg):
    """begin -> (warp, valid mask, accumulate) per view -> finalize, as multipoint_amd.utils.homographies._adapt drives them"""
    B, H, W = images[0].shape
    prob, count = R.begin(images[0], images[1] if agg else None, agg)
    h32 = homs.astype(np.float32).astype(np.float64)
    for g in range(len(homs)):
        per_image = np.repeat(np.linalg.inv(h32[g:g + 1]), B, axis=0)
        maps = [R.warp(img, per_image, (H, W), 'bilinear', 'reflection')['want'].astype(np.float32) for img in images]
        mask = R.valid_mask(np.linalg.inv(homs[g:g + 1]), H, W, cfg['erosion_radius'], cfg['mask_border'])
        a = R.accumulate(maps[0], maps[1] if agg else None, mask, h32[g:g + 1], B, agg, prob, count)
        prob, count = a['prob'].astype(np.float32), a['count'].astype(np.float32)
    return R.finalize(prob, count, agg, cfg['min_count']), count


@pytest.mark.parametrize('agg,name', [(0, None), (1, 'prod'), (2, 'sum')])
def test_chain_against_oracle(agg, name):
    """the reference's loop with forward_fn returning its input; the tolerance is the driver test's (test_gpu_ha.py): pixels
    whose valid count differs by one view change by O(prob / count)"""
    H, W, B = 40, 56, 2
    cfg = {'num': 4, 'erosion_radius': 2, 'mask_border': True, 'min_count': 2, 'filter_size': 0}
    homs = C.sampled_homographies(7, 3, H, W, **HA.DEFAULT_CONFIG['homographies'])
    images = [C.noise(8, B, H, W), C.noise(9, B, H, W)][:2 if agg else 1]
    want, want_count = HA.homographic_adaptation([torch.from_numpy(i)[:, None] for i in images], lambda i, x: x, cfg, homs, name)
    got, count = _chain(images, homs, cfg, agg)
    diff = np.abs(got - want[:, 0].numpy())
    assert (count != want_count[:, 0].numpy()).mean() <= 5e-3
    assert (diff > 1e-4).mean() <= 5e-3 and np.median(diff) <= 1e-6 and diff.mean() <= 2e-5, ((diff > 1e-4).mean(), diff.mean())


@pytest.mark.parametrize('case', DESC_CASES, ids=lambda c: c['name'])
def test_descriptors_against_oracle(case, oracle):
    """the oracle evaluates the same chain in float32: it must lie within the restatement's own bound"""
    r = R.sample_descriptors(case['desc'], case['H'], case['W'], case['kp'], case['count'])
    B, K = case['kp'].shape[:2]
    low = np.zeros((B, K), bool)
    for b, k in case['low_norm_rows']:
        low[b, k] = True
    # the listed rows are exactly the rows whose norm is decided by the floor or by cancellation
    assert np.array_equal(low, r['valid'] & (r['norm'] < 1e-6) & (r['norm'] > 0)), case['name']
    for b, k in case['zero_rows']:
        assert r['valid'][b, k] and r['norm'][b, k] == 0.0 and not r['want'][b, k].any()
    assert (r['tap_ratio'][~low] <= 4.0).all(), r['tap_ratio'].max()
    assert not r['want'][~r['valid']].any()
    assert np.abs(np.linalg.norm(r['want'], axis=-1)[r['valid'] & (r['norm'] >= 1e-6)] - 1).max(initial=0) <= 1e-12
    for b in range(B):
        n = int(r['valid'][b].sum())
        if n == 0:
            continue
        rows = oracle.interpolate_descriptors(case['kp'][b, :n], case['desc'][b].transpose(2, 0, 1), case['H'], case['W'])
        ok = ~low[b, :n]
        assert (np.abs(rows - r['want'][b, :n])[ok] <= r['bound'][b, :n][ok]).all(), (case['name'], b)


def test_descriptors_against_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, 'sampling.npz'))
    kp = g['keypoints'].astype(np.int32)[None]
    r = R.sample_descriptors(g['desc'].transpose(1, 2, 0)[None], int(g['H']), int(g['W']), kp, [kp.shape[1]])
    assert (np.abs(r['want'][0] - g['rows']) <= r['bound'][0]).all()


def test_pointwise_restatements():
    """begin and finalize are single IEEE operations; the cases hold what they must"""
    for shape in C.POINTWISE_SHAPES:
        for agg in C.AGGREGATIONS:
            c = C.pointwise_case(shape, agg)
            prob, count = R.begin(c['pa'], c['pb'], agg)
            want = [c['pa'], c['pa'] * c['pb'], c['pa'] + c['pb']][agg]
            assert np.array_equal(prob, want) and (count == 1).all() and prob.dtype == np.float32
            if np.prod(shape) >= 255:
                assert set(np.unique(c['count'])) == {0.0, 1.0, 2.0, 2.5, 3.0} and set(C.MIN_COUNTS) - {0.0} <= set(np.unique(c['count']))
                assert ((c['prob'] == 0) & (c['count'] == 0)).any() and (c['prob'] < 0).any()
                out = R.finalize(c['prob'], c['count'], agg, 0.0)
                assert np.isnan(out).any() and np.isinf(out).any()
                assert np.isfinite(R.finalize(c['prob'], c['count'], agg, 1.0)[c['count'] == 0]).all()


# ---- every mutant is told apart ----
def _separated(want, mut, bound, usable):
    want, mut = np.asarray(want, np.float64), np.asarray(mut, np.float64)
    with np.errstate(invalid='ignore'):
        same = (want == mut) | (np.isnan(want) & np.isnan(mut))
        d = np.where(same, 0.0, np.abs(mut - want))
        d = np.where(np.isnan(d), np.inf, d)
        return bool(((d > bound) & usable).any())


def _warp_separates(mutant):
    for case, mode, pad in WARP_RUNS:
        if case['src'].size > 7 * 5 * 65:
            continue                                        # the small frames are enough; keeps the test quick
        r, m = warp_result(case, mode, pad), warp_result(case, mode, pad, mutant)
        if _separated(r['want'], m['want'], r['bound'], ~r['tie'] & ~r['vacuous']):
            return case['name'], mode, pad
    return None


def _filter_separates(mutant):
    for k in C.FILTER_SIZES:
        for kind in C.FILTER_WEIGHTS:
            for H, W in C.filter_frames(k)[:2]:
                x, w = C.filter_input(k, H, W), C.filter_weights(kind, k)
                want, bound = R.gaussian_filter(x, w)
                if _separated(want, R.gaussian_filter(x, w, mutant)[0], bound, True):
                    return k, kind, H, W
    return None


def _accumulate_separates(mutant):
    for case in ACC_CASES:
        if case['H'] > 5:
            continue
        r, m = _acc(case), _acc(case, mutant)
        usable = ~r['tie'] & (r['bound'] <= R.VACUOUS_FRACTION * np.abs(r['prob']).max())
        if _separated(r['prob'], m['prob'], r['bound'], usable) or _separated(r['count'], m['count'], 0.0, usable):
            return case['name']
    return None


def _finalize_separates(mutant):
    for shape in C.POINTWISE_SHAPES:
        for agg in C.AGGREGATIONS:
            for mc in C.MIN_COUNTS:
                c = C.pointwise_case(shape, agg)
                if _separated(R.finalize(c['prob'], c['count'], agg, mc), R.finalize(c['prob'], c['count'], agg, mc, mutant), 0.0, True):
                    return shape, agg, mc
    return None


def _desc_separates(mutant):
    for case in DESC_CASES:
        r = R.sample_descriptors(case['desc'], case['H'], case['W'], case['kp'], case['count'])
        m = R.sample_descriptors(case['desc'], case['H'], case['W'], case['kp'], case['count'], mutant)
        usable = np.ones(r['want'].shape, bool)
        for b, k in case['low_norm_rows']:
            usable[b, k] = False
        if _separated(r['want'], m['want'], r['bound'], usable):
            return case['name']
    return None


SEPARATORS = {'warp': _warp_separates, 'filter': _filter_separates, 'accumulate': _accumulate_separates,
              'finalize': _finalize_separates, 'desc': _desc_separates}


@pytest.mark.parametrize('mutant', sorted(R.MUTANTS))
def test_every_mutant_is_told_apart(mutant):
    found = SEPARATORS[R.MUTANTS[mutant]](mutant)
    print('mutant %-28s separated by %s' % (mutant, found))
    assert found is not None, 'no committed case separates %s: a case is missing' % mutant


def test_mutant_list_is_complete():
    assert len(R.MUTANTS) >= 15 and set(R.MUTANTS.values()) == set(SEPARATORS)
