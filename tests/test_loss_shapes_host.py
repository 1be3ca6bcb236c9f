"""CPU: the premises of the inputs tests/loss_shape_cases.py builds for tests/test_gpu_loss_shapes.py, on the float64
restatements alone: the cell counts lie on every tile edge, every sum the descriptor kernels form on the exact cases is exact
in fp32 (so the GPU tests may ask for float64's bits), the fixtures hold the ties, boundaries and clamps they are chosen for,
and a dropped or doubled cell moves a detector sum far beyond the tolerance."""
import numpy as np
import pytest

import loss_grad_restatement as RG
import loss_restatement as R
import loss_shape_cases as C

EXACT = 2.0 ** 24          # integers below it are exact in fp32, and so is every sum of them that stays below it
ALL_EXACT = ([('grid', n) for n in C.descriptor_names()] + [('stale', i) for i in range(len(C.STALE_CASES))] +
             [('threshold', i) for i in range(len(C.THRESHOLD_CASES))])


def _case(kind, key):
    return {'grid': C.descriptor_case, 'stale': C.stale_case, 'threshold': C.threshold_case, 'random': C.random_case}[kind](key)


def test_cell_counts_lie_on_every_tile_edge():
    """the coverage claim, not the list: for every granularity one N below, at and above a multiple; N = 1, a row, a column"""
    Ns = [h * w for h, w in C.GRIDS]
    for g in C.GRANULES:
        for r in (g - 1, 0, 1):
            assert any(n % g == r and n >= g - 1 for n in Ns), (g, r)
    assert (1, 1) in C.GRIDS
    assert any(w == 1 and h > 256 for h, w in C.GRIDS) and any(h == 1 and w > 256 for h, w in C.GRIDS)
    assert max(Ns) == 4 * 128 + 1 == 2 * 256 + 1                  # 4 x 4 forward tiles plus a cell, two per-cell workgroups plus one
    assert len(set(C.GRIDS)) == len(C.GRIDS)
    # every descriptor case is one of these grids at one of the three sizes, with images that differ
    assert len(C.descriptor_names()) == 3 * len(C.GRIDS)
    for name in C.descriptor_names():
        c = C.descriptor_case(name)
        assert c['D'] in C.DIMS and c['grid'] in C.GRIDS and c['B'] in (2, 3)
        assert c['B'] * c['N'] ** 2 * c['D'] <= 2.1e8
        for s in (1, 2):
            d = c['inputs']['desc%d' % s]
            assert d.shape == (c['B'], c['D']) + c['grid'] and d.dtype == np.float32
            assert c['N'] * c['D'] < 200 or not np.array_equal(d[0], d[1])


def test_layouts_and_homographies_meet_every_size_and_tile_class():
    seen = {(C.descriptor_case(n)['layout'], C.descriptor_case(n)['D']) for n in C.descriptor_names()}
    assert seen == {(l, D) for l in C.LAYOUTS for D in C.DIMS}
    seen = {(C.descriptor_case(n)['hom'], C.descriptor_case(n)['D']) for n in C.descriptor_names()}
    assert seen == {(h, D) for h in C.HOMS for D in C.DIMS}
    for layout in C.LAYOUTS:                                      # each layout on several forward tiles and on a single one
        Ns = [C.descriptor_case(n)['N'] for n in C.descriptor_names() if C.descriptor_case(n)['layout'] == layout]
        assert any(n > 256 for n in Ns) and any(n <= 128 for n in Ns), layout
    assert {C.random_case(n)['D'] for n in C.random_names()} == set(C.DIMS)
    assert {C.random_case(n)['N'] for n in C.random_names()} == {33, 129, 513}
    for n in C.random_names():                                    # corresponding and other valid pairs in every image
        c = C.random_case(n)
        assert c['layout'] in ('all_valid', 'tile_edges') and len(set(c['norms'].tolist())) == 1
        w = [R.warp_centres(c['inputs']['homography%d' % s], c['B'], *c['grid']).astype(np.float32) for s in (1, 2)]
        sums = C.descriptor_answers(c, w[0], w[1], gradients=False)['sums']
        assert sums[:, 2].min() >= 3 and sums[:, :2].min() > 0, (n, sums.tolist())
    assert {(c[0][0] * c[0][1], c[1]) for c in C.STALE_CASES} == {(1, 64), (129, 128), (257, 64), (33, 256)}


def test_mask_layouts():
    for N in (1, 33, 129, 513):
        e = C.tile_edge_cells(N)
        want = {0, N - 1} | {i for m in range(32, N, 32) for i in (m - 1, m, m + 1) if i < N}
        assert set(e.tolist()) == want and e.max() == N - 1
        a = C.last_tile_cells(N)
        assert a[0] % 128 == 0 and a[-1] == N - 1 and 1 <= len(a) <= 128
    for name in C.descriptor_names():
        c = C.descriptor_case(name)
        v1, v2 = C.cell_valid(c)                                  # what the restatement reads from the pixel maps
        B, N = c['B'], c['N']
        assert np.array_equal(v1.reshape(B, N), c['valid'][0]) and np.array_equal(v2.reshape(B, N), c['valid'][1])
        for s in (1, 2):                                          # an invalid cell is invalid by a single pixel
            m = R.space_to_depth(c['inputs']['valid_mask%d' % s][:, 0])
            assert np.all((~m).sum(1) == ~c['valid'][s - 1].reshape((B,) + c['grid']))
        norms = c['valid'][0].sum(1) * c['valid'][1].sum(1)
        if c['layout'] == 'all_valid':
            assert v1.all() and v2.all()
        elif c['layout'] == 'tile_edges':
            assert all(set(np.flatnonzero(v[b]).tolist()) == set(C.tile_edge_cells(N).tolist())
                       for b in range(B) for v in (c['valid'][b % 2],))
        elif c['layout'] == 'last_tile':
            assert all(np.flatnonzero(v[b]).min() >= 128 * ((N - 1) // 128) for b in range(B) for v in c['valid'])
        elif c['layout'] == 'empty_side':
            assert B == 3 and not c['valid'][1][1].any() and c['valid'][0][1].any() and norms[1] == 0
            assert norms[0] == norms[2] > 0
        else:
            assert not c['config']['descriptor_loss_use_mask'] and (N == 1 or not (v1.all() and v2.all()))
        if c['config']['descriptor_loss_use_mask'] and c['layout'] != 'empty_side':
            assert len(set(norms.tolist())) == 1 and norms[0] == c['norm'] > 0      # one norm per case


@pytest.mark.parametrize('kind,key', ALL_EXACT, ids=lambda v: str(v))
def test_exact_inputs_and_centres(kind, key):
    """descriptors on the quarter grid with |k| <= 3, exact margins, a power-of-two lambda_d, 0 / 1 weights, and warped centres
    that are integers: the reference needs no kernel output and float32 holds it exactly"""
    c = _case(kind, key)
    for s in (1, 2):
        k = c['inputs']['desc%d' % s].astype(np.float64) * 4
        assert np.array_equal(k, np.round(k)) and np.abs(k).max() <= 3
        assert c['inputs']['valid_mask%d' % s].dtype == bool
    cfg = c['config']
    assert (cfg['positive_margin'], cfg['negative_margin']) == (1.0, 0.25)
    assert (cfg['positive_margin'] * 16) % 1 == 0 and (cfg['negative_margin'] * 16) % 1 == 0      # on the dot lattice
    assert np.log2(cfg['lambda_d']) % 1 == 0
    Hc, Wc = c['grid']
    centres = R.cell_centres(Hc, Wc)
    for s, w in zip((1, 2), C.exact_centres(c)):
        hom = c['inputs'].get('homography%d' % s)
        assert np.array_equal(w, np.round(w)) and np.array_equal(w.astype(np.float32).astype(np.float64), w)
        for b in range(c['B']):
            t = np.zeros(2) if hom is None else hom[b, 1::-1, 2].astype(np.float64)             # (ty, tx)
            assert hom is None or (np.array_equal(hom[b, :, :2], np.eye(3)[:, :2]) and np.all(t % 4 == 0))
            assert np.array_equal(w[b], centres - t)


def test_one_side_without_homography_and_a_translation_on_the_other():
    cases = [C.descriptor_case(n) for n in C.descriptor_names() if C.descriptor_case(n)['hom'] == 'none_translation']
    assert cases
    for c in cases:
        assert 'homography1' not in c['inputs'] and np.abs(c['inputs']['homography2'][:, :2, 2]).max() > 0


@pytest.mark.parametrize('kind,key', ALL_EXACT + [('random', n) for n in C.random_names()], ids=lambda v: str(v))
def test_forward_sums_are_exact_in_fp32(kind, key):
    """Every dot is a multiple of 1/16 below 2^24 / 16; for every image and every 128 x 128 tile the sum of |term| in units
    of 1/16 stays below 2^24 for the positive and the negative terms: every partial sum, in any order and with or without
    FMA, is exact.  (Random homographies change which pairs correspond, not this: the bound is taken over both roles.)"""
    c = _case(kind, key)
    thresholds = C.THRESHOLDS if kind == 'threshold' else [c['config']['descriptor_loss_threshold']]
    if kind == 'random':
        w1 = w2 = np.zeros((c['B'], c['N'], 2), np.float32)
        thresholds = [float('inf'), -1.0]                          # every pair positive, every pair negative
    else:
        w1, w2 = C.exact_centres(c)
    for t in thresholds:
        dot, corr, w, pos, neg = C.pair_terms(c, w1, w2, {'descriptor_loss_threshold': t})
        assert np.array_equal(dot * 16, np.round(dot * 16)) and np.abs(dot).max() <= 9 * c['D'] / 16 <= 144
        for x in (pos, neg):
            assert np.array_equal(x * 16, np.round(x * 16))
            assert C.tile_sums(x).max() * 16 < EXACT, (t, C.tile_sums(x).max() * 16)
        assert set(np.unique(w.astype(np.float64)).tolist()) <= {0.0, 1.0}


@pytest.mark.parametrize('name', C.descriptor_names())
def test_exact_cases_hold_pairs_of_both_kinds_and_ties(name):
    c = C.descriptor_case(name)
    ref = C.descriptor_reference(name)
    w1, w2 = C.exact_centres(c)
    dot, corr, w, pos, neg = C.pair_terms(c, w1, w2)
    live = [b for b in range(c['B']) if c['norms'][b] > 0]
    assert np.array_equal(ref['sums'][:, 2], (corr & w).sum((1, 2)))
    assert np.array_equal(ref['sums'][:, 3], c['norms'].astype(np.float64))
    for b in live:
        assert (corr[b] & w[b]).any(), 'no corresponding valid pair'
        if w[b].sum() >= 900:
            assert ref['sums'][b, 0] > 0 and ref['sums'][b, 1] > 0 and (~corr[b] & w[b]).any()
    # a handful of valid pairs (N = 1, one cell in the last tile): a live hinge in some image
    assert any(ref['sums'][b, 0] + ref['sums'][b, 1] > 0 for b in live)
    if c['N'] >= 127 and c['layout'] in ('all_valid', 'mask_unused'):
        # exact hinge ties (their half weight is the gradient's, RG.hinge) among the counted pairs
        assert (w & ~corr & (dot == c['config']['negative_margin'])).sum() > 20
    if c['layout'] == 'empty_side':
        assert np.array_equal(ref['sums'][1], np.zeros(4))
        assert np.isnan(ref['g1'][1]).all() and np.isnan(ref['g2'][1]).all()
    for b in live:
        assert np.isfinite(ref['g1'][b]).all() and np.isfinite(ref['g2'][b]).all()
        assert w[b].sum() < 900 or (np.abs(ref['g1'][b]).max() > 0 and np.abs(ref['g2'][b]).max() > 0)
    assert any(np.abs(ref['g1'][b]).max() > 0 and np.abs(ref['g2'][b]).max() > 0 for b in live)


def test_positive_margin_ties_exist():
    """pairs whose dot equals a margin exactly, on a full tile at D = 64: about 1 % of the pairs each"""
    c = C.descriptor_case('8x16-64')
    dot = C.pair_terms(c, *C.exact_centres(c))[0]
    assert (dot == 1.0).sum() > 100 and (dot == 0.25).sum() > 100


@pytest.mark.parametrize('kind,key', ALL_EXACT + [('random', n) for n in C.random_names()], ids=lambda v: str(v))
def test_gradient_sums_are_exact_in_fp32(kind, key):
    """ka and kb, evaluated as the kernel does (double, rounded to float once), are the powers of two KA and KB; G takes the
    values {1, 1/2} x {ka, kb} and X lies on the quarter grid, so every product is a multiple of min(|ka|, |kb|) / 8, and per
    own cell and channel the sum of |G X| in that unit is at most N x max|G| x max|X| / unit < 2^24."""
    c = _case(kind, key)
    ka, kb = C.kernel_coefficients(c)
    assert (float(ka), float(kb)) == (C.KA, C.KB)
    assert all(np.log2(abs(k)) % 1 == 0 for k in (C.KA, C.KB))
    assert np.array_equal(C.upstream(c), [0.0, 0.0, c['alpha'], c['beta']]) and c['alpha'] != c['beta']
    unit = min(abs(C.KA), abs(C.KB)) / 8
    xmax = max(np.abs(c['inputs']['desc%d' % s]).max() for s in (1, 2))
    assert c['N'] * max(abs(C.KA), abs(C.KB)) * xmax / unit < EXACT
    for b in range(c['B']):                                       # an image with norm 0 has NaN coefficients, as the reference
        if c['norms'][b] == 0:
            with np.errstate(divide='ignore', invalid='ignore'):
                assert not np.isfinite(np.float32(c['beta'] * (np.float64(1.0) / (c['B'] * 0.0))))
        else:
            assert c['norms'][b] == c['norm']


def test_shuffled_fp32_accumulation_equals_float64():
    """the largest case, N = 513 at D = 256: an fp32 accumulation of the gradient's terms in a shuffled order gives the float64
    sum bit for bit (one image, 64 own cells, all channels)"""
    name = '19x27-256'
    c, ref = C.descriptor_case(name), C.descriptor_reference(name)
    assert c['N'] == 513 and c['D'] == 256
    w1, w2 = C.exact_centres(c)
    dot, corr, w, _, _ = C.pair_terms(c, w1, w2)
    cc = (corr & w).astype(np.float64)
    G = (C.KA * cc * RG.hinge(1.0 - dot) + C.KB * (w - cc) * RG.hinge(dot - 0.25))[0]          # [i side 2][j side 1]
    X2 = c['inputs']['desc2'][0].reshape(256, 513).T                                           # [i][d]
    order = np.random.RandomState(0).permutation(513)
    acc = np.zeros((64, 256), np.float32)
    for i in order:
        acc = acc + G[i, :64, None].astype(np.float32) * X2[i][None, :]
    got = acc.T.reshape(256, 64)
    assert np.array_equal(got.astype(np.float64), ref['g1'][0].reshape(256, 513)[:, :64])


@pytest.mark.parametrize('i', range(len(C.THRESHOLD_CASES)))
def test_threshold_cases_separate_the_thresholds(i):
    """Valid pairs at squared distance 0 or 64 and at 128 exist, sqrt(128) is not a float32 (so the bound on the squared
    distance cannot be thr * thr rounded), and the six thresholds give the counts their definition gives."""
    c = C.threshold_case(i)
    assert c['N'] in (33, 129, 257)
    w1, w2 = C.exact_centres(c)
    d = w1[:, None, :, :] - w2[:, :, None, :]
    s = (d * d).sum(-1)
    w = C.pair_terms(c, w1, w2)[2]
    n = {v: int(((s == v) & w).sum()) for v in (0.0, 64.0, 128.0)}
    assert n[64.0] > 0 and n[128.0] > 0
    t = np.float32(C.THRESHOLDS[4])
    assert float(t) ** 2 != 128.0 and t == np.sqrt(np.float32(128)) and np.float32(C.THRESHOLDS[5]) < t
    counts = [C.threshold_reference(i, k)[:, 2].sum() for k in range(len(C.THRESHOLDS))]
    below = int(((s < 128.0) & w).sum())
    assert counts == [n[0.0], 0, w.sum(), int(((s <= 64.0) & w).sum()), below + n[128.0], below]
    # nothing lies between 64 and 128 on the cell lattice: 8.0 and the float below sqrt(128) agree, the others differ
    assert counts[1] < counts[3] == counts[5] < counts[4] < counts[2] and (n[0.0] == 0 or n[0.0] < counts[3])


# ---- detector ----
def test_detector_cases_cover_the_grids_and_modes():
    names = C.detector_names()
    assert len(names) == 3 * (len(C.GRIDS) + 1)
    for g in C.GRIDS + ['sweep']:
        for mode in C.DETECTOR_MODES:                             # CE with host and with device noise, and BCE, on every grid
            assert ('%dx%d-%s' % (g + (mode,)) if g != 'sweep' else 'sweep-%s' % mode) in names
    for name in names:
        c = C.detector_case(name)
        lg = c['inputs']['logits1']
        assert lg.shape == (c['B'], 65) + c['grid'] and np.array_equal(lg * 8, np.round(lg * 8))
        assert (c['noise'][0] is None) == (c['mode'] == 'bce')
        if c['mode'] != 'bce':
            assert c['noise'][0].shape == (c['B'], 64) + c['grid'] and not np.array_equal(c['noise'][0], c['noise'][1])


def test_device_noise_decides_labels_on_single_rows_and_columns():
    """cells with several keypoints whose label follows the hash: a wrong index (b, c, h, w) or n / Wc decode changes labels"""
    for g in ('1x257', '257x1', '1x31', '97x1'):
        c = C.detector_case(g + '-ce_device')
        kp = c['inputs']['keypoints1']
        lab = R.detector_labels(kp, c['noise'][0])
        assert (R.space_to_depth(kp).sum(1) > 1).sum() >= c['grid'][0] * c['grid'][1] // 4
        other = R.detector_labels(kp, np.roll(c['noise'][0], 1, axis=-1 if c['grid'][0] == 1 else -2))
        assert (lab != other).sum() > 2


def test_pixel_position_sweep():
    for mode in C.DETECTOR_MODES:
        c = C.detector_case('sweep-' + mode)
        inp = c['inputs']
        assert c['grid'] == (8, 8) and c['B'] == 3
        kp = R.space_to_depth(inp['keypoints1'])
        for k in range(64):                                       # cell k: one keypoint, at pixel position k = channel k
            assert np.flatnonzero(kp[0, :, k // 8, k % 8]).tolist() == [k]
            assert np.flatnonzero(~R.space_to_depth(inp['valid_mask1'][:, 0])[1, :, k // 8, k % 8]).tolist() == [k]
        assert kp[2, :, 0, 5].all()                               # all 64 keypoints in one cell
        ref = C.detector_reference('sweep-' + mode)
        assert ref['count1'].tolist() == [64.0, 0.0, 64.0 - 22.0] and ref['sum1'][1] == 0.0
        assert np.isnan(ref['grad1'][1]).all() and np.isfinite(ref['grad1'][[0, 2]]).all()
        valid = R.cell_valid(inp['valid_mask1'], 3, 64, 64)
        g = ref['grad1']
        assert np.all((np.abs(g[2]).max(0) > 0) == valid[2])      # the gradient shows each cell's validity ...
        if c['use_ce']:                                           # ... and its label: the one negative entry is channel k
            assert np.array_equal(g[0].argmin(0), np.arange(64).reshape(8, 8)) and (g[0] < 0).sum() == 64


def test_bce_clamp_cells():
    """the top logit is >= 128 above every other, the other gaps stay <= 10; p is exactly 1 and 0 in float32, so both log
    clamps at -100 and the backward's 1e-12 clamp act, and the cell's loss is 200"""
    for g in C.GRIDS:
        c = C.detector_case('%dx%d-bce' % g)
        N = g[0] * g[1]
        for s in (1, 2):
            lg = c['inputs']['logits%d' % s].reshape(c['B'], 65, N)
            srt = np.sort(lg, 1)
            gap, rest = srt[:, -1] - srt[:, -2], srt[:, -2] - srt[:, 0]
            clamp = np.zeros((c['B'], N), bool)
            clamp[0, C.clamp_cells(N)] = True
            assert np.all(gap[clamp] >= C.CLAMP_GAP) and np.all(rest <= 10) and np.all(gap[~clamp] <= 10)
            p = np.exp(lg - lg.max(1, keepdims=True), dtype=np.float32)
            p = p / p.sum(1, keepdims=True, dtype=np.float32)
            kp = R.space_to_depth(c['inputs']['keypoints%d' % s]).reshape(c['B'], 64, N)
            for n in C.clamp_cells(N):
                top = lg[0, :, n].argmax()
                assert p[0, top, n] == 1.0 and np.delete(p[0, :, n], top).max() == 0.0
                assert kp[0, :, n].sum() == 1 and (top == 64 or not kp[0, top, n])
            loss, valid = C.cell_losses(c, s)
            assert valid[0, C.clamp_cells(N)].all() and np.allclose(loss[0, C.clamp_cells(N)], 200.0, rtol=1e-12)
    for g in C.GRIDS:                                             # every other logit everywhere lies in [-5, 5]
        for mode in ('ce_host', 'ce_device'):
            assert np.abs(C.detector_case('%dx%d-%s' % (g + (mode,)))['inputs']['logits2']).max() <= 5


def test_detector_tolerance_and_what_a_cell_weighs():
    """The tolerance is computed, not a constant: 4 x the float32 restatement's own relative error or 8 fp32 ulps, whichever
    is larger, of the largest reference value.  Dropping or doubling any single valid cell moves its image's sum by more than
    10 x the tolerance."""
    floor = C.detector_floor()
    print('float32 floor (relative): sum %.3g, grad %.3g; 8 ulps = %.3g' % (floor['sum'], floor['grad'], 8 * C.EPS32))
    assert 0 < floor['sum'] < 1e-5 and 0 < floor['grad'] < 1e-4
    for name in C.detector_names():
        c, ref = C.detector_case(name), C.detector_reference(name)
        for s in (1, 2):
            tol = C.detector_tolerance('sum', ref['sum%d' % s])
            assert tol == max(4 * floor['sum'], 8 * C.EPS32) * np.abs(ref['sum%d' % s]).max()
            loss, valid = C.cell_losses(c, s)
            assert np.array_equal(valid.sum(1), ref['count%d' % s])
            assert np.allclose(np.where(valid, loss, 0).sum(1), ref['sum%d' % s], rtol=1e-12, atol=0)
            assert np.all(loss[valid] > 10 * tol), (name, s, loss[valid].min(), tol)
            live = ref['count%d' % s] > 0
            assert np.all(ref['sum%d' % s][live] > 0) and (live.all() or name.startswith('sweep'))


def test_restatement_defaults_are_float64_and_float32_mode_differs():
    c = C.detector_case('7x9-bce')
    inp = c['inputs']
    args = (inp['logits1'], inp['keypoints1'], inp['valid_mask1'], False)
    a, b = R.detector_loss_sums(*args), R.detector_loss_sums(*args, dtype=np.float64)
    f = R.detector_loss_sums(*args, dtype=np.float32)
    assert a[0].dtype == np.float64 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], f[1])
    assert not np.array_equal(a[0], f[0]) and np.allclose(a[0], f[0], rtol=1e-5)
    ga, gf = RG.detector_grad(*args, 1.0), RG.detector_grad(*args, 1.0, dtype=np.float32)
    assert ga.dtype == gf.dtype == np.float64 and not np.array_equal(ga, gf) and np.allclose(ga, gf, atol=1e-6)
