"""GPU (MI355X): the Fourier-Mellin registration kernels (csrc/register.hip) and their driver against the float64 restatement
(tests/registration_restatement.py) on the planted pairs of tests/registration_cases.py."""
import functools
import math

import numpy as np
import pytest
import torch

import registration_cases as C
import registration_restatement as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _reg():
    import multipoint_amd.utils.registration as G
    return G


def _fft2d(x):
    from multipoint_amd.models.classic_detectors import fft2d
    return fft2d(x)


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


# ---------------------------------------------------------------------------------------------------------------------
# 1. prepare
# ---------------------------------------------------------------------------------------------------------------------
SIMILARITIES = {
    'identity': None,
    'rot7_scale08': (0.8 * math.cos(math.radians(7.0)), 0.8 * math.sin(math.radians(7.0))),
    'rot180': (math.cos(math.pi), math.sin(math.pi)),
}


@pytest.mark.parametrize('sim', sorted(SIMILARITIES))
@pytest.mark.parametrize('H,W,N', [(8, 8, 8), (9, 13, 16), (30, 40, 48), (96, 128, 160)])
def test_prepare_matches_the_restatement(H, W, N, sim):
    rng = np.random.RandomState(H * 1000 + W)
    frames = rng.rand(2, H, W).astype(np.float32)
    cs = None if SIMILARITIES[sim] is None else np.array([SIMILARITIES[sim]] * 2, np.float32)
    border = []
    want = R.prepare(frames, N, cs, border)
    got = _reg().register_prepare(_dev(frames), N, None if cs is None else _dev(cs))
    assert got.shape == (2, N, N) and got.dtype == torch.complex64
    got = got.cpu().numpy()
    assert not got.imag.any()
    got = got.real.astype(np.float64)
    oy, ox = (N - H) // 2, (N - W) // 2
    outside = np.ones((N, N), bool)
    outside[oy:oy + H, ox:ox + W] = False
    for i in range(2):
        assert not got[i][outside].any()
        flipped = (got[i] == 0) != (want[i] == 0)
        print('%dx%d in %d %s frame %d: %d non-zero, %d zero tests flipped, largest difference %.3g' % (
            H, W, N, sim, i, np.count_nonzero(want[i]), flipped.sum(), np.abs(got[i] - want[i])[~flipped].max()))
        assert not (flipped & ~border[i]).any()
        assert flipped.sum() <= 0.005 * N * N
        assert np.abs(got[i] - want[i])[~flipped].max() <= 1e-6
    assert np.count_nonzero(want) > 0 or H == 8           # (8 x 8 under a similarity may leave no pixel whose taps all lie inside)
    if sim == 'identity':
        assert np.count_nonzero(want[0]) >= (H - 4) * (W - 4) - 2


# ---------------------------------------------------------------------------------------------------------------------
# 2. logpolar
# ---------------------------------------------------------------------------------------------------------------------
def _check_logpolar(spectrum, A, R_):
    got = _reg().register_logpolar(spectrum, A, R_).cpu().numpy()
    want = R.logpolar(spectrum.cpu().numpy(), A, R_)
    assert got.shape == want.shape and not got.imag.any()
    diff = np.abs(got.real.astype(np.float64) - want)
    tol = 4e-6 * np.maximum(1.0, np.abs(want))
    print('logpolar N %d A %d R %d: largest value %.3f, largest difference %.3g, largest difference / tolerance %.3f' % (
        spectrum.shape[-1], A, R_, np.abs(want).max(), diff.max(), (diff / tol).max()))
    assert (diff <= tol).all()
    assert np.abs(want).max() > 0.1


@pytest.mark.parametrize('N,A,R_', [(8, 8, 8), (48, 48, 48), (48, 12, 20), (160, 160, 160)])
def test_logpolar_of_random_spectra(N, A, R_):
    rng = np.random.RandomState(N + A)
    # magnitudes from 1e-3 to 1e3: log1p over its small-argument and its large-argument range
    mag = 10.0 ** rng.uniform(-3, 3, (2, N, N))
    ph = rng.uniform(0, 2 * np.pi, (2, N, N))
    _check_logpolar(_dev((mag * np.exp(1j * ph)).astype(np.complex64)), A, R_)


@pytest.mark.parametrize('N,H,W', [(8, 8, 8), (48, 30, 40), (160, 96, 128)])
def test_logpolar_of_prepared_frames(N, H, W):
    rng = np.random.RandomState(N)
    frames = _dev(rng.rand(2, H, W).astype(np.float32))
    A = _reg().fft_length_at_least(N)
    _check_logpolar(_fft2d(_reg().register_prepare(frames, N)), A, A)


# ---------------------------------------------------------------------------------------------------------------------
# 3. cross-power
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P,offsets,hw', [(1, [0, 1], (8, 8)), (5, [0, 1, 4, 5], (15, 20)), (5, [0, 2, 2, 5, 5], (9, 40)),
                                          (3, [0, 0, 3], (48, 48))])
def test_cross_power(P, offsets, hw):
    rng = np.random.RandomState(P * 10 + len(offsets))
    a = (rng.randn(P, *hw) + 1j * rng.randn(P, *hw)).astype(np.complex64)
    b = (rng.randn(P, *hw) + 1j * rng.randn(P, *hw)).astype(np.complex64)
    # bins made exactly zero: in a of one pair, in b of another, in every pair of a group
    a[0, 1, 2] = 0
    b[P - 1, 2, 1] = 0
    a[:, 3, 3] = 0
    want = R.cross_power(a, b, offsets)
    go = torch.tensor(offsets, dtype=torch.int32)
    got_t = _reg().register_cross_power(_dev(a), _dev(b), go)
    got = got_t.cpu().numpy()
    G = len(offsets) - 1
    assert got.shape == (G,) + hw
    for g in range(G):
        size = offsets[g + 1] - offsets[g]
        diff = np.abs(got[g].astype(np.complex128) - want[g]).max()
        print('cross-power P %d group %d of %d pairs: largest difference %.3g' % (P, g, size, diff))
        assert diff <= 1e-6 * max(size, 1)
        assert got[g, 0, 0] == 0 and got[g, 3, 3] == 0
        assert (got[g][want[g] == 0] == 0).all()
        if size == 0:
            assert not got[g].any()
    again = _reg().register_cross_power(_dev(a), _dev(b), go)
    assert torch.equal(torch.view_as_real(again), torch.view_as_real(got_t))
    if P >= 3:                # the pairs fed in two calls: the bits of one call
        cut = 2
        first = torch.tensor([min(o, cut) for o in offsets], dtype=torch.int32)
        rest = torch.tensor([max(o, cut) - cut for o in offsets], dtype=torch.int32)
        acc = _reg().register_cross_power(_dev(a[:cut]), _dev(b[:cut]), first)
        acc = _reg().register_cross_power(_dev(a[cut:]), _dev(b[cut:]), rest, out=acc)
        assert torch.equal(torch.view_as_real(acc), torch.view_as_real(got_t))


# ---------------------------------------------------------------------------------------------------------------------
# 4. peak
# ---------------------------------------------------------------------------------------------------------------------
KY, KX, DY, DX, TOP = 0.5, 0.25, 0.25, -0.375, 2.0       # the planted parabola: every sample exact in fp32


def _plant(plane, y, x):
    h, w = plane.shape
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            plane[(y + dy) % h, (x + dx) % w] = TOP - KY * (dy - DY) ** 2 - KX * (dx - DX) ** 2


def _positions(h, w):
    return [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h // 2, 0), (h - 1, w // 2), (h // 2, w - 1),
            (h // 2, w // 2), (min(h // 2 + 1, h - 1), min(w // 2 + 1, w - 1))]


def _check_peaks(planes, expect_index=None):
    """register_peak of float32 planes [G,h,w] against the restatement; returns the GPU result as numpy arrays."""
    pk = _reg().register_peak(_dev(planes))
    idx, off, sgn = pk.index.cpu().numpy(), pk.offset.cpu().numpy(), pk.signed.cpu().numpy()
    top, second = pk.peak.cpu().numpy(), pk.second.cpu().numpy()
    for g in range(planes.shape[0]):
        want = R.peak(planes[g])
        assert tuple(idx[g]) == want['index']
        if expect_index is not None:
            assert tuple(idx[g]) == tuple(expect_index[g])
        assert np.abs(off[g] - want['offset']).max() <= 1e-6 and np.abs(sgn[g] - want['signed']).max() <= 1e-5
        assert top[g] == np.float32(want['peak']) and second[g] == np.float32(want['second'])
    return idx, off, sgn, top, second


@pytest.mark.parametrize('h,w', [(3, 3), (8, 8), (15, 20), (160, 160)])
def test_peak_at_corners_and_edges(h, w):
    rng = np.random.RandomState(h * w)
    pos = _positions(h, w)
    planes = (rng.rand(len(pos), h, w) * 0.5).astype(np.float32)
    for g, (y, x) in enumerate(pos):
        _plant(planes[g], y, x)
    idx, off, sgn, top, second = _check_peaks(planes, pos)
    assert np.abs(off - [DY, DX]).max() <= 1e-6
    for g, (y, x) in enumerate(pos):
        assert sgn[g, 0] == pytest.approx((y - h if y > h // 2 else y) + DY, abs=1e-5)
        assert sgn[g, 1] == pytest.approx((x - w if x > w // 2 else x) + DX, abs=1e-5)
    assert (top == np.float32(TOP - KY * DY ** 2 - KX * DX ** 2)).all()
    if h == 3:
        assert np.isneginf(second).all()          # the wrapped 3 x 3 block is the whole plane
        return
    # the second-highest value just outside the block (two columns / rows away, wrapped), then just inside it
    for g, (y, x) in enumerate(pos):
        planes[g, y, (x + 2) % w] = 1.0
        planes[g, (y - 2) % h, (x - 1) % w] = 0.75
    assert (_check_peaks(planes, pos)[4] == 1.0).all()
    for g, (y, x) in enumerate(pos):
        planes[g, y, (x + 2) % w] = 0.25
        planes[g, (y - 2) % h, (x - 1) % w] = 0.25
        planes[g, (y + 1) % h, (x - 1) % w] = 1.9          # inside: not the second
    second = _check_peaks(planes, pos)[4]
    assert (second <= 0.5).all() and (second > 0.25).all()


def test_peak_ties_go_to_the_first_in_row_major_order():
    cases = []
    for h, w, spots in ((8, 8, [(2, 5), (2, 6), (5, 0)]), (15, 20, [(7, 19), (8, 0)]), (160, 160, [(10, 5), (150, 7)]),
                        (160, 160, [(103, 1), (102, 159)])):          # (160 x 160: the two in different chunks of the first stage)
        p = np.zeros((1, h, w), np.float32)
        for y, x in spots:
            p[0, y, x] = 1.0
        cases.append((p, min(spots)))
    for p, first in cases:
        idx, off, _, top, second = _check_peaks(p, [first])
        assert top[0] == 1.0 and second[0] in (0.0, 1.0)          # (1.0 where a tied value lies outside the block of the first)
    # a constant plane: every value ties, position (0, 0), flat parabola
    idx, off, sgn, top, second = _check_peaks(np.full((2, 8, 12), 0.5, np.float32), [(0, 0), (0, 0)])
    assert not off.any() and not sgn.any() and (second == 0.5).all()


def test_peak_signed_folding():
    for h, w in ((8, 8), (15, 20)):
        rows = [h // 2, h // 2 + 1]
        cols = [w // 2, w // 2 + 1]
        planes = np.zeros((4, h, w), np.float32)
        for g, (y, x) in enumerate([(rows[0], 1), (rows[1], 1), (1, cols[0]), (1, cols[1])]):
            planes[g, y, x] = 1.0
        idx, off, sgn, _, _ = _check_peaks(planes)
        assert not off.any()
        assert sgn[:, 0].tolist() == [h // 2, h // 2 + 1 - h, 1, 1] and sgn[:, 1].tolist() == [1, 1, w // 2, w // 2 + 1 - w]


def test_peak_second_stage_and_complex_planes():
    """1024 x 1024: 64 chunks per plane, so the second stage reduces more than one partial result per plane."""
    h = w = 1024
    rng = np.random.RandomState(7)
    planes = (rng.rand(3, h, w) * 0.5).astype(np.float32)
    pos = [(h - 1, w - 1), (517, 3), (0, 600)]
    for g, (y, x) in enumerate(pos):
        _plant(planes[g], y, x)
    planes[1, 900, 900] = planes[1, 517, 3]          # an exact tie in a later chunk: the earlier one stays the peak
    planes[2, 511, 1023] = 1.25                      # the second, in another chunk than the peak
    idx, off, sgn, top, second = _check_peaks(planes, pos)
    assert np.abs(off - [DY, DX]).max() <= 1e-6
    assert second[1] == top[1] and second[2] == 1.25
    # the real part of complex planes (stride 2) gives the same result
    z = torch.complex(_dev(planes[:2, :160, :160].copy()), torch.full((2, 160, 160), 9.0, device=DEV))
    a, b = _reg().register_peak(z), _reg().register_peak(_dev(planes[:2, :160, :160].copy()))
    for u, v in zip(a, b):
        assert torch.equal(u, v)


# ---------------------------------------------------------------------------------------------------------------------
# 5. end to end
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(name):
    o, t, T = C.case(name)
    return R.estimate(o[None], t[None]), T


@functools.lru_cache(maxsize=None)
def _gpu(name):
    o, t, _ = C.case(name)
    G = _reg()
    est = G.FourierEstimator(o.shape, t.shape, 1)
    est.add_stage1(_dev(o[None]), _dev(t[None]))
    est.finish_stage1()
    est.add_stage2(_dev(o[None]), _dev(t[None]))
    T, rep = est.finish()
    return est, T, rep


@pytest.mark.parametrize('name', sorted(C.CASES))
def test_end_to_end_against_restatement_and_truth(name):
    ref, T_true = _reference(name)
    est, T, rep = _gpu(name)
    b = int(rep.branch[0])
    assert tuple(est.pk1.index[0].tolist()) == ref['pk1'][0]['index']
    assert b == ref['branch'][0]
    assert tuple(est.pk2[b].index[0].tolist()) == ref['pk2'][0]['index']
    err, diff = C.corner_error(T[0], T_true), C.corner_error(T[0], ref['T'][0])
    print('%s: corner error against the planted transform %.4f px (restatement %.4f px), GPU against restatement %.5f px; '
          'ratios %.3f %.3f (restatement %.3f %.3f)' % (
              name, err, C.corner_error(ref['T'][0], T_true), diff, rep.peak1[0] / rep.second1[0], rep.peak2[0] / rep.second2[0],
              ref['pk1'][0]['peak'] / ref['pk1'][0]['second'], ref['pk2'][0]['peak'] / ref['pk2'][0]['second']))
    assert err <= 1.5
    # the report is the decomposition of the transform, and the one-call form gives the same model
    import multipoint_amd.utils as U
    assert (rep.angle[0], rep.scale[0], rep.dx[0], rep.dy[0]) == U.decompose_similarity(T[0])
    o, t, _ = C.case(name)
    T2, rep2 = U.estimate_similarity_fourier(_dev(o[None]), _dev(t[None]))
    assert np.array_equal(T2, T) and rep2.peak2[0] == rep.peak2[0]


def test_phase_correlation_finds_a_cyclic_shift():
    rng = np.random.RandomState(3)
    a = rng.rand(2, 48, 60).astype(np.float32)
    b = np.stack([np.roll(a[0], (-5, 7), (0, 1)), np.roll(a[1], (11, -20), (0, 1))])          # a(x) = b(x - p): p = (5, -7), (-11, 20)
    pk = _reg().phase_correlation(torch.complex(_dev(a), torch.zeros_like(_dev(a))), torch.complex(_dev(b), torch.zeros_like(_dev(b))),
                                  torch.tensor([0, 1, 2], dtype=torch.int32))
    assert pk.index.tolist() == [[5, 60 - 7], [48 - 11, 20]]
    assert np.abs(pk.signed.cpu().numpy() - [[5, -7], [-11, 20]]).max() <= 1e-3 and (pk.peak > 0.99).all()


# ---------------------------------------------------------------------------------------------------------------------
# 6. pooling
# ---------------------------------------------------------------------------------------------------------------------
def test_pooled_surface_is_the_sum_of_the_single_pair_surfaces():
    G = _reg()
    o, t, T_true = C.group_case()
    od, td = _dev(o), _dev(t)
    pooled = G.FourierEstimator(o.shape[1:], t.shape[1:], 1)
    pooled.add_stage1(od, td)
    cs = pooled.finish_stage1()
    single = G.FourierEstimator(o.shape[1:], t.shape[1:], 4)
    single.add_stage1(od, td, np.arange(4))
    single.finish_stage1()
    d1 = (pooled.surface1[0] - single.surface1.sum(0)).abs().max().item()
    # stage 2 under ONE similarity for all four pairs (each single-pair estimate would prepare under its own)
    N = pooled.N
    fo = _fft2d(G.register_prepare(od, N))
    ft = _fft2d(G.register_prepare(td, N, _dev(np.repeat(cs, 4, 0))))
    s_pool = G.register_cross_power(fo, ft, torch.tensor([0, 4], dtype=torch.int32))
    s_single = G.register_cross_power(fo, ft, torch.arange(5, dtype=torch.int32))
    from multipoint_amd.models.classic_detectors import fft2d
    a = fft2d(s_pool, inverse=True) / (N * N)
    b = fft2d(s_single, inverse=True).sum(0, keepdim=True) / (N * N)
    d2 = (a - b).abs().max().item()
    print('pooled against summed surfaces: stage 1 %.3g, stage 2 %.3g' % (d1, d2))
    assert d1 <= 4e-6 and d2 <= 4e-6
    pooled.add_stage2(od, td)
    T, rep = pooled.finish()
    ref = R.estimate(o, t, [0, 4])
    assert tuple(pooled.pk1.index[0].tolist()) == ref['pk1'][0]['index'] and int(rep.branch[0]) == ref['branch'][0]
    assert C.corner_error(T[0], T_true) <= 1.5


def test_groups_are_indexed_and_chunks_accumulate_to_the_same_bits():
    import multipoint_amd.utils as U
    G = _reg()
    o, t, gid, T_true = C.shift_groups_case()
    od, td = _dev(o), _dev(t)
    ref = R.estimate(o, t, np.searchsorted(gid, np.arange(4)))
    T, rep = U.estimate_similarity_fourier(od, td, groups=gid)
    assert T.shape == (3, 3, 3)
    whole = G.FourierEstimator(o.shape[1:], t.shape[1:], 3)
    whole.add_stage1(od, td, gid)
    whole.finish_stage1()
    whole.add_stage2(od, td, gid)
    Tw, _ = whole.finish()
    assert np.array_equal(Tw, T)
    for g in range(3):
        b = int(rep.branch[g])
        assert tuple(whole.pk1.index[g].tolist()) == ref['pk1'][g]['index'] and b == ref['branch'][g]
        assert tuple(whole.pk2[b].index[g].tolist()) == ref['pk2'][g]['index']
        err, diff = C.corner_error(T[g], T_true[g]), C.corner_error(T[g], ref['T'][g])
        print('group %d: corner error %.4f px, GPU against restatement %.5f px' % (g, err, diff))
        assert err <= 1.5 and diff <= 0.5          # (0.5 px: the room the 1.5 px bound leaves above the fixtures' 1.0 px)
    # the same batch in two chunks (the cut inside group 2) through the accumulating path
    parts = G.FourierEstimator(o.shape[1:], t.shape[1:], 3)
    for sl in (slice(0, 4), slice(4, 6)):
        parts.add_stage1(od[sl], td[sl], gid[sl])
    parts.finish_stage1()
    assert torch.equal(torch.view_as_real(parts.x1), torch.view_as_real(whole.x1))
    for sl in (slice(0, 4), slice(4, 6)):
        parts.add_stage2(od[sl], td[sl], gid[sl])
    Tp, repp = parts.finish()
    for b in range(2):
        assert torch.equal(torch.view_as_real(parts.x2[b]), torch.view_as_real(whole.x2[b]))
    assert np.array_equal(Tp, T) and np.array_equal(repp.peak2, rep.peak2)
    # the float64 host composition: the documented formula
    assert np.allclose(T[0], R.compose((1.0, -1.0)[int(rep.branch[0])] * whole.cs[0].astype(np.float64),
                                         whole.pk2[int(rep.branch[0])].signed[0].double().cpu().numpy(), o.shape[1:], t.shape[1:], whole.N),
                       rtol=0, atol=1e-12)
