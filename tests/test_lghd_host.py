"""CPU: the numpy restatement of the LGHD baseline (tests/lghd_restatement.py) against what the reference's own LGHD returned
(tests/golden/lghd.npz, written by tests/golden/make_golden_lghd.py), FAST on hand-made patterns, and the condition the
orientation-map tolerance of tests/test_gpu_lghd.py rests on, checked on the reference side alone."""
import os

import numpy as np
import pytest

import lghd_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lghd.npz')


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def test_filter_bank_is_the_references(golden):
    want = golden['bank_48x80']
    got = R.filter_bank(48, 80)
    assert got.shape == want.shape == (24, 48, 80)
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()         # the fixture stores fp32
    from multipoint_amd.models.classic_detectors import log_gabor_bank
    assert np.array_equal(log_gabor_bank(48, 80), got)


@pytest.mark.parametrize('name,kind,seed,H,W', R.IMAGES)
def test_restatement_matches_the_reference(golden, name, kind, seed, H, W):
    assert name in list(golden['names'])
    u8 = R.quantize(R.make_image(kind, seed, H, W))
    kp, desc, _ = R.detect_and_compute(u8)
    assert np.array_equal(kp, golden['kp_' + name].astype(np.int64))
    assert np.array_equal(desc, golden['desc_' + name].astype(np.float64))
    assert np.array_equal(kp, golden['prob_kp_' + name].astype(np.int64))
    assert len(kp) >= 13
    assert np.all(desc.reshape(len(kp), 4, 16, 6).sum(-1) == 100)          # every 10 x 10 cell counts 100 pixels per scale


def test_quantisation_truncates_the_fp32_product():
    k = np.arange(256)
    img = (k / 255.0).astype(np.float32)
    u8 = R.quantize(img)
    assert np.array_equal(u8, (img * 255.0).astype(np.uint8))
    assert np.all((u8 == k) | (u8 == k - 1))           # k / 255 as fp32, times 255, may land below k (with numpy's fp32 it does not)
    x = np.random.default_rng(0).random(4096).astype(np.float32)
    assert np.array_equal(R.quantize(x), (x * np.float32(255.0)).astype(np.int32).astype(np.uint8))


def _pattern(p, ring, H=9, W=9, at=(4, 4)):
    """a frame of value p with the 16 circle pixels around `at` set to ring[i]"""
    im = np.full((H, W), p, np.uint8)
    for (dx, dy), v in zip(R.CIRCLE, ring):
        im[at[0] + dy, at[1] + dx] = v
    return im


def test_fast_arc_of_nine_and_of_eight():
    nine = [200] * 9 + [100] * 7
    assert R.fast_scores(_pattern(100, nine))[4, 4] == 99
    eight = [200] * 8 + [100] * 8
    assert R.fast_scores(_pattern(100, eight))[4, 4] == 0
    dark = [10] * 9 + [100] * 7
    assert R.fast_scores(_pattern(100, dark))[4, 4] == 89


def test_fast_arc_wraps():
    ring = [100] * 16
    for i in (12, 13, 14, 15, 0, 1, 2, 3, 4):
        ring[i] = 150
    assert R.fast_scores(_pattern(100, ring))[4, 4] == 49
    ring[0] = 100                       # broken at the wrap: 4 + 4
    assert R.fast_scores(_pattern(100, ring))[4, 4] == 0


def test_fast_difference_of_exactly_ten_is_no_corner():
    assert R.fast_scores(_pattern(100, [110] * 9 + [100] * 7))[4, 4] == 0
    assert R.fast_scores(_pattern(100, [111] * 9 + [100] * 7))[4, 4] == 10
    assert R.fast_scores(_pattern(100, [90] * 9 + [100] * 7))[4, 4] == 0
    assert R.fast_scores(_pattern(100, [89] * 9 + [100] * 7))[4, 4] == 10


def test_fast_equal_neighbours_drop_each_other():
    s = np.zeros((9, 12), np.int32)
    s[4, 4] = s[4, 5] = 30
    s[4, 9] = 30
    s[6, 2] = 12; s[7, 3] = 11
    keep = R.fast_corners(s)
    assert not keep[4, 4] and not keep[4, 5]
    assert keep[4, 9] and keep[6, 2] and not keep[7, 3]
    assert keep.sum() == 2


def test_fast_corners_at_the_first_and_last_tested_rows():
    H, W = 12, 11
    ring = [200] * 9 + [100] * 7
    for y in (3, H - 4):
        im = _pattern(100, ring, H, W, at=(y, 5))
        sc = R.fast_scores(im)
        assert sc[y, 5] == 99
        assert [tuple(p) for p in R.fast_keypoints(im) if p[0] == y] == [(y, 5)]
    # rows 2 and H - 3 are never tested, whatever surrounds them
    noise = np.random.default_rng(0).integers(0, 256, (H, W)).astype(np.uint8)
    sc = R.fast_scores(noise)
    assert not sc[:3].any() and not sc[H - 3:].any() and not sc[:, :3].any() and not sc[:, W - 3:].any()


def test_validity_rule():
    kp = np.array([[19, 30], [20, 20], [28, 60], [29, 30], [28, 61]])
    assert np.array_equal(R.valid_keypoints(kp, 48, 80), kp[1:3])


@pytest.mark.parametrize('name,kind,seed,H,W', R.IMAGES)
def test_few_pixels_are_ambiguous_in_float64(name, kind, seed, H, W):
    """The condition of the GPU orientation test, on the reference side alone: with err32 the error of a float32 np.fft against
    the float64 one on this image's 24 responses, at most 1 % of a scale's pixels have their two largest float64 magnitudes within
    16 err32 of each other.  Piecewise-constant images are excluded on purpose: their far-field responses are rounding noise in
    float64 too, and 20 to 60 % of their pixels sit that close to a tie."""
    u8 = R.quantize(R.make_image(kind, seed, H, W))
    bank = R.filter_bank(H, W)
    m64 = R.responses(u8, bank)
    err32 = np.abs(R.responses(u8, bank, single=True) - m64).max()
    assert 0 < err32 <= 2e-6 * m64.max()
    share = (R.top_two_gap(m64) < 16 * err32).reshape(4, -1).mean(1)
    print(name, 'err32 / max = %.3g' % (err32 / m64.max()), 'share below 16 err32 per scale:', share)
    assert np.all(share <= 0.01)
