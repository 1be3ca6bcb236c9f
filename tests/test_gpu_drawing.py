"""GPU: the result views of multipoint_amd.utils.drawing (csrc/draw.hip) against their numpy restatement
(tests/drawing_restatement.py), byte for byte: everything is integer arithmetic or a single fp32 product.  Every comparison is
made on a canvas with a sentinel fill, so pixels outside the drawn set are checked too, and every call is made twice."""
import ctypes

import numpy as np
import pytest
import torch

import drawing_restatement as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = 201


def _twice(fn):
    """fn() -> uint8 tensor; the bytes of two identical calls must agree"""
    a = fn().cpu().numpy().copy()
    b = fn().cpu().numpy()
    assert np.array_equal(a, b), 'two identical calls differ'
    return a


def _values(n, gain, seed):
    """n fp32 values that start with the edges of the 8-bit conversion: below 0, above 1, k / 255 (over the gain) and its two
    fp32 neighbours, 1.0, -0.0, NaN"""
    rng = np.random.default_rng(seed)
    special = [-1.0, -1e-3, 1.5, 1.0, -0.0, np.nan, 0.0, 1e-30, np.inf, -np.inf]
    for k in (0, 1, 2, 3, 85, 127, 128, 200, 254, 255):
        v = np.float32(np.float32(k) / np.float32(255) / np.float32(gain))
        special += [v, np.nextafter(v, np.float32(-9)), np.nextafter(v, np.float32(9))]
    special = np.array(special, np.float32)
    out = (rng.random(n, dtype=np.float32) * 1.4 - 0.2) / np.float32(gain)
    start = seed % len(special)
    m = min(n, len(special))
    out[:m] = np.roll(special, -start)[:m]
    return out.astype(np.float32)


@pytest.mark.parametrize('gain', [1.0, 60.0])
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 5, 7), (3, 16, 33), (1, 64, 80)])
def test_gray_to_rgb(shape, masked, gain):
    from multipoint_amd.utils import drawing as D
    B, H, W = shape
    rng = np.random.default_rng(B * 1000 + H)
    mask = None
    for seed in ((0, 5, 11, 17, 23, 29) if H * W == 1 else (3,)):       # the single pixel takes one edge value per round
        x = _values(B * H * W, gain, seed).reshape(B, H, W)
        if masked:
            mask = rng.choice(np.array([0.0, 1.0, 1.0, 0.5], np.float32), size=(B, H, W))
        xd = torch.from_numpy(x).to(DEV)
        md = None if mask is None else torch.from_numpy(mask).to(DEV)
        want = R.gray_to_rgb(np.zeros((B, H, W, 3), np.uint8), x, mask, gain)
        assert np.array_equal(_twice(lambda: D.gray_to_rgb(xd, md, gain)), want)
        if gain == 1.0 and not masked:                      # the reference's expression itself
            assert np.array_equal(want[..., 0], (np.clip(np.nan_to_num(x, nan=0.0), 0, 1) * 255.0).astype(np.uint8))
        # into a larger canvas: an odd offset, one whose rows are dword-aligned, one partly and one wholly off the canvas
        for offset in ((3, 5), (2, 4), (-2, -3), (H + 7, 0)):
            def call():
                canvas = torch.full((B, H + 7, W + 12, 3), SENTINEL, dtype=torch.uint8, device=DEV)
                assert D.gray_to_rgb(xd[:, None], md, gain, out=canvas, offset=offset) is canvas
                return canvas
            want = R.gray_to_rgb(np.full((B, H + 7, W + 12, 3), SENTINEL, np.uint8), x, mask, gain, offset)
            assert np.array_equal(_twice(call), want), offset
    if B == 1:                                               # one frame without the batch axis, a bool mask
        got = D.gray_to_rgb(xd[0], None if md is None else md[0] > 0, gain)
        want = R.gray_to_rgb(np.zeros((1, H, W, 3), np.uint8), x, None if mask is None else mask > 0, gain)
        assert got.shape == (1, H, W, 3) and np.array_equal(got.cpu().numpy(), want)


# (y, x) on a 24 x 40 canvas: the four corners, the four edges, the centre twice (a duplicate), two overlapping neighbours
MARKS = [(0, 0), (0, 39), (23, 0), (23, 39), (0, 20), (23, 20), (12, 0), (12, 39), (12, 20), (12, 20), (10, 18), (13, 23)]
PALETTES = {1: [(0, 255, 0)], 3: [(255, 0, 0), (0, 255, 0), (10, 20, 255)]}


def _marks_case(kp, counts, r, t, kind, palette, offset, shape=(2, 24, 40)):
    from multipoint_amd.utils import drawing as D
    B, H, W = shape
    kpd, cd = torch.from_numpy(kp).to(DEV), torch.from_numpy(np.asarray(counts, np.int32)).to(DEV)

    def call():
        canvas = torch.full((B, H, W, 3), SENTINEL, dtype=torch.uint8, device=DEV)
        assert D.draw_keypoints(canvas, kpd, cd, radius=r, thickness=t, kind=kind, offset=offset, palette=palette) is canvas
        return canvas
    want = R.draw_marks(np.full((B, H, W, 3), SENTINEL, np.uint8), kp, counts, r, t, kind, palette, offset)
    got = _twice(call)
    assert np.array_equal(got, want), (r, t, kind, len(palette), offset)
    return got


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('r', [0, 1, 4, 6, 59])
def test_draw_keypoints(r, kind):
    K = len(MARKS)
    kp = np.zeros((2, K, 2), np.int32)
    kp[0] = MARKS
    kp[1] = MARKS[::-1]
    drawn = 0
    for t in (1, 3, 5):
        for n, palette in PALETTES.items():
            # image 1 has no marks and image 0's count lies above K; then both draw, image 1 only its first three
            for counts in ((K + 5, 0), (K, 3)):
                # on the canvas; pushed partly off it; pushed wholly off it
                for offset in ((0, 0), (-3, 35), (100, -200)):
                    if (kind != 'ring' and t > 1) or (counts[1] and (n == 1 or offset != (0, 0))):
                        continue                             # disc and cross do not read t: once is enough
                    got = _marks_case(kp, counts, r, t, kind, palette, offset)
                    drawn += int((got != SENTINEL).any())
                    if counts[1] == 0:
                        assert (got[1] == SENTINEL).all()
                    if offset == (100, -200):
                        assert (got == SENTINEL).all()
    assert drawn


def test_draw_keypoints_single_list_forms():
    """K = 1, and one (N, 2) list for one canvas: a numpy array and a torch.nonzero result"""
    from multipoint_amd.utils import drawing as D
    _marks_case(np.array([[[5, 6]]], np.int32), (1,), 4, 1, 'ring', PALETTES[1], (0, 0), shape=(1, 24, 40))
    prob = torch.zeros((24, 40), device=DEV)
    for y, x in MARKS[:9]:
        prob[y, x] = 1.0
    nz = torch.nonzero(prob)                                 # int64 (N, 2), row-major order
    want = R.draw_marks(np.full((1, 24, 40, 3), SENTINEL, np.uint8), nz.cpu().numpy()[None], (nz.shape[0],), 4, 1, 'ring',
                        [(0, 0, 255)], (0, 0))
    for lst in (nz, nz.cpu().numpy()):
        canvas = torch.full((24, 40, 3), SENTINEL, dtype=torch.uint8, device=DEV)        # (H, W, 3): no batch axis
        D.draw_keypoints(canvas, lst, color=(0, 0, 255))
        assert np.array_equal(canvas.cpu().numpy(), want[0])
    empty = torch.full((24, 40, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    D.draw_keypoints(empty, np.zeros((0, 2), np.int64))
    assert (empty == SENTINEL).all()


def test_draw_keypoints_long_list_and_far_coordinates():
    """More marks than one pass over a tile lists (1024), coordinates up to +-2^20, a count below K"""
    rng = np.random.default_rng(7)
    K, n = 2500, 2300
    kp = np.stack([rng.integers(-4, 37, K), rng.integers(-4, 70, K)], -1).astype(np.int32)[None]
    kp[0, ::97] = rng.integers(-2 ** 20, 2 ** 20, (len(kp[0, ::97]), 2))
    kp[0, n:] = (16, 30)                                     # beyond the count: must not show
    kp[0, 5] = (-2 ** 20 + 10, 2 ** 20 + 20)                 # lands on (10, 20) under the last case's offset
    for kind, r, t in (('ring', 2, 1), ('cross', 3, 1), ('disc', 1, 1)):
        _marks_case(kp, (n,), r, t, kind, PALETTES[3], (0, 0), shape=(1, 33, 65))
    _marks_case(kp, (n,), 2, 3, 'ring', PALETTES[3], (2 ** 20, -2 ** 20), shape=(1, 33, 65))


H_M, W_M, K_M = 24, 40, 8


def _match_case():
    """Two pairs of 24 x 40 frames, K = 8; thermal keypoints are given in their own frame (the picture adds W = 40 to x), so a
    negative x puts the end of a segment anywhere on the canvas.  Pair 0: counts (7, 6); pair 1: counts above K."""
    kp_a = np.zeros((2, K_M, 2), np.int32)
    kp_b = np.zeros((2, K_M, 2), np.int32)
    idx = np.full((2, K_M), -1, np.int32)
    kp_a[0] = [(5, 3), (2, 15), (3, 2), (1, 10), (10, 25), (7, 7), (15, 20), (18, 30)]
    kp_b[0] = [(5, 30), (20, -25), (9, 35), (22, -25), (10, -30), (7, -33), (1, 1), (2, 2)]
    #          horizontal, vertical, shallow, steep, right to left, zero length, train index >= count_b, q >= count_a
    idx[0] = [0, 1, 2, 3, 4, 5, 6, 0]
    kp_a[1] = [(0, 0), (23, 0), (2, 6), (18, 6), (-5, -5), (9, 9), (12, 20), (3, 3)]
    kp_b[1] = [(23, 39), (0, 39), (18, 30), (2, 30), (40, 60), (12, -20), (0, 0), (0, 0)]
    #          canvas corner to corner twice, two crossing segments (q = 2, 3), both ends off the canvas, -1, zero length, -1
    idx[1] = [0, 1, 2, 3, 4, -1, 5, -1]
    counts_a, counts_b = np.array([7, 100], np.int32), np.array([6, 100], np.int32)
    mask = np.array([[1, 0, 1, 0, 1, 1, 1, 1], [0, 1, 1, 1, 2, 1, 1, 1]], np.uint8)
    rng = np.random.default_rng(2)
    optical, thermal = rng.random((2, H_M, W_M), dtype=np.float32), rng.random((2, H_M, W_M), dtype=np.float32)
    return optical, thermal, kp_a, kp_b, counts_a, counts_b, idx, mask


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('r,t', [(3, 1), (0, 1), (2, 3)])
def test_draw_matches(r, t, masked):
    from multipoint_amd.utils import drawing as D
    optical, thermal, kp_a, kp_b, ca, cb, idx, mask = _match_case()
    mask = mask if masked else None
    dev = [None if a is None else torch.from_numpy(a).to(DEV) for a in (optical, thermal, kp_a, kp_b, idx, ca, cb, mask)]
    for palette in (None, PALETTES[3], PALETTES[1]):
        want = R.match_picture(optical, thermal, kp_a, kp_b, ca, cb, idx, mask, r, t,
                               D.match_palette(64) if palette is None else palette)
        got = _twice(lambda: D.draw_matches(*dev, radius=r, thickness=t, palette=palette))
        assert got.shape == (2, H_M, 2 * W_M, 3) and np.array_equal(got, want)
    if not masked and (r, t) == (3, 1):
        # (the restatement itself) the segments q = 2 and q = 3 of pair 1 cross on pixel (38, 10), which shows the higher one;
        # pair 0's q = 6 (train index beyond count_b) and q = 7 (beyond count_a) leave the pixels around their keypoints alone
        want = R.match_picture(optical, thermal, kp_a, kp_b, ca, cb, idx, None, r, t, PALETTES[3])
        plain = R.match_picture(optical, thermal, kp_a, kp_b, ca, cb, np.full_like(idx, -1), None, r, t, PALETTES[3])
        crossing = set(R.line_pixels(80, 24, (6, 2), (70, 18))) & set(R.line_pixels(80, 24, (6, 18), (70, 2)))
        assert (38, 10) in crossing and all(tuple(want[1, y, x]) == PALETTES[3][3 % 3] for x, y in crossing)
        assert np.array_equal(want[0, 14:23, 19:35], plain[0, 14:23, 19:35]) and not np.array_equal(want[0], plain[0])


def test_draw_matches_far_coordinates():
    from multipoint_amd.utils import drawing as D
    big = 2 ** 20
    kp_a = np.array([[(-big, -big + 5), (big, 3), (4, -big)]], np.int32)
    kp_b = np.array([[(big, big), (-big, -big), (4, big)]], np.int32)
    idx = np.array([[0, 1, 2]], np.int32)
    optical = np.full((1, 17, 29), 0.5, np.float32)
    want = R.match_picture(optical, optical, kp_a, kp_b, (3,), (3,), idx, None, 2, 1, PALETTES[3])
    assert (want != 127).any()
    o = torch.from_numpy(optical).to(DEV)
    got = _twice(lambda: D.draw_matches(o, o, kp_a, kp_b, idx, radius=2, palette=PALETTES[3]))
    assert np.array_equal(got, want)


def test_draw_pair_results_is_the_array_call():
    from multipoint_amd.pipeline import PairPipeline, PairResults
    from multipoint_amd.utils import drawing as D
    optical, thermal, kp_a, kp_b, ca, cb, idx, mask = _match_case()
    kp = np.stack([kp_a, kp_b], 1).reshape(4, K_M, 2)       # image 2 p optical, 2 p + 1 thermal
    counts = np.stack([ca, cb], 1).reshape(4)
    t = lambda a: torch.from_numpy(a).to(DEV)
    res = PairResults(t(kp), None, t(counts), None, t(idx), None, None, H_M, W_M)
    images = PairPipeline.interleave(t(optical)[:, None], t(thermal)[:, None])
    for m in (None, t(mask)):
        got = _twice(lambda: D.draw_pair_results(res, images, mask=m, radius=2, thickness=3))
        want = D.draw_matches(t(optical), t(thermal), t(kp_a), t(kp_b), t(idx), t(ca), t(cb), m, radius=2, thickness=3)
        assert np.array_equal(got, want.cpu().numpy())
        assert np.array_equal(got, R.match_picture(optical, thermal, kp_a, kp_b, ca, cb, idx, None if m is None else mask, 2, 3,
                                                   D.match_palette(64)))


@pytest.mark.parametrize('mode', R.MODES)
def test_compose(mode):
    from multipoint_amd.utils import drawing as D
    rng = np.random.default_rng(4)
    a = (rng.random((2, 9, 13), dtype=np.float32) * 1.4 - 0.2).astype(np.float32)
    a[a < 0] = 0.01                                          # only the region below is outside
    t = (rng.random((2, 9, 13), dtype=np.float32) * 1.4 - 0.2).astype(np.float32)
    a[0, :4, 8:] = -1.0
    a[1, 6:, :] = -1.0
    a[1, 0, 0], t[1, 0, 1], t[1, 8, 2] = np.nan, np.nan, np.nan
    ad, td = torch.from_numpy(a).to(DEV), torch.from_numpy(t).to(DEV)
    for alpha in (0, 128, 256):
        for cell in (1, 4, 64):
            want = R.compose(a, t, mode, alpha, cell)
            assert np.array_equal(_twice(lambda: D.compose(ad, td, mode, alpha, cell)), want)
            if mode not in ('blend', 'checker') or (alpha, cell) == (128, 4):      # the other two modes read neither

                def call():
                    canvas = torch.full((2, 12, 20, 3), SENTINEL, dtype=torch.uint8, device=DEV)
                    D.compose(ad[:, None], td[:, None], mode, alpha, cell, out=canvas, offset=(2, 3))
                    return canvas
                sheet = R.paste(np.full((2, 12, 20, 3), SENTINEL, np.uint8), want, (2, 3))
                assert np.array_equal(_twice(call), sheet)
    if mode == 'blend':
        assert np.array_equal(R.compose(a, t, mode, 256, 1)[0, 5], np.repeat(R.to_u8(a)[0, 5][:, None], 3, 1))


def test_alignment_views_warp_and_compose():
    from multipoint_amd.utils import alignment, drawing as D
    rng = np.random.default_rng(9)
    optical = torch.from_numpy(rng.random((2, 1, 20, 28), dtype=np.float32)).to(DEV)
    thermal = torch.from_numpy(rng.random((2, 1, 16, 24), dtype=np.float32)).to(DEV)
    T = np.array([[1.0, 0.02, 3.5], [-0.01, 1.0, -2.25], [0.0, 0.0, 1.0]])
    views = D.alignment_views(optical, thermal, T, modes=R.MODES, alpha=77, cell=5)
    warped = alignment.warp_image(optical, T, 16, 24)[:, 0].cpu().numpy()
    assert (warped == -1).any() and (warped >= 0).any()
    for mode in R.MODES:
        assert np.array_equal(views[mode].cpu().numpy(), R.compose(warped, thermal[:, 0].cpu().numpy(), mode, 77, 5))


def test_refusals():
    from multipoint_amd import _lib
    from multipoint_amd.utils import drawing as D
    canvas = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV)
    kp = np.array([[[4, 4]]], np.int32)
    for kw in (dict(radius=-1), dict(radius=65), dict(radius=64, thickness=2), dict(radius=60, thickness=10),
               dict(thickness=0), dict(palette=[]), dict(kind='square')):
        with pytest.raises(ValueError):
            D.draw_keypoints(canvas, kp, **kw)
    D.draw_keypoints(canvas, kp, radius=64, kind='disc')     # the limit itself, and a ring whose outer radius is the limit
    D.draw_keypoints(canvas, kp, radius=63, thickness=3)
    x = torch.zeros((1, 8, 4), device=DEV)
    idx = np.zeros((1, 1), np.int32)
    for kw in (dict(radius=-1), dict(radius=64, thickness=2), dict(thickness=0), dict(palette=[])):
        with pytest.raises(ValueError):
            D.draw_matches(x, x, kp, kp, idx, **kw)
    for kw in (dict(alpha=-1), dict(alpha=257), dict(cell=0), dict(mode='sum')):
        with pytest.raises(ValueError):
            D.compose(x, x, **dict(dict(mode='blend'), **kw))
    # NULL tensors and non-positive sizes, at the C ABI
    h = _lib.get_handle(canvas.device)
    s = _lib.stream_ptr(canvas.device)
    f = torch.zeros((1, 8, 8), device=DEV)
    ints = torch.zeros(8, dtype=torch.int32, device=DEV)
    pal = torch.zeros((1, 3), dtype=torch.uint8, device=DEV)
    p, c, i, pl = _lib.ptr(f), _lib.ptr(canvas), _lib.ptr(ints), _lib.ptr(pal)
    gain = ctypes.c_float(1.0)
    bad = [h.lib.mp_draw_gray_to_rgb(h.ptr, None, None, 1, 8, 8, gain, c, 8, 8, 0, 0, s),
           h.lib.mp_draw_gray_to_rgb(h.ptr, p, None, 1, 8, 8, gain, None, 8, 8, 0, 0, s),
           h.lib.mp_draw_gray_to_rgb(h.ptr, p, None, 0, 8, 8, gain, c, 8, 8, 0, 0, s),
           h.lib.mp_draw_gray_to_rgb(h.ptr, p, None, 1, 0, 8, gain, c, 8, 8, 0, 0, s),
           h.lib.mp_draw_gray_to_rgb(h.ptr, p, None, 1, 8, 8, gain, c, 8, -1, 0, 0, s),
           h.lib.mp_draw_marks(h.ptr, None, i, 1, 1, 0, 1, 1, pl, 1, c, 8, 8, 0, 0, s),
           h.lib.mp_draw_marks(h.ptr, i, None, 1, 1, 0, 1, 1, pl, 1, c, 8, 8, 0, 0, s),
           h.lib.mp_draw_marks(h.ptr, i, i, 1, 1, 0, 1, 1, None, 1, c, 8, 8, 0, 0, s),
           h.lib.mp_draw_marks(h.ptr, i, i, 1, 1, 0, 1, 1, pl, 1, None, 8, 8, 0, 0, s),
           h.lib.mp_draw_marks(h.ptr, i, i, 1, 0, 0, 1, 1, pl, 1, c, 8, 8, 0, 0, s),
           h.lib.mp_draw_marks(h.ptr, i, i, 0, 1, 0, 1, 1, pl, 1, c, 8, 8, 0, 0, s),
           h.lib.mp_draw_marks(h.ptr, i, i, 1, 1, 0, 1, 1, pl, 0, c, 8, 8, 0, 0, s),
           h.lib.mp_draw_marks(h.ptr, i, i, 1, 1, 3, 1, 1, pl, 1, c, 8, 8, 0, 0, s),
           h.lib.mp_draw_matches(h.ptr, i, i, i, i, None, None, 1, 1, 0, 0, 0, 0, 1, 1, pl, 1, c, 8, 8, s),
           h.lib.mp_draw_matches(h.ptr, i, None, i, i, i, None, 1, 1, 0, 0, 0, 0, 1, 1, pl, 1, c, 8, 8, s),
           h.lib.mp_draw_matches(h.ptr, i, i, i, None, i, None, 1, 1, 0, 0, 0, 0, 1, 1, pl, 1, c, 8, 8, s),
           h.lib.mp_draw_matches(h.ptr, i, i, i, i, i, None, 1, 0, 0, 0, 0, 0, 1, 1, pl, 1, c, 8, 8, s),
           h.lib.mp_draw_matches(h.ptr, i, i, i, i, i, None, 1, 1, 0, 0, 0, 0, 1, 1, pl, 1, c, 0, 8, s),
           h.lib.mp_draw_compose(h.ptr, None, p, 1, 8, 8, 0, 128, 4, c, 8, 8, 0, 0, s),
           h.lib.mp_draw_compose(h.ptr, p, None, 1, 8, 8, 0, 128, 4, c, 8, 8, 0, 0, s),
           h.lib.mp_draw_compose(h.ptr, p, p, 1, 8, 8, 0, 128, 4, None, 8, 8, 0, 0, s),
           h.lib.mp_draw_compose(h.ptr, p, p, 1, 8, 0, 0, 128, 4, c, 8, 8, 0, 0, s)]
    assert bad == [-1] * len(bad), bad
    with pytest.raises(ValueError):
        h.check(bad[0])
    torch.cuda.synchronize()
    assert (canvas[0, 4, 4] == torch.tensor([0, 255, 0], dtype=torch.uint8, device=DEV)).all()    # only the two allowed calls drew
