"""GPU: the local residual field (csrc/residual.hip, multipoint_amd.utils.residual) against its numpy restatement
at the smallest shapes that can go wrong, its bit promises, the planted pairs of the host tests, the refusals, and the segment
drawing of the needle map against a numpy walk of the same rule.

Tolerances (residual_cases): integer peaks must agree in every window whose two best restated scores differ by more than DELTA
= 1e-5 (at most 2 % of a case's windows may lie inside it; measured: none); sub-pixel d within 4 x 1e-6 px and the scores within
4 x 4e-7, four times the restatement's own float32-against-float64 difference (measured 4.8e-7 px and 2.7e-7)."""
import numpy as np
import pytest
import torch

import residual_cases as C
import residual_restatement as R
from shapes_restatement import line_pixels

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KEYS = ('d', 'rho', 'rho0', 'second', 'n', 'status')


def _run(fo, ft, mask, shape, **kw):
    from multipoint_amd.utils import residual as U
    H, W, w, s, r = shape
    args = dict(window=w, stride=s, radius=r, min_valid=C.MIN_VALID, var_floor=C.VAR_FLOOR)
    args.update(kw)
    return U.residual_field_from_features(torch.from_numpy(np.ascontiguousarray(fo)).to(DEV),
                                          torch.from_numpy(np.ascontiguousarray(ft)).to(DEV),
                                          None if mask is None else np.ascontiguousarray(mask), **args)


def _same_bytes(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in KEYS)


def _frame(f, b):
    return {k: f[k][b:b + 1] for k in KEYS}


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('kind', C.MASKS)
@pytest.mark.parametrize('shape', C.SHAPES, ids=lambda s: '%dx%d_w%d_s%d_r%d' % s)
def test_kernel_against_restatement(shape, kind, B):
    fo, ft = C.shape_frames(shape)
    mask = C.shape_mask(shape, kind)
    ref = {k: v[:B] if k != 'origin' else v for k, v in C.restated(shape, kind, True).items()}
    got = _run(fo[:B], ft[:B], mask if mask is None or mask.ndim == 2 else mask[:B], shape)
    assert np.array_equal(got['origin'], ref['origin'])
    assert np.array_equal(got['status'], ref['status']) and np.array_equal(got['n'], ref['n'])
    sel = C.decided(ref)
    left_out = 1.0 - sel.mean()
    assert left_out <= C.LEFT_OUT_CAP
    peak = sel & np.isin(ref['status'], (R.OK, R.AT_EDGE))
    assert np.array_equal(np.rint(got['d'][peak]), np.rint(ref['d'][peak]))
    dd, ds = C.max_difference(got, ref, sel)
    print('%s %s B=%d: left out %.3f, d %.3g px, scores %.3g' % (shape, kind, B, left_out, dd, ds))
    assert dd <= C.MARGIN * C.F32_DIFFERENCE['d'] and ds <= C.MARGIN * C.F32_DIFFERENCE['score']


@pytest.mark.parametrize('kind', ['none', 'per_frame'])
@pytest.mark.parametrize('shape', [C.SHAPES[1], C.SHAPES[3], C.SHAPES[6]], ids=lambda s: '%dx%d_w%d' % s[:3])
def test_bits(shape, kind):
    fo, ft = C.shape_frames(shape)
    mask = C.shape_mask(shape, kind)
    whole = _run(fo, ft, mask, shape)
    assert _same_bytes(whole, _run(fo, ft, mask, shape)), 'two identical calls differ'
    for b in range(C.FRAMES):                                          # a frame alone has the bits it has in the batch
        alone = _run(fo[b:b + 1], ft[b:b + 1], None if mask is None else mask[b:b + 1], shape)
        assert _same_bytes(alone, _frame(whole, b)), b
    perm = [2, 0, 1]
    shuffled = _run(fo[perm], ft[perm], None if mask is None else mask[perm], shape)
    for at, b in enumerate(perm):
        assert _same_bytes(_frame(shuffled, at), _frame(whole, b)), (at, b)
    if mask is None:                                                   # no mask is a mask of ones
        assert _same_bytes(whole, _run(fo, ft, np.ones(fo.shape[1:], np.uint8), shape))


@pytest.fixture(scope='module')
def planted_fields():
    from multipoint_amd.utils import residual as U
    out = {}
    kinds = ('integer', 'fractional', 'two_region')
    o = torch.from_numpy(np.stack([C.planted(k)[0] for k in kinds])).to(DEV)
    t = torch.from_numpy(np.stack([C.planted(k)[1] for k in kinds])).to(DEV)
    p = C.PARAMS
    f = U.residual_field(o, t, window=p['w'], stride=p['s'], radius=p['r'], min_valid=p['min_valid'], var_floor=p['var_floor'])
    for b, k in enumerate(kinds):
        one = {key: f[key][b] for key in KEYS}
        one['origin'] = f['origin']
        out[k] = (one, C.planted(k)[2])
    return out


def test_planted_integer(planted_fields):
    f, _ = planted_fields['integer']
    conf = C.confident(f)
    assert conf.sum() >= C.MIN_CONFIDENT['integer']
    assert (np.rint(f['d'][conf]) == np.array([2.0, -3.0])).all()
    assert (np.abs(f['d'][conf] - np.array([2.0, -3.0])) < 0.5).all()
    assert (f['n'][conf] == 32 * 32).all()


@pytest.mark.parametrize('kind', ['fractional', 'two_region'])
def test_planted_fractional(planted_fields, kind):
    f, truth = planted_fields[kind]
    errs, n, total = C.planted_errors(f, truth)
    print('%s: %d confident windows with a truth of %d, largest error %.4f px (recorded %.3f)' % (kind, n, total, errs.max(),
                                                                                                   C.REACHED[kind]))
    assert n >= C.MIN_CONFIDENT[kind]
    assert errs.max() <= C.PLANTED_MARGIN * C.REACHED[kind]


def test_planted_matches_restated_features():
    """utils.residual.residual_field's own features and mask growth: the integer pair with an optical mask, against the
    restatement on restated features and a mask grown by the same radius."""
    from multipoint_amd.utils import residual as U
    from multipoint_amd.utils.ecc import ecc_mask_radii
    o, t, _ = C.planted('integer')
    mask = np.ones(C.HW, np.uint8)
    mask[:, :30] = 0
    p = C.PARAMS
    got = U.residual_field(torch.from_numpy(o).to(DEV), torch.from_numpy(t).to(DEV), window=p['w'], stride=p['s'], radius=p['r'],
                           optical_mask=mask, min_valid=p['min_valid'], var_floor=p['var_floor'])
    grown = np.ones(C.HW, np.uint8)
    grown[:, :30 + ecc_mask_radii('gradient', 5)[1]] = 0
    ref = R.field(C.features(o), C.features(t), grown, f32=True, **p)
    assert np.array_equal(got['status'][0], ref['status']) and np.array_equal(got['n'][0], ref['n'])
    assert (ref['status'] == R.FEW_VALID).any() and (ref['status'] == R.OK).any()
    ok = ref['status'] == R.OK
    assert np.abs(got['d'][0][ok] - ref['d'][ok]).max() <= C.MARGIN * C.F32_DIFFERENCE['d']
    assert np.abs(got['rho'][0][ok] - ref['rho'][ok]).max() <= C.MARGIN * C.F32_DIFFERENCE['score']


def test_tie_order():
    a = np.array([[0.1, 0.7], [0.4, 0.9]], np.float32)
    fo = np.tile(a, (12, 12))[None]
    f = _run(fo, fo.copy(), None, (24, 24, 8, 4, 2), var_floor=0.0)
    assert (f['d'] == np.array([-2.0, -2.0])).all() and (f['status'] == R.AT_EDGE).all()
    assert (f['second'] == f['rho']).all() and (f['rho0'] == f['rho']).all()


def test_refusals():
    from multipoint_amd import _lib
    from multipoint_amd.utils import residual as U
    x = torch.rand((1, 48, 48), device=DEV)
    h = _lib.get_handle(x.device)
    out_d = torch.full((1, 1, 1, 5), 7.0, dtype=torch.float64, device=DEV)
    out_i = torch.full((1, 1, 1, 2), 7, dtype=torch.int32, device=DEV)

    def call(H, W, w, s, r, B=1, min_valid=0.5, var_floor=0.0, mask=None, mask_frames=1):
        return h.lib.mp_residual_field(h.ptr, _lib.ptr(x), _lib.ptr(x), _lib.ptr(mask), mask_frames, B, H, W, w, s, r, min_valid,
                                       var_floor, _lib.ptr(out_d), _lib.ptr(out_i), _lib.stream_ptr(x.device))
    assert call(47, 48, 32, 16, 8) == -1                               # no window
    assert b'no window' in h.lib.mp_last_error(h.ptr)
    assert call(48, 48, 32, 16, 9) == -1 and call(48, 48, 20, 16, 8) == -1
    assert call(48, 48, 32, 0, 8) == -1 and call(48, 48, 32, 16, 0) == -1
    assert call(48, 48, 32, 16, 8, B=0) == -1 and call(48, 48, 32, 16, 8, B=65536) == -1
    assert call(48, 48, 32, 16, 8, min_valid=0.0) == -1 and call(48, 48, 32, 16, 8, var_floor=-1.0) == -1
    assert call(4097, 48, 32, 16, 8) == -1
    m = torch.ones((1, 48, 48), dtype=torch.uint8, device=DEV)
    assert call(48, 48, 32, 16, 8, mask=m, mask_frames=2) == -1
    torch.cuda.synchronize()
    assert (out_d == 7.0).all() and (out_i == 7).all()                 # nothing was launched
    assert call(48, 48, 32, 16, 8) == 0
    torch.cuda.synchronize()
    assert int(out_i[0, 0, 0, 0]) == 32 * 32
    with pytest.raises(ValueError):
        U.residual_field(x, x, window=32, stride=16, radius=9)
    with pytest.raises(ValueError):
        U.residual_field(x, x, window=20)
    with pytest.raises(ValueError):
        U.residual_field(x[:, :47], x[:, :47], window=32, stride=16, radius=8)
    with pytest.raises(ValueError):
        U.residual_field(x, torch.rand((1, 48, 50), device=DEV))


# ---------------------------------------------------------------------------------------------------------------------------
# segments
# ---------------------------------------------------------------------------------------------------------------------------
def _segments_numpy(canvas, seg, count, t, palette):
    """The rule of mp_segments_draw: the LINE_8 walk clipped to the canvas, every pixel a t x t box, ascending index."""
    B, Hc, Wc = canvas.shape[:3]
    lo, hi = (t - 1) // 2, t // 2
    for b in range(B):
        for i in range(min(max(int(count[b]), 0), seg.shape[1])):
            y0, x0, y1, x1, c = (int(v) for v in seg[b, i])
            for x, y in line_pixels(Wc, Hc, (x0, y0), (x1, y1)):
                canvas[b, max(y - lo, 0):min(y + hi, Hc - 1) + 1, max(x - lo, 0):min(x + hi, Wc - 1) + 1] = palette[c % len(palette)]
    return canvas


@pytest.mark.parametrize('thickness', [1, 3])
def test_draw_segments(thickness):
    from multipoint_amd.utils import drawing as D
    Hc, Wc = 32, 48
    rng = np.random.RandomState(9)
    fixed = [(5, 5, 20, 40, 0), (20, 40, 5, 5, 1), (0, 0, 31, 47, 2), (31, 0, 0, 47, 0), (0, 10, 31, 10, 1), (7, 0, 7, 47, 2),
             (10, 10, 10, 10, 0), (0, 0, 0, 0, 1), (31, 47, 31, 47, 2),                 # zero length: inside and on the corners
             (-5, -7, 12, 30, 0), (16, 20, 60, 90, 1), (-10, 24, 50, 25, 2), (40, -9, -3, 60, 0),      # end points outside
             (-4, -4, -4, 60, 1), (50, 50, 50, 50, 2), (3, -20, 3, -2, 0), (15, 47, 15, 70, 1),        # wholly outside / touching
             (31, 5, 31, 30, 2), (5, 47, 25, 47, 0)]                                                   # on the edge
    extra = np.concatenate([rng.randint(-12, Hc + 12, (14, 1)), rng.randint(-12, Wc + 12, (14, 1)),
                            rng.randint(-12, Hc + 12, (14, 1)), rng.randint(-12, Wc + 12, (14, 1)), rng.randint(0, 7, (14, 1))], 1)
    one = np.concatenate([np.array(fixed, np.int64), extra])
    seg = np.stack([one, one[::-1]])                                    # the second canvas: the other layer order
    count = np.array([len(one), len(one) - 5])
    palette = np.array([[0, 255, 0], [255, 0, 0], [10, 20, 250]], np.uint8)
    want = _segments_numpy(np.full((2, Hc, Wc, 3), 201, np.uint8), seg, count, thickness, palette)

    def draw():
        canvas = torch.full((2, Hc, Wc, 3), 201, dtype=torch.uint8, device=DEV)
        return D.draw_segments(canvas, seg, count, thickness, palette)
    a = draw().cpu().numpy().copy()
    assert np.array_equal(a, draw().cpu().numpy()), 'two identical calls differ'
    assert np.array_equal(a, want)
    single = D.draw_segments(torch.full((Hc, Wc, 3), 201, dtype=torch.uint8, device=DEV), one, None, thickness, palette)
    assert np.array_equal(single.cpu().numpy(), _segments_numpy(np.full((1, Hc, Wc, 3), 201, np.uint8), one[None], [len(one)],
                                                                thickness, palette)[0])
    for bad in (0, 16):
        with pytest.raises(ValueError):
            D.draw_segments(torch.zeros((Hc, Wc, 3), dtype=torch.uint8, device=DEV), one, None, bad, palette)


def test_draw_residual_field():
    from multipoint_amd.utils import drawing as D
    from multipoint_amd.utils import residual as U
    o, t, _ = C.planted('two_region')
    p = C.PARAMS
    f = U.residual_field(torch.from_numpy(o).to(DEV), torch.from_numpy(t).to(DEV), window=p['w'], stride=p['s'], radius=p['r'])
    f['status'][0, 0, 0] = R.FLAT                                       # one window that is not confident: a grey ring

    def draw():
        canvas = D.gray_to_rgb(torch.from_numpy(t).to(DEV))[0].contiguous()
        return D.draw_residual_field(canvas, f, 0, scale=4)
    a = draw().cpu().numpy().copy()
    assert a.tobytes() == draw().cpu().numpy().tobytes()
    green, red, grey = ((a == np.array(c, np.uint8)).all(-1) for c in ((0, 255, 0), (255, 0, 0), (128, 128, 128)))
    assert green.any() and red.any()
    cy, cx = f['origin'][0, 0] + p['w'] // 2
    assert grey[cy - 2, cx] and grey[cy, cx + 2] and not grey[cy, cx] and not green[cy, cx]
    assert green[:, :40].any() and not red[:, :40].any()                # the left half is aligned: green needles only
    assert red[:, 96:].any() and not green[:, 96:].any()                # the right half is 2.8 px off: red needles only
