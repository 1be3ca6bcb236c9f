"""GPU: the kernels of csrc/photometric.hip at every mean length, blur tile edge and ping-pong parity at which they take
another path, against numpy and the restatement tests/photometric_restatement.py.  tests/photometric_shape_cases.py builds
the inputs (once per process); tests/test_photometric_shapes_host.py checks their premises on the CPU: that every mean batch
can tell numpy's summation order from others, and that the restated blur and motion blur agree with a float64 evaluation.

What each test reaches that tests/test_gpu_photometric.py does not:

  test_mean_is_numpys[H-W]           photo_mean_kernel held to numpy's image.mean() bit for bit (a contrast of strength 0
                                     writes the mean into every pixel): the n < 8 leaf, the first split, the 65-leaf tail, the
                                     level-by-level reduction of full chunks, tail == MEAN_CHUNK, one to three groups of 16
                                     chunks, a group that holds only a 1-pixel tail, H as the long side, eight workgroups
  test_mean_of_the_pingpong_buffer   photo_cur_ptrs_kernel: the mean of an image whose current buffer is `alt`, alone and next
                                     to images whose current buffer is `out` or that have no contrast at that step
  test_blur_tiles[H-W]               blur_cols_kernel with a second row of tiles of one row (H = 65), three rows of tiles,
                                     H = 1 and W = 1 (reflect101's n == 1), a 15 / 16 / 17 / 33 pixel row of tiles, k = 1 and
                                     k = MP_PHOTO_MAX_BLUR, images of different k in one launch; shade_ellipse_kernel with
                                     ellipses centred on the corners, on the edges and outside the frame
  test_motion_blur_sizes[H-W]        every mode at 1, 3 and MP_PHOTO_MAX_TAPS taps, frames smaller than the kernel
  test_parity[H-W]                   one to eight motion blurs per plan, elementwise steps and a mean while `alt` is current,
                                     photo_copy_back_kernel on a batch of mixed parity and plan length, out aliased to images
  test_refusals / test_shade_lds_limit   the limits of photometric_check, the static LDS of shade_ellipse_kernel included
"""
import ctypes

import numpy as np
import pytest
import torch

import photometric_restatement as R
import photometric_shape_cases as C
from multipoint_amd import _lib
from multipoint_amd.datasets import augmentation as A

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _plan(shape, ops):
    return A.PhotometricPlan(tuple(shape), 'host', ops)


def _chain(shape, spec):
    return _plan(shape, C.plan_ops(spec, A._motion_taps))


def _contrast(shape, strength):
    return _plan(shape, [{'name': 'random_contrast', 'value': strength}])


def _device(imgs):
    return torch.from_numpy(np.array(imgs, np.float32)).to(DEV)[:, None]


def _run(imgs, plans):
    """(n, H, W) numpy in, (n, H, W) numpy out"""
    return A.photometric_augmentation_batch(_device(imgs), plans)[:, 0].cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the mean ----
@pytest.mark.parametrize('H,W', C.MEAN_SHAPES)
def test_mean_is_numpys(H, W):
    """random_contrast computes clip01((x - m) * s + m).  With s = 0 the product is +-0 and every output pixel is m itself
    (0 <= m < 1), so the batch shows the kernel's mean of each image: it must be numpy's own float32 image.mean(), taken on
    the host.  With s = 1.3 the whole image must be the restatement's, and an image run alone must give the bits it gives
    inside the batch of eight."""
    imgs = C.mean_batch(H, W)
    n = len(imgs)
    got = _run(imgs, [_contrast((H, W), 0.0)] * n)
    for i in range(n):
        want = imgs[i].mean()
        assert want.dtype == np.float32
        assert np.all(got[i] == want), (i, C.MEAN_FAMILIES[i], float(got[i].flat[0]), float(want))
    plan = _contrast((H, W), 1.3)
    got = _run(imgs, [plan] * n)
    for i in range(n):
        assert np.array_equal(got[i], R.apply_plan(imgs[i], plan)), (i, C.MEAN_FAMILIES[i])
        alone = _run(imgs[i:i + 1], [plan])[0]
        assert np.array_equal(_bits(alone), _bits(got[i])), i


@pytest.mark.parametrize('H,W', [(17, 8192), (31, 45)])
def test_mean_of_the_pingpong_buffer(H, W):
    """After one motion blur the image lives in `alt`; a contrast of strength 0 behind it must write the mean of the blurred
    image -- numpy's mean of the GPU's own [m] result -- into every pixel.  Then three images in one batch: contrast at step
    0 (current buffer `out`), contrast at step 1 behind a motion blur (current buffer `alt`), no contrast at all; each must
    equal its result when run alone."""
    imgs = C.mean_batch(H, W)[:3] if (H, W) in C.MEAN_SHAPES else C.parity_batch(H, W)[:3]
    blur = ('m', 2, 5)
    b = _run(imgs[1:2], [_chain((H, W), [blur])])[0]
    assert not np.array_equal(b, imgs[1])
    got = _run(imgs[1:2], [_chain((H, W), [blur, ('c', 0.0)])])[0]
    assert np.all(got == b.mean()), (float(got.flat[0]), float(b.mean()))
    plans = [_chain((H, W), [('c', 1.3), ('b', 0.05)]), _chain((H, W), [blur, ('c', 0.0)]),
             _chain((H, W), [('m', 1, 3), ('b', -0.1)])]
    batch = _run(imgs, plans)
    assert np.all(batch[1] == b.mean())
    for i in range(3):
        alone = _run(imgs[i:i + 1], [plans[i]])[0]
        assert np.array_equal(_bits(batch[i]), _bits(alone)), i
        assert np.array_equal(batch[i], R.apply_plan(imgs[i], plans[i])), i


# ---- blur tiles ----
@pytest.mark.parametrize('H,W', C.BLUR_FRAMES)
def test_blur_tiles(H, W):
    """One batch per frame, one image per blur size of C.blur_ksizes (the launch's LDS is sized by the largest k, each image
    uses its own radius).  The raw mask must be R.cv_ellipse_fill's exactly; the blurred mask within 2e-6 of R.gaussian_blur,
    the bound of test_gpu_photometric.py::test_shade_mask_and_blur (the weights' exp is evaluated on the device).

    Why an ellipse on or outside the frame writes no row outside [0, H) (from reading shade_ellipse_kernel and mp_raster.h):
    the outline goes through line2, which returns when clip_line rejects the segment and otherwise walks a segment clipped to
    the frame, and every pixel of it goes through `put`, which tests 0 <= x < W and 0 <= y < H itself.  convex_spans returns
    before its loop when the polygon's bounding box misses the frame (xmax < 0, ymax < 0, xmin >= W or ymin >= H); otherwise
    it clamps ymax to H - 1, walks y from ymin to ymax and calls span only for y >= 0, so spans[2 * y] and spans[2 * y + 1]
    stay inside the 2 H ints of dynamic LDS, and [ylo, yhi] are the first and last of those consecutive rows.  The span it
    passes is clipped to [0, W - 1] or is the empty (1, 0), so the fill loop writes columns 0 .. W - 1 of rows ylo .. yhi
    only.  A polygon of fewer than three vertices (no span) leaves yhi = -1: no row."""
    case = C.blur_case(H, W)
    plans = [_plan((H, W), [{'name': 'additive_shade', 'value': 0.5, 'ksize': k, 'ellipses': ells}]) for k, ells in case]
    want = C.blur_masks(H, W)
    raw = A.photometric_shade_masks(plans, 0, blurred=False, device=DEV).cpu().numpy()
    blurred = A.photometric_shade_masks(plans, 0, blurred=True, device=DEV).cpu().numpy()
    worst = 0.0
    for i, (k, _) in enumerate(case):
        assert np.array_equal(raw[i], want[i]), (k, int((raw[i] != want[i]).sum()))
        dev = float(np.abs(blurred[i] - R.gaussian_blur(want[i], k)).max())
        worst = max(worst, dev)
        print('blur %dx%d k=%d: max deviation %.3e' % (H, W, k, dev))
        assert dev <= 2e-6, k
        if k == 1:
            assert np.array_equal(blurred[i], want[i])
    print('blur %dx%d: worst %.3e' % (H, W, worst))


# ---- motion blur ----
@pytest.mark.parametrize('H,W', C.MOTION_FRAMES)
def test_motion_blur_sizes(H, W):
    """Every mode at 1, 3 and 11 taps in one batch, against R.filter2d with the reference's kernel (R.motion_taps).  Equality
    is expected: the float32 taps come from the host, the kernel sums s = 0; s = s + tap * pixel in the taps' row-major order
    with contraction off, as the restatement does."""
    imgs = C.motion_batch(H, W)
    plans = [_chain((H, W), [('m', mode, k)]) for mode, k in C.MOTION_PARAMS]
    got = _run(imgs, plans)
    for i, (mode, k) in enumerate(C.MOTION_PARAMS):
        want = R.filter2d(imgs[i], R.motion_taps(C.MOTION_MODES[mode], k))
        dev = float(np.abs(got[i] - want).max())
        print('motion %dx%d mode %d k=%d: max deviation %.3e' % (H, W, mode, k, dev))
        assert np.array_equal(got[i], want), (mode, k, dev)


# ---- parity ----
@pytest.mark.parametrize('H,W', C.PARITY_FRAMES)
def test_parity(H, W):
    """The chains of C.PARITY_PLANS (brightness, contrast and motion blur only: exact against R.apply_plan) as one batch of
    mixed parity and plan length, each image alone, and the batch again with out aliased to images."""
    imgs = C.parity_batch(H, W)
    plans = [_chain((H, W), spec) for spec in C.PARITY_PLANS]
    assert max(len(p.ops) for p in plans) == _lib.MP_PHOTO_MAX_OPS
    batch = _run(imgs, plans)
    for i, spec in enumerate(C.PARITY_PLANS):
        assert np.array_equal(batch[i], R.apply_plan(imgs[i], plans[i])), spec
        alone = _run(imgs[i:i + 1], [plans[i]])[0]
        assert np.array_equal(_bits(alone), _bits(batch[i])), spec
        if not spec:
            assert np.array_equal(_bits(batch[i]), _bits(imgs[i]))
    t = _device(imgs)
    ret = A.photometric_augmentation_batch(t, plans, out=t)
    assert ret.data_ptr() == t.data_ptr()
    assert np.array_equal(_bits(t[:, 0].cpu().numpy()), _bits(batch))


# ---- refusals ----
def _raw_shade_mask(c_plans, n_ellipses, H, W):
    """mp_photometric_shade_mask on hand-made ctypes plans (what no PhotometricPlan can express)"""
    n = len(c_plans)
    ell = np.zeros((max(n_ellipses, 1), 5), np.int32)
    ell[:, 2:4] = 1
    ws = A._workspace(n, H, W, n_ellipses, torch.device(DEV))
    out = torch.zeros((n, H, W), dtype=torch.float32, device=DEV)
    h = _lib.get_handle(torch.device(DEV))
    with torch.cuda.device(DEV):
        h.check(h.lib.mp_photometric_shade_mask(h.ptr, n, H, W, c_plans, ell.ctypes.data_as(ctypes.c_void_p), n_ellipses, 0,
                                                0, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(torch.device(DEV))))
    return out


def test_refusals():
    """photometric_check returns before any launch"""
    H, W = 8, 8
    img = torch.zeros((1, 1, H, W), device=DEV)
    bright = {'name': 'random_brightness', 'value': 0.1}
    with pytest.raises(ValueError, match='at most 16'):                                    # 17 ops: the Python binding
        A.photometric_augmentation_batch(img, [_plan((H, W), [bright] * 17)])
    taps = A._motion_taps('h', 11)
    for mode, k in ((0, 13), (4, 3)):
        with pytest.raises(ValueError, match='motion blur needs'):
            A.photometric_augmentation_batch(img, [_plan((H, W), [{'name': 'motion_blur', 'mode': mode, 'ksize': k,
                                                                   'taps': taps}])])
    shade = {'name': 'additive_shade', 'value': 0.5, 'ksize': 803, 'ellipses': [(4, 4, 2, 2, 0)]}
    with pytest.raises(ValueError, match='blur size must be odd'):
        A.photometric_augmentation_batch(img, [_plan((H, W), [shade])])
    with pytest.raises(ValueError, match='blur size must be odd'):
        A.photometric_shade_masks([_plan((H, W), [shade])], 0, device=DEV)
    # through ctypes: 17 ops, and an ellipse range past the table (2 + 1 > 2)
    c = (_lib.PhotometricPlan * 1)()
    c[0].n_ops = 17
    with pytest.raises(ValueError, match='n_ops outside'):
        _raw_shade_mask(c, 0, H, W)
    c[0].n_ops = 1
    c[0].op[0].kind, c[0].op[0].ksize = 4, 3
    c[0].op[0].ellipse_offset, c[0].op[0].ellipse_count = 2, 1
    with pytest.raises(ValueError, match='ellipses outside the table'):
        _raw_shade_mask(c, 2, H, W)
    c[0].op[0].ellipse_offset = 1                                                           # the last entry of the table
    assert float(_raw_shade_mask(c, 2, H, W).sum()) > 0


def test_shade_lds_limit():
    """shade_ellipse_kernel asks for 8 H bytes of dynamic LDS next to its static vertex arrays (2576 bytes).  Together they
    fit the 65536 bytes of photometric_check up to H = 7870: that frame runs and gives the restatement's mask, H = 7871 is
    refused with the check's error before any launch.  Plans without a shade op need no spans and run up to H = 8192
    (test_mean_is_numpys[8192-1])."""
    assert C.photometric_lds_bytes(7870, 2, 1) == C.LDS_LIMIT < C.photometric_lds_bytes(7871, 2, 1)
    W = 2
    for H, fits in ((7870, True), (7871, False)):
        ells = [(0, H - 1, 1, 3, 0), (1, H // 2, 2, 2, 37), (0, 0, 1, 1, 90)]
        plan = _plan((H, W), [{'name': 'additive_shade', 'value': 0.5, 'ksize': 1, 'ellipses': ells}])
        if not fits:
            with pytest.raises(ValueError, match='frame too wide for the blur size'):
                A.photometric_shade_masks([plan], 0, blurred=False, device=DEV)
            with pytest.raises(ValueError, match='frame too wide for the blur size'):
                A.photometric_augmentation_batch(torch.zeros((1, 1, H, W), device=DEV), [plan])
            continue
        want = np.zeros((H, W), np.float32)
        for x, y, ax, ay, angle in ells:
            R.cv_ellipse_fill(want, (x, y), (ax, ay), angle)
        got = A.photometric_shade_masks([plan], 0, blurred=False, device=DEV)[0].cpu().numpy()
        assert want.any() and np.array_equal(got, want)
