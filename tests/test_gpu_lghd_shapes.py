"""GPU: the kernels of csrc/fft.hip and csrc/lghd.hip at every line length, column-bundle width, thread count and ARGMAX slot
they have code for, on the inputs of tests/lghd_shape_cases.py (whose premises tests/test_lghd_shapes_host.py checks without a
device): the FFT at all 131 lengths against np.fft in float64, the orientation maps of the smallest frames that reach each
launch shape and of the model's 512 x 640 frame against the float64 arg-max, inputs with exact answers, batches that take several
trips through the workspace, descriptors of a ragged batch, and FAST on frames around its 64 x 4 block."""
import ctypes

import numpy as np
import pytest
import torch

import lghd_restatement as R
import lghd_shape_cases as S

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GROUPS = S.length_groups()


@pytest.fixture(scope='module')
def C():
    from multipoint_amd.models import classic_detectors
    return classic_detectors


def _gpu_bank(H, W):
    return torch.from_numpy(S.bank(H, W).astype(np.float32)).to(DEV)


def _maps(C, u8, H, W):
    return C.orientation_maps(torch.from_numpy(np.ascontiguousarray(u8)).to(DEV), _gpu_bank(H, W)).cpu().numpy()


# ---- a. the FFT at every length ----

def _sweep(C, what, n, x, axes):
    for inverse in (False, True):
        got = C.fft2d(torch.from_numpy(x).to(DEV), inverse=inverse, axes=axes).cpu().numpy()
        err, err32 = S.fft_errors(got, x, {1: (-1,), 2: (-2,)}[axes], inverse)
        print('n = %d %s inverse %d: gpu %.3g, np.fft float32 %.3g, ratio %.2f' % (n, what, inverse, err, err32, err / err32))
        assert err <= S.FFT_SWEEP_BOUND * err32


@pytest.mark.parametrize('group', range(len(GROUPS)), ids=['%d-%d' % (g[0], g[-1]) for g in GROUPS])
def test_fft_rows_at_every_length(C, group):
    for n in GROUPS[group]:
        _sweep(C, 'rows', n, S.complex_noise(n, S.ROW_LINES + (n,)), 1)


@pytest.mark.parametrize('group', range(len(GROUPS)), ids=['%d-%d' % (g[0], g[-1]) for g in GROUPS])
def test_fft_columns_at_every_length(C, group):
    """19 columns: one full bundle and a partial one at 16 columns, more and a partial one at 8, 4 and 2"""
    for n in GROUPS[group]:
        _sweep(C, 'columns of %d' % S.COLUMN_WIDTHS[0], n, S.complex_noise(n + 1, (2, n, S.COLUMN_WIDTHS[0])), 2)


@pytest.mark.parametrize('n', S.NARROW_LENGTHS)
def test_fft_three_columns(C, n):
    """a frame narrower than the bundle (16, 16 and 8 columns), and at 4096 a bundle of 2 and one of a single column"""
    _sweep(C, 'columns of %d' % S.COLUMN_WIDTHS[1], n, S.complex_noise(n + 2, (1, n, S.COLUMN_WIDTHS[1])), 2)


# ---- b. small 2-D transforms ----

@pytest.mark.parametrize('shape', S.PLANES_2D, ids=['x'.join(map(str, s)) for s in S.PLANES_2D])
def test_fft_2d_there_and_back(C, shape):
    """several planes, rows and then columns in place: the forward transform against np.fft in float64, and forward then inverse
    over H W against the input, each within the sweep's bound of what np.fft does in float32"""
    x = S.complex_noise(shape[1] * 10000 + shape[2], shape)
    t = torch.from_numpy(x).to(DEV)
    spec = C.fft2d(t)
    err, err32 = S.fft_errors(spec.cpu().numpy(), x, (-2, -1), False)
    print('%s forward: gpu %.3g, np.fft float32 %.3g, ratio %.2f' % (shape, err, err32, err / err32))
    assert err <= S.FFT_SWEEP_BOUND * err32
    back = C.fft2d(spec, inverse=True).cpu().numpy().astype(np.complex128) / (shape[1] * shape[2])
    single = np.fft.ifft2(np.fft.fft2(x))
    assert single.dtype == np.complex64
    top = np.abs(x).max()
    err, err32 = np.abs(back - x).max() / top, np.abs(single - x).max() / top
    print('%s there and back: gpu %.3g, np.fft float32 %.3g, ratio %.2f' % (shape, err, err32, err / err32))
    assert err <= S.FFT_SWEEP_BOUND * err32
    assert np.array_equal(t.cpu().numpy(), x)                       # the input is not written


# ---- c. orientation maps ----

@pytest.mark.parametrize('name', S.FRAME_NAMES)
def test_orientation_maps(C, name):
    u8, _, m64, err32, want = S.reference(name)
    H, W = u8.shape
    got = _maps(C, u8[None], H, W)
    assert got.shape == (1, 4, H, W) and got.dtype == np.uint8
    S.check_orientation(got[0], name, m64, err32, want)


# ---- d. exact cases ----

@pytest.mark.parametrize('H,W', S.FRAME_SIZES)
def test_a_zero_image_has_orientation_zero(C, H, W):
    """every response is 0: the first maximum stays"""
    got = _maps(C, np.zeros((2, H, W), np.uint8), H, W)
    assert got.shape == (2, 4, H, W) and not got.any()


@pytest.mark.parametrize('H,W', S.CONSTANT_SIZES)
def test_a_constant_image_has_orientation_zero(C, H, W):
    """Radices 4 and 2 only: the butterflies subtract equal values and every non-DC bin is exactly zero.  At DC (the bank's sample
    next to the origin on an even frame) only orientation 0 of a scale has a coefficient above 0, at most 8e-12: the response is
    the same number at every pixel, 0 for the orientations 1 to 5, so orientation 0 holds the first maximum either way."""
    dc = S.bank(H, W)[:, 0, 0].astype(np.float32).reshape(4, 6)
    assert not dc[:, 1:].any() and dc.max() <= 8e-12
    x = np.stack([np.full((H, W), v, np.uint8) for v in (200, 255, 1)])
    spec = C.fft2d(torch.from_numpy(x.astype(np.complex64)).to(DEV)).cpu().numpy()
    assert np.array_equal(spec[:, 0, 0], np.array([200, 255, 1], np.complex64) * (H * W))
    spec[:, 0, 0] = 0
    assert not spec.any()
    assert not _maps(C, x, H, W).any()


# ---- e. batches in several chunks ----

@pytest.fixture(scope='module')
def alone(C):
    """the maps of the 9 batch frames, each run alone"""
    H, W = S.BATCH_FRAME
    return np.concatenate([_maps(C, u8[None], H, W) for u8 in S.batch_u8()])


def test_a_batch_of_nine_equals_its_frames_alone(C, alone):
    """chunks of 4, 4 and 1 through a workspace of 4 images"""
    H, W = S.BATCH_FRAME
    assert not np.array_equal(alone[0], alone[3]) and len({a.tobytes() for a in alone}) == 9
    got = _maps(C, S.batch_u8(), H, W)
    for b in range(9):
        assert np.array_equal(got[b], alone[b]), b


def _orientation_through(u8, images, short=0):
    """mp_lghd_orientation with a workspace of `images` images less `short` bytes: (return code, maps, message)"""
    from multipoint_amd import _lib
    B, H, W = u8.shape
    dev = _lib.require_cuda(DEV)
    h = _lib.get_handle(dev)
    nbytes = images * S.image_bytes(H, W) - short
    ws = torch.empty((images * S.image_bytes(H, W),), dtype=torch.uint8, device=dev)
    out = torch.full((B, 4, H, W), 99, dtype=torch.uint8, device=dev)
    t = torch.from_numpy(u8).to(dev)
    with torch.cuda.device(dev):
        rc = h.lib.mp_lghd_orientation(h.ptr, _lib.ptr(t), _lib.ptr(_gpu_bank(H, W)), B, H, W, _lib.ptr(out), _lib.ptr(ws), nbytes,
                                       _lib.stream_ptr(dev))
    torch.cuda.synchronize(dev)
    return rc, out.cpu().numpy(), (h.lib.mp_last_error(h.ptr) or b'').decode()


def test_small_workspaces_give_the_same_bytes(alone):
    """B = 3 one image at a time, B = 5 in chunks of 2, 2 and 1"""
    H, W = S.BATCH_FRAME
    nbytes = ctypes.c_longlong(0)
    from multipoint_amd import _lib
    assert _lib.load_library().mp_lghd_workspace_bytes(1, H, W, ctypes.byref(nbytes)) == 0 and nbytes.value == S.image_bytes(H, W)
    rc, three, _ = _orientation_through(S.batch_u8()[:3], 1)
    assert rc == 0 and np.array_equal(three, alone[:3])
    rc, five, _ = _orientation_through(S.batch_u8()[:5], 2)
    assert rc == 0 and np.array_equal(five, alone[:5])
    assert np.array_equal(five[:3], three)


def test_a_workspace_one_byte_short_is_refused():
    rc, out, msg = _orientation_through(S.batch_u8()[:3], 1, short=1)
    assert rc == -1                                         # MP_EINVAL
    assert 'one image needs %d B' % S.image_bytes(*S.BATCH_FRAME) in msg
    assert np.all(out == 99)                                # nothing ran


# ---- f. descriptors of a ragged batch ----

def test_describe_a_ragged_batch(C):
    H, W = S.BATCH_FRAME
    K = S.DESCRIBE_K
    ori = C.orientation_maps(torch.from_numpy(S.batch_u8()[:3]).to(DEV), _gpu_bank(H, W))
    lists = S.describe_lists()
    kp_t = torch.from_numpy(lists).to(DEV)
    cnt = torch.tensor(S.DESCRIBE_COUNTS, dtype=torch.int32, device=DEV)
    raw = C.describe(ori, kp_t, cnt, raw=True).cpu().numpy()
    unit = C.describe(ori, kp_t, cnt).cpu().numpy()
    assert raw.shape == unit.shape == (3, K, 384)
    maps = ori.cpu().numpy()
    zero_rows = 0
    for b, n in enumerate(S.DESCRIBE_COUNTS):
        n = min(n, K)
        want = np.zeros((K, 384))
        for k in range(n):
            y, x = lists[b, k]
            if S.patch_inside(y, x):
                want[k] = R.patch_descriptors(maps[b], lists[b, k:k + 1])[0]
        assert np.array_equal(raw[b].astype(np.float64), want), b
        assert np.abs(unit[b] - R.unit_rows(want)).max() <= 1e-6
        empty = ~want.any(1)
        assert not raw[b][empty].any() and not unit[b][empty].any()           # outside the frame or beyond the count: zeros
        assert not raw[b, n:].any() and not unit[b, n:].any()
        zero_rows += empty.sum()
    assert zero_rows == 3 + 11 + 4 and np.all(raw[0].sum(1)[[0, 2, 3]] == 4 * 1600)


# ---- g. FAST around the 64 x 4 block ----

@pytest.mark.parametrize('H,W', S.FAST_FRAMES)
def test_fast_on_frames_around_a_block(C, H, W):
    u8 = S.fast_frame(H, W)
    ws = R.fast_scores(u8)
    wc = R.fast_corners(ws)
    score, corners, prob = C.fast_detect(torch.from_numpy(u8[None]).to(DEV))
    assert np.array_equal(score[0].cpu().numpy().astype(np.int32), ws)
    assert np.array_equal(corners[0].cpu().numpy().astype(bool), wc)
    assert not prob.any()                                    # no 40 x 40 patch fits
    tested = max(H - 6, 0) * max(W - 6, 0)
    assert tested == {(7, 7): 1, (6, 40): 0, (40, 6): 0, (9, 65): 177, (13, 129): 861, (5, 64): 0}[H, W]
    assert (ws > 0).sum() <= tested and (tested < 100 or wc.sum() > 0)
