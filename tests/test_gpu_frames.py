"""GPU: the frame preparation (csrc/frames.hip, multipoint_amd.utils.frames) against the numpy restatement
tests/frames_restatement.py, bit for bit -- integers equal, fp32 equal as bits -- and prepare_frames against
tests/golden/frames.npz, the reference's own preprocess_images."""
import ctypes
import os

import numpy as np
import pytest
import torch

import frames_restatement as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
# (batch, H, W): one block; odd sizes that are a multiple of nothing; one row and one column (taps leave the frame on both
# sides); several blocks in a batch of 3; blocks that hold the end of one frame and the start of the next (frames of 9 pixels:
# many per block)
UNDISTORT_SHAPES = [(1, 24, 32), (1, 37, 53), (1, 1, 9), (1, 9, 1), (3, 64, 80), (3, 37, 53), (40, 1, 9)]


@pytest.fixture(scope='module')
def F():
    from multipoint_amd.utils import frames
    return frames


def _u16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _new_matrices(K, D, H, W):
    """[(name, K_new)]: alpha 0 and 1 where the frame has two dimensions, and one matrix that pushes a third of the frame
    outside (border 0 on two sides)"""
    out = []
    if H > 1 and W > 1:
        out += [('alpha%d' % a, R.optimal_new_camera_matrix(K, D, (W, H), a)) for a in (0, 1)]
    shifted = K.copy()
    shifted[0, 0], shifted[1, 1] = 0.8 * K[0, 0], 0.8 * K[1, 1]
    shifted[0, 2], shifted[1, 2] = K[0, 2] + W / 3.0, K[1, 2] - H / 3.0
    return out + [('third_outside', shifted)]


@pytest.mark.parametrize('shape', UNDISTORT_SHAPES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('D', R.DISTORTIONS, ids=['d0', 'barrel4', 'pincushion5'])
def test_undistort_is_the_restatements(F, shape, D):
    B, H, W = shape
    K = R.test_camera(H, W)
    bgr = np.stack([R.noise_bgr8(10 * H + b, H, W) if b else R.smooth_bgr8(H, H, W) for b in range(B)])
    u16 = np.stack([R.noise_u16(20 * H + b, H, W) if b else R.thermal_u16(W, H, W) for b in range(B)])
    d_bgr, d_u16 = torch.from_numpy(bgr).to(DEV), torch.from_numpy(u16.view(np.int16)).to(DEV).view(torch.uint16)
    for name, K_new in _new_matrices(K, D, H, W):
        for rotate in (False, True):
            got = F.undistort(d_bgr, K, D, K_new, rotate180=rotate).cpu().numpy()
            got16 = _u16(F.undistort(d_u16, K, D, K_new, rotate180=rotate))
            for b in range(B):
                assert np.array_equal(got[b], R.undistort(bgr[b], K, D, K_new, rotate)), (name, rotate, b)
                assert np.array_equal(got16[b], R.undistort(u16[b], K, D, K_new, rotate)), (name, rotate, b)
        if name == 'third_outside' and H > 1 and W > 1:
            assert (R.undistort(u16[0], K, D, K_new) == 0).mean() > 0.2           # (the border is really in the picture)
    if not any(D):
        assert torch.equal(F.undistort(d_bgr, K, D, K), d_bgr)                     # the identity map copies
        assert np.array_equal(_u16(F.undistort(d_u16, K, D, K, rotate180=True)), u16[:, ::-1, ::-1])
    # one frame without the batch axis, and a numpy input
    assert torch.equal(F.undistort(d_bgr[0], K, D, K), F.undistort(d_bgr, K, D, K)[0])
    assert np.array_equal(_u16(F.undistort(u16[0], K, D, K)), _u16(F.undistort(d_u16, K, D, K)[0]))


@pytest.mark.parametrize('case', [(36, 52, 24, 34), (37, 53, 24, 34), (24, 32, 24, 32), (9, 7, 3, 2), (64, 80, 30, 41)],
                         ids=lambda c: '%dx%d_to_%dx%d' % c)
def test_resize_is_the_restatements(F, case):
    H, W, oh, ow = case
    x = np.stack([R.smooth_bgr8(1, H, W), R.noise_bgr8(2, H, W), R.noise_bgr8(3, H, W)])
    got = F.resize_bgr8(torch.from_numpy(x).to(DEV), (oh, ow)).cpu().numpy()
    assert got.shape == (3, oh, ow, 3)
    for b in range(3):
        assert np.array_equal(got[b], R.resize_bgr8(x[b], (oh, ow))), b
    if (H, W) == (oh, ow):
        assert np.array_equal(got, x)
    assert np.array_equal(F.resize_bgr8(x[1], (oh, ow)).cpu().numpy(), got[1])


def _check_rescale(F, frames, rejection):
    got = F.thermal_rescale(torch.from_numpy(np.stack(frames).view(np.int16)).to(DEV).view(torch.uint16), rejection)
    raw, rescaled, saved = _u16(got[0]), got[1].cpu().numpy(), _u16(got[2])
    for b, x in enumerate(frames):
        want = R.thermal_rescale(x, rejection)
        assert np.array_equal(raw[b], want[0]), b
        assert np.array_equal(_bits(rescaled[b]), _bits(want[1])), b
        assert np.array_equal(saved[b], want[2]), b


@pytest.mark.parametrize('rejection', [True, False], ids=['rejection', 'plain'])
@pytest.mark.parametrize('name', ['fractional_bounds', 'constant', 'rank_on_element', 'noise_33x47', 'all_65535'])
def test_rescale_is_the_restatements(F, name, rejection):
    _check_rescale(F, [R.rescale_cases()[name]], rejection)


@pytest.mark.parametrize('rejection', [True, False], ids=['rejection', 'plain'])
@pytest.mark.parametrize('shape', [(33, 47), (64, 80), (1, 9), (130, 256)], ids=lambda s: '%dx%d' % s)
def test_rescale_batch_with_different_bounds(F, shape, rejection):
    """every image of a batch gets its own bounds: thermal frames at different temperatures, noise, a constant frame, a frame
    of two values; 33 x 47 and 1 x 9 run the one-pixel path, 64 x 80 and 130 x 256 (more than one block per image) the
    eight-pixel one"""
    H, W = shape
    two = np.where(R.noise_u16(9, H, W) > 600, 40000, 39999).astype(np.uint16)
    frames = [R.thermal_u16(1, H, W), R.thermal_u16(2, H, W, base=12000, span=300), R.noise_u16(3, H, W),
              np.full((H, W), 777, np.uint16), two, R.thermal_u16(4, H, W, base=60000, span=5000, outliers=0.2)]
    _check_rescale(F, frames, rejection)
    # the input is not modified, one frame comes back without the batch axis
    x = torch.from_numpy(frames[0].view(np.int16)).to(DEV).view(torch.uint16)
    raw, rescaled, saved = F.thermal_rescale(x, rejection)
    assert np.array_equal(_u16(x), frames[0]) and raw.shape == (H, W) and rescaled.dtype == torch.float32


def test_prepare_frames_is_the_references(F):
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'frames.npz'))
    for name in z['case_names']:
        optical, thermal, params, calibration, want = R.golden_case(z, str(name))
        # a batch of two: the golden pair and a second one, which must not disturb it
        o2, t2 = R.noise_bgr8(5, *optical.shape[:2]), R.thermal_u16(6, *thermal.shape, base=9000)
        got = F.prepare_frames(np.stack([optical, o2]), np.stack([thermal, t2]), params, calibration, return_saved=True)
        assert np.array_equal(got[0][0].cpu().numpy(), want[0])
        assert np.array_equal(_u16(got[1])[0], want[1])
        assert np.array_equal(_bits(got[2][0].cpu().numpy()), _bits(want[2]))
        assert np.array_equal(_u16(got[3])[0], R.saved_u16(want[2]))
        second = R.prepare_frames(o2, t2, params, calibration)
        assert np.array_equal(got[0][1].cpu().numpy(), second[0]) and np.array_equal(_u16(got[1])[1], second[1])
        assert np.array_equal(_bits(got[2][1].cpu().numpy()), _bits(second[2]))


@pytest.mark.parametrize('undistort', [False, True])
@pytest.mark.parametrize('rotate', [False, True])
def test_prepare_frames_switches(F, undistort, rotate):
    """every combination of the switches against the restatement's sequence, without outlier rejection too (where the
    reference raises NameError): a plain min-max rescale of the unclipped frame"""
    optical, thermal = R.smooth_bgr8(3, 30, 44), R.thermal_u16(4, 20, 26)
    calibration = R.calibration_of([('thermal', R.DISTORTIONS[1]), ('optical', R.DISTORTIONS[2])], (30, 44), (20, 26))
    for downscale, rejection in [(True, True), (False, False)]:
        params = {'undistort_images': undistort, 'image/undistort_alpha': 0.5, 'image/thermal/rotate': rotate,
                  'image/optical/downscale': downscale, 'image/thermal/rescale_outlier_rejection': rejection}
        got = F.prepare_frames(optical[None], thermal[None], params, calibration if undistort else None)
        want = R.prepare_frames(optical, thermal, params, calibration)
        assert np.array_equal(got[0][0].cpu().numpy(), want[0]) and np.array_equal(_u16(got[1])[0], want[1])
        assert np.array_equal(_bits(got[2][0].cpu().numpy()), _bits(want[2]))
        if not rejection:
            assert np.array_equal(want[1], R.undistort(thermal, *_thermal_camera(calibration, thermal, 0.5), rotate) if undistort
                                  else (thermal[::-1, ::-1] if rotate else thermal))


def _thermal_camera(calibration, thermal, alpha):
    from multipoint_amd.utils.frames import camera_from_calibration
    K, D = camera_from_calibration(calibration, 'thermal')
    return K, D, R.optimal_new_camera_matrix(K, D, thermal.shape[::-1], alpha)


def test_error_paths(F):
    from multipoint_amd import _lib
    K = R.test_camera(8, 12)
    bgr = torch.zeros((2, 8, 12, 3), dtype=torch.uint8, device=DEV)
    u16 = torch.zeros((2, 8, 12), dtype=torch.int16, device=DEV).view(torch.uint16)
    with pytest.raises(ValueError, match='4 or 5 distortion coefficients'):
        F.undistort(bgr, K, np.zeros(6), K)                                        # five plus one
    with pytest.raises(ValueError, match='4 or 5 distortion coefficients'):
        F.undistort(u16, K, np.zeros(3), K)
    with pytest.raises(ValueError):
        F.undistort(bgr, K, np.zeros(4), np.diag([0.0, 1.0, 1.0]))                 # a zero focal length in K_new
    with pytest.raises(ValueError):
        F.undistort(bgr, K, (np.nan, 0, 0, 0), K)
    with pytest.raises(RuntimeError, match='GPU only'):
        F.undistort(torch.zeros((2, 8, 12, 3), dtype=torch.uint8), K, np.zeros(4), K)          # a CPU tensor
    with pytest.raises(RuntimeError, match='GPU only'):
        F.thermal_rescale(torch.zeros((2, 8, 12), dtype=torch.int16).view(torch.uint16))
    with pytest.raises(ValueError):
        F.undistort(torch.zeros((2, 8, 12), dtype=torch.float32, device=DEV), K, np.zeros(4), K)
    with pytest.raises(ValueError):
        F.resize_bgr8(u16, (4, 4))
    with pytest.raises(ValueError):
        F.resize_bgr8(bgr, (0, 4))
    with pytest.raises(ValueError):
        F.thermal_rescale(bgr)
    params = {'undistort_images': False, 'image/undistort_alpha': 0.0, 'image/thermal/rotate': True,
              'image/optical/downscale': True, 'image/thermal/rescale_outlier_rejection': True}
    with pytest.raises(ValueError, match='2 optical frames and 1 thermal frames'):
        F.prepare_frames(bgr, u16[:1], params)                                     # mismatched batch sizes
    with pytest.raises(ValueError, match='needs the calibration'):
        F.prepare_frames(bgr, u16, dict(params, undistort_images=True))
    bad = R.calibration_of([('optical', R.DISTORTIONS[1]), ('lidar', R.DISTORTIONS[1])], (8, 12), (8, 12))
    with pytest.raises(ValueError, match='ERROR unknown camera label: lidar'):
        F.prepare_frames(bgr, u16, dict(params, undistort_images=True), bad)
    # the C ABI's own checks
    h = _lib.get_handle(bgr.device)
    out = torch.empty_like(u16)
    res = torch.empty((2, 8, 12), dtype=torch.float32, device=DEV)
    ws = torch.empty(64, dtype=torch.uint8, device=DEV)
    rc = h.lib.mp_thermal_rescale(h.ptr, _lib.ptr(u16), 2, 8, 12, 1, _lib.ptr(out), _lib.ptr(res), None, _lib.ptr(ws), 64, None)
    assert rc == -1 and b'workspace of 64 B' in h.lib.mp_last_error(h.ptr)
    rc = h.lib.mp_thermal_rescale(h.ptr, None, 2, 8, 12, 1, _lib.ptr(out), _lib.ptr(res), None, _lib.ptr(ws), 64, None)
    assert rc == -1 and h.lib.mp_last_error(h.ptr) == b'mp_thermal_rescale: NULL tensor'
    need = ctypes.c_longlong()
    assert h.lib.mp_thermal_rescale_workspace_bytes(0, ctypes.byref(need)) == -1
    assert h.lib.mp_thermal_rescale_workspace_bytes(2, ctypes.byref(need)) == 0 and need.value > 0
    rc = h.lib.mp_resize_bgr8(h.ptr, _lib.ptr(bgr), 2, 8, 12, 8, 12, _lib.ptr(bgr), None)
    assert rc == -1 and b'different buffers' in h.lib.mp_last_error(h.ptr)
    Kc = (ctypes.c_double * 9)(*K.reshape(-1))
    Dc = (ctypes.c_double * 5)()
    rc = h.lib.mp_undistort(h.ptr, _lib.ptr(bgr), _lib.MP_FRAMES_U8, 2, 8, 12, Kc, Dc, 4, Kc, 0, _lib.ptr(out), None)
    assert rc == -1 and b'dtype' in h.lib.mp_last_error(h.ptr)
    rc = h.lib.mp_undistort(h.ptr, _lib.ptr(bgr), _lib.MP_FRAMES_BGR8, 2, 8, 12, Kc, Dc, 4, Kc, 0, _lib.ptr(bgr), None)
    assert rc == -1 and b'different buffers' in h.lib.mp_last_error(h.ptr)
