"""GPU: the kernels of the RIFT baseline (csrc/fft.hip pc_rows_kernel and the AMP mode, csrc/rift.hip, the shared FAST and
patch-histogram kernels of csrc/lghd.hip) on the inputs of tests/rift_cases.py, whose premises
tests/test_rift_host.py checks without a device.  The numbered rules are the issue's:
  1  M and m against float64 within 8 float32-restatement errors of the same frame
  2  T bit for bit from the exact median of the amplitude plane the GPU returned; against float64 within 8 float32 errors
  3  the maximum index map equals the float64 arg-max wherever the float64 top-two gap is at least 16 float32 errors of sumA
  4  u8m, FAST and prob bit-exact against numpy on the GPU's own M
  5  descriptor counts bit-exact against numpy on the GPU's own map, unit rows within 1e-6, the zero padding
  6  batches and workspace chunking byte for byte the maps of each frame alone
  7  refusals

Measured on the MI355X: see the docstrings of the tests."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import lghd_restatement as L
import rift_cases as C
import rift_restatement as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MAP_NAMES = [im[0] for im in C.MAP_FRAMES]
EINVAL = -1          # MP_EINVAL of include/multipoint_hip.h


@pytest.fixture(scope='module')
def D():
    from multipoint_amd.models import classic_detectors
    return classic_detectors


@functools.lru_cache(maxsize=None)
def _bank(H, W):
    return torch.from_numpy(L.filter_bank(H, W).astype(np.float32)).to(DEV)


_gpu_cache = {}


def _gpu_maps(D, name):
    """the GPU's (M, m, mim, T, amp) of one map frame as numpy arrays, computed once"""
    if name not in _gpu_cache:
        u8 = C.map_frame(name)
        out = D.phase_congruency(torch.from_numpy(u8)[None].to(DEV), _bank(*u8.shape), want_amplitudes=True)
        _gpu_cache[name] = tuple(t[0].cpu().numpy() for t in out)
    return _gpu_cache[name]


# ---- 1. M and m ----

@pytest.mark.parametrize('name', MAP_NAMES)
def test_moments_against_float64(D, name):
    """Measured ratios (GPU error / float32-restatement error), M and m: see DESIGN.md 3.26."""
    f64, f32 = C.restated_maps(name)
    M, m = _gpu_maps(D, name)[:2]
    for key, got in (('M', M), ('m', m)):
        err, err32 = np.abs(got - f64[key]).max(), np.abs(f32[key] - f64[key]).max()
        print('%s %s: gpu %.3g, float32 restatement %.3g, ratio %.2f, range %.3g' % (name, key, err, err32, err / err32, np.ptp(f64[key])))
        assert err <= 8 * err32


# ---- 2. T ----

@pytest.mark.parametrize('name', MAP_NAMES)
def test_noise_thresholds(D, name):
    f64, f32 = C.restated_maps(name)
    T, amp = _gpu_maps(D, name)[3:]
    assert amp.dtype == np.float32 and T.dtype == np.float32 and (amp >= 0).all()
    want = np.array([np.float32(R.noise_threshold(amp[o])) for o in range(6)])
    assert np.array_equal(T, want)                                                     # bit for bit from the returned plane
    err, err32 = np.abs(T - f64['T']).max(), np.abs(f32['T'] - f64['T']).max()
    print('%s T: gpu %.3g, float32 restatement %.3g, ratio %.2f' % (name, err, err32, err / err32))
    assert err <= 8 * err32
    # the planes themselves, by the same rule
    err, err32 = np.abs(amp - f64['amp0']).max(), np.abs(f32['amp0'] - f64['amp0']).max()
    print('%s amp0: gpu %.3g, float32 restatement %.3g, ratio %.2f' % (name, err, err32, err / err32))
    assert err <= 8 * err32


def test_noise_threshold_other_k(D):
    """k is an argument: k = 0 and k = 2.5 from the same planes"""
    u8 = C.map_frame('smooth_48x80')
    for k in (0.0, 2.5):
        out = D.phase_congruency(torch.from_numpy(u8)[None].to(DEV), _bank(48, 80), k=k, want_amplitudes=True)
        T, amp = out[3][0].cpu().numpy(), out[4][0].cpu().numpy()
        assert np.array_equal(T, np.array([np.float32(R.noise_threshold(amp[o], k)) for o in range(6)]))


# ---- 3. the maximum index map ----

@pytest.mark.parametrize('name', MAP_NAMES)
def test_maximum_index_map(D, name):
    f64 = C.restated_maps(name)[0]
    amb = C.ambiguous(name)
    mim = _gpu_maps(D, name)[2]
    assert mim.dtype == np.uint8 and mim.max() <= 5
    print('%s: %d ambiguous pixels, %d of them differ' % (name, amb.sum(), (mim != f64['mim'])[amb].sum()))
    assert amb.mean() <= C.AMBIGUOUS_CAP
    assert np.array_equal(mim[~amb], f64['mim'][~amb])


@pytest.mark.parametrize('name', [c[0] for c in C.CONSTANT_FRAMES])
def test_constant_frames(D, name):
    """Every PC is 0: MIM exactly 0, T exactly 0, M = eps / 2 = the fp32 of 5e-5.  m = (cy2 + cx2 - d) / 2 with d = eps is -eps / 2:
    the issue's sentence "M = m = eps / 2" contradicts its own step 5 (and Kovesi's minimum moment); the formula is what is built."""
    u8 = C.constant_frame(name)
    M, m, mim, T = (t[0].cpu().numpy() for t in D.phase_congruency(torch.from_numpy(u8)[None].to(DEV), _bank(*u8.shape)))
    half = np.float32(R.EPS) / np.float32(2)
    assert half == np.float32(5e-5)
    assert not mim.any() and not T.any()
    assert np.all(M == half) and np.all(m == -half)
    # FAST on a constant map: u8m all zero, no corner
    u8m, score, corners, prob = D.rift_detect(torch.from_numpy(M)[None].to(DEV), 6, 24)
    assert not u8m.any() and not score.any() and not corners.any() and not prob.any()


# ---- 4. u8m, FAST, prob ----

def _check_detect(D, M, thr, patch):
    M = np.ascontiguousarray(M, np.float32)
    u8m, score, corners, prob = (t[0].cpu().numpy() for t in D.rift_detect(torch.from_numpy(M)[None].to(DEV), thr, patch))
    w_u8m, w_score, w_corners, w_prob = R.detect(M, thr, patch)
    assert np.array_equal(u8m, w_u8m)
    assert np.array_equal(score, w_score) and np.array_equal(corners, w_corners.astype(np.uint8))
    assert prob.shape == (1,) + M.shape and prob.dtype == np.float32 and np.array_equal(prob[0], w_prob)
    return int((w_prob > 0).sum()), int(w_corners.sum())


@pytest.mark.parametrize('name', MAP_NAMES)
def test_detect_is_bit_exact(D, name):
    M = _gpu_maps(D, name)[0]
    H, W = M.shape
    for patch in (24, 48, 96):
        if patch <= min(H, W):
            for thr in (6, 13):
                n, c = _check_detect(D, M, thr, patch)
                print('%s patch %d threshold %d: %d corners, %d valid' % (name, patch, thr, c, n))


@pytest.mark.parametrize('shape', C.DETECT_FRAMES, ids=['x'.join(map(str, s)) for s in C.DETECT_FRAMES])
def test_detect_on_tiny_frames(D, shape):
    """detect alone: no interior (6 x 40, 40 x 6), a single interior pixel (7 x 7), a partial 64 x 4 block (9 x 65).  No patch fits,
    so prob is 0 everywhere; an isolated peak makes a corner where there is an interior"""
    M = np.random.default_rng(shape[0] * 100 + shape[1]).random(shape).astype(np.float32) * 0.1
    if min(shape) >= 7:
        M[3, 3] = 1.0
    n, c = _check_detect(D, M, 13, 24)
    assert n == 0 and (c >= 1) == (min(shape) >= 7)


def test_detect_batch_has_per_image_ranges(D):
    """each image of a batch is stretched by its own minimum and maximum"""
    Ms = np.stack([_gpu_maps(D, 'smooth_64x64')[0], _gpu_maps(D, 'noise_64x64')[0], np.full((64, 64), 0.25, np.float32)])
    u8m, score, corners, prob = (t.cpu().numpy() for t in D.rift_detect(torch.from_numpy(Ms).to(DEV), 6, 24))
    for b in range(3):
        w = R.detect(Ms[b], 6, 24)
        assert np.array_equal(u8m[b], w[0]) and np.array_equal(score[b], w[1]) and np.array_equal(prob[b, 0], w[3])
    assert not u8m[2].any()


# ---- 5. describe ----

def _border_keypoints(H, W, patch, n, seed):
    """n keypoints inside the validity border, the first four exactly on its limits"""
    b = patch // 2
    rng = np.random.default_rng(seed)
    kp = np.stack([rng.integers(b, H - b + 1, n), rng.integers(b, W - b + 1, n)], 1)
    kp[:4] = [(b, b), (b, W - b), (H - b, b), (H - b, W - b)]
    return kp.astype(np.int32)


@pytest.mark.parametrize('patch', (24, 48, 96))
def test_describe_ragged_batch(D, patch):
    """B = 3 with counts (11, 0, 25) at K = 25, keypoints on the border limits, the GPU's own maps of three frames"""
    names = {24: ('smooth_96x128',) * 3, 48: ('smooth_96x128',) * 3, 96: ('smooth_160x192',) * 3}[patch]
    mim = np.stack([_gpu_maps(D, n)[2] for n in names])
    mim[1] = (mim[1] + 1) % 6
    mim[2] = mim[2][::-1, ::-1]
    _, H, W = mim.shape
    K, counts = 25, (11, 0, 25)
    kp = np.stack([_border_keypoints(H, W, patch, K, 7 + b) for b in range(3)])
    args = (torch.from_numpy(np.ascontiguousarray(mim)).to(DEV), torch.from_numpy(kp).to(DEV), torch.tensor(counts, dtype=torch.int32))
    raw = D.rift_describe(*args, patch_size=patch, raw=True).cpu().numpy()
    unit = D.rift_describe(*args, patch_size=patch).cpu().numpy()
    assert raw.shape == unit.shape == (3, K, 256)
    for b, n in enumerate(counts):
        want = R.descriptors(mim[b], kp[b, :n], patch)
        assert np.array_equal(raw[b, :n, :216], want)                                   # exact counts
        assert (want.sum(1) == patch * patch).all()
        assert np.abs(unit[b, :n, :216] - L.unit_rows(want)).max(initial=0) <= 1e-6
        assert not raw[b, n:].any() and not unit[b, n:].any()                           # rows beyond the count
        assert not raw[b, :, 216:].any() and not unit[b, :, 216:].any()                 # the padding: exactly 0


def test_describe_patch_outside_the_frame_is_zero(D):
    mim = torch.from_numpy(_gpu_maps(D, 'smooth_64x64')[2])[None].to(DEV)
    kp = torch.tensor([[[11, 30], [30, 53], [12, 12], [52, 52]]], dtype=torch.int32)
    raw = D.rift_describe(mim, kp, torch.tensor([4], dtype=torch.int32), patch_size=24, raw=True).cpu().numpy()[0]
    assert not raw[0].any() and not raw[1].any() and raw[2].sum() == 576 and raw[3].sum() == 576


# ---- 6. batches and chunking ----

def test_batch_and_workspace_chunking(D):
    """B = 5 through workspaces of one and of two images, and through the wrapper's own: byte for byte each frame alone"""
    from multipoint_amd import _lib
    H, W = 48, 80
    frames = [C.map_frame('noise_48x80'), C.map_frame('smooth_48x80'), C.constant_frame('zero_48x80'),
              255 - C.map_frame('smooth_48x80'), C.map_frame('noise_48x80')[::-1].copy()]
    u8 = torch.from_numpy(np.stack(frames)).to(DEV)
    bank = _bank(H, W)
    alone = [[t.cpu().numpy() for t in D.phase_congruency(u8[b:b + 1], bank, want_amplitudes=True)] for b in range(5)]
    whole = [t.cpu().numpy() for t in D.phase_congruency(u8, bank, want_amplitudes=True)]
    for b in range(5):
        for a, w in zip(alone[b], whole):
            assert a[0].tobytes() == w[b].tobytes()
    h = _lib.get_handle(torch.device(DEV, torch.cuda.current_device()))
    one = ctypes.c_longlong(0)
    h.check(h.lib.mp_rift_workspace_bytes(1, H, W, ctypes.byref(one)))
    assert one.value == 224 * H * W

    def run(nbytes, with_amp=True):
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
        M = torch.full((5, H, W), -1.0, device=DEV)
        m = torch.full((5, H, W), -1.0, device=DEV)
        mim = torch.full((5, H, W), 9, dtype=torch.uint8, device=DEV)
        T = torch.full((5, 6), -1.0, device=DEV)
        amp = torch.full((5, 6, H, W), -1.0, device=DEV) if with_amp else None
        rc = h.lib.mp_phase_congruency(h.ptr, _lib.ptr(u8), _lib.ptr(bank), 5, H, W, 1.0, 3.0, 0.5, _lib.ptr(M), _lib.ptr(m), _lib.ptr(mim),
                                       _lib.ptr(T), _lib.ptr(amp), _lib.ptr(ws), nbytes, _lib.stream_ptr(torch.device(DEV, 0)))
        torch.cuda.synchronize()
        return rc, [t.cpu().numpy() for t in (M, m, mim, T)] + ([amp.cpu().numpy()] if with_amp else [])

    for images in (1, 2):
        rc, got = run(images * one.value)
        assert rc == _lib.MP_OK
        for g, w in zip(got, whole):
            assert g.tobytes() == w.tobytes()
    rc, got = run(2 * one.value + 17, with_amp=False)          # the amplitude planes stay in the workspace
    assert rc == _lib.MP_OK and all(g.tobytes() == w.tobytes() for g, w in zip(got, whole))
    rc, got = run(one.value - 1)
    assert rc == EINVAL and (got[0] == -1).all() and (got[2] == 9).all()           # refused before any launch


# ---- 7. refusals ----

def test_refusals(D):
    from multipoint_amd import _lib
    from multipoint_amd.models import ClassicDetectors
    with pytest.raises(ValueError):
        D.phase_congruency(torch.zeros((1, 56, 70), dtype=torch.uint8, device=DEV), torch.zeros((24, 56, 70), device=DEV))       # 7 | 56
    nbytes = ctypes.c_longlong(0)
    h = _lib.get_handle(torch.device(DEV, torch.cuda.current_device()))
    assert h.lib.mp_rift_workspace_bytes(1, 56, 70, ctypes.byref(nbytes)) == EINVAL
    M = torch.rand((1, 64, 64), device=DEV)
    mim = torch.zeros((1, 64, 64), dtype=torch.uint8, device=DEV)
    kp, cnt = torch.tensor([[[32, 32]]], dtype=torch.int32), torch.tensor([1], dtype=torch.int32)
    for patch in (0, -12, 20, 50, 168):                        # no multiple of 12, not positive, above the cap of 156
        with pytest.raises(Exception, match='patch_size'):
            D.rift_detect(M, 13, patch)
        with pytest.raises(Exception, match='patch_size'):
            D.rift_describe(mim, kp, cnt, patch_size=patch)
        with pytest.raises(ValueError, match='patch_size'):
            ClassicDetectors({'method': 'RIFT', 'patch_size': patch})
    for thr in (0, 256):
        with pytest.raises(Exception, match='fast_threshold'):
            D.rift_detect(M, thr, 24)
    with pytest.raises(Exception, match='holds no patch'):   # a patch larger than the frame
        D.rift_describe(mim, kp, cnt, patch_size=96)
    model = ClassicDetectors({'method': 'RIFT', 'patch_size': 96}).to(DEV)
    with pytest.raises(ValueError, match='holds no patch'):
        model({'image': torch.zeros((1, 1, 64, 64), device=DEV)})
    with pytest.raises(ValueError):
        model({'image': torch.zeros((1, 1, 112, 112), device=DEV)})             # 7 | 112: no FFT length
