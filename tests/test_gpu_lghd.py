"""GPU: the LGHD kernels (csrc/lghd.hip, csrc/fft.hip) behind multipoint_amd.models.classic_detectors against the numpy
restatement tests/lghd_restatement.py: quantisation and FAST bit for bit, the FFT against np.fft in float64 within 8 float32
np.fft errors, the orientation maps wherever float64 decides them by more than 16 such errors, exact patch histograms."""
import functools

import numpy as np
import pytest
import torch

import lghd_restatement as R
from lghd_shape_cases import check_orientation

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def C():
    from multipoint_amd.models import classic_detectors
    return classic_detectors


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(image float32, u8, bank float64, float64 magnitudes, err32, float64 orientation maps) of a committed test image; computed once"""
    _, kind, seed, H, W = next(i for i in R.IMAGES if i[0] == name)
    image = R.make_image(kind, seed, H, W)
    u8 = R.quantize(image)
    bank = R.filter_bank(H, W)
    m64 = R.responses(u8, bank)
    err32 = np.abs(R.responses(u8, bank, single=True) - m64).max()
    return image, u8, bank, m64, err32, R.orientation_maps(m64)


# ---- 1. quantisation + FAST ----

def _detect_inputs():
    rng = np.random.default_rng(5)
    ramp = rng.random((16, 256)).astype(np.float32)
    ramp[0] = (np.arange(256) / 255.0).astype(np.float32)            # every k / 255: the fp32 product may land below k
    ramp[5:12] = (rng.integers(0, 256, (7, 256)) / 255.0).astype(np.float32)
    odd = (rng.integers(0, 256, (37, 131)) / 255.0).astype(np.float32)
    return [ramp[None], odd[None], np.stack([R.make_image(k, s, 48, 80) for k, s in (('noise', 11), ('smooth', 12), ('noise', 21))]),
            R.make_image('noise', 15, 96, 120)[None]]


@pytest.mark.parametrize('case', range(4))
def test_quantisation_and_fast_are_bit_exact(C, case):
    from multipoint_amd.utils import utils as U
    images = _detect_inputs()[case]
    B, H, W = images.shape
    t = torch.from_numpy(images).to(DEV)
    u8 = C.quantize(t)
    want_u8 = R.quantize(images)
    assert np.array_equal(u8.cpu().numpy(), want_u8)
    score, corners, prob = C.fast_detect(u8)
    kp, _, cnt = U.extract_keypoints(prob, 0.5)
    for b in range(B):
        ws = R.fast_scores(want_u8[b])
        wc = R.fast_corners(ws)
        assert np.array_equal(score[b].cpu().numpy().astype(np.int32), ws)
        assert np.array_equal(corners[b].cpu().numpy().astype(bool), wc)
        assert wc.sum() > 20
        valid = R.valid_keypoints(np.argwhere(wc), H, W)
        n = int(cnt[b])
        assert n == len(valid)
        assert np.array_equal(kp[b, :n].cpu().numpy().astype(np.int64), valid)              # row-major order
        pm = prob[b, 0].cpu().numpy()
        assert set(np.unique(pm)) <= {0.0, 1.0} and np.array_equal(np.argwhere(pm == 1.0), valid)


def test_fast_hand_made_patterns(C):
    """the patterns of tests/test_lghd_host.py on the kernel: arcs of 9 and 8, a wrapping arc, a difference of exactly 10, equal
    neighbours, the first and last tested rows"""
    def pattern(p, ring, at):
        im = np.full((14, 80), p, np.uint8)
        for (dx, dy), v in zip(R.CIRCLE, ring):
            im[at[0] + dy, at[1] + dx] = v
        return im
    wrap = [100] * 16
    for i in (12, 13, 14, 15, 0, 1, 2, 3, 4):
        wrap[i] = 150
    frames = [pattern(100, [200] * 9 + [100] * 7, (3, 10)), pattern(100, [200] * 8 + [100] * 8, (6, 10)),
              pattern(100, wrap, (10, 70)), pattern(100, [110] * 9 + [100] * 7, (6, 40)), pattern(100, [89] * 9 + [100] * 7, (10, 3)),
              pattern(100, [200] * 9 + [100] * 7, (10, 76))]
    flat = np.full((14, 80), 100, np.uint8)               # two equal scores side by side
    flat[4:9, 20:27] = np.array([[100, 100, 200, 200, 200, 100, 100]] * 5)
    frames.append(flat)
    u8 = torch.from_numpy(np.stack(frames)).to(DEV)
    score, corners, _ = C.fast_detect(u8, want_prob=False)
    score, corners = score.cpu().numpy().astype(np.int32), corners.cpu().numpy().astype(bool)
    for b, f in enumerate(frames):
        ws = R.fast_scores(f)
        assert np.array_equal(score[b], ws) and np.array_equal(corners[b], R.fast_corners(ws))
    assert score[0][3, 10] == 99 and corners[0][3, 10]
    assert score[1][6, 10] == 0 and score[2][10, 70] == 49 and score[3][6, 40] == 0 and score[4][10, 3] == 10
    assert score[5][10, 76] == 99 and corners[5][10, 76]


# ---- 2. FFT ----

def _fft_case(C, x, axes, inverse):
    """max |gpu - float64| and max |np.fft float32 - float64| of one transform, both relative to the largest float64 magnitude"""
    ax = {1: (-1,), 2: (-2,), 3: (-2, -1)}[axes]
    f = (lambda a: np.fft.ifftn(a, axes=ax, norm='forward')) if inverse else (lambda a: np.fft.fftn(a, axes=ax))
    want = f(x.astype(np.complex128))
    single = f(x)
    assert single.dtype == np.complex64
    got = C.fft2d(torch.from_numpy(x).to(DEV), inverse=inverse, axes=axes).cpu().numpy()
    top = np.abs(want).max()
    return np.abs(got - want).max() / top, np.abs(single - want).max() / top


@pytest.mark.parametrize('n', [48, 64, 80, 96, 120, 512, 640])
def test_fft_lines(C, n):
    """forward and inverse, along rows (one line per workgroup) and along columns (20 columns: bundles of 16, or of 8 at n = 640,
    the last one partial)"""
    rng = np.random.default_rng(n)
    for axes, shape in ((1, (2, 5, n)), (2, (2, n, 20))):
        x = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
        for inverse in (False, True):
            err, err32 = _fft_case(C, x, axes, inverse)
            print('n = %d axes %d inverse %d: gpu %.3g, np.fft float32 %.3g, ratio %.2f' % (n, axes, inverse, err, err32, err / err32))
            assert err <= 8 * err32


def test_fft_2d_512x640(C):
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((1, 512, 640)) + 1j * rng.standard_normal((1, 512, 640))).astype(np.complex64)
    for inverse in (False, True):
        err, err32 = _fft_case(C, x, 3, inverse)
        print('512 x 640 inverse %d: gpu %.3g, np.fft float32 %.3g, ratio %.2f' % (inverse, err, err32, err / err32))
        assert err <= 8 * err32


def test_fft_refuses_other_lengths(C):
    x = torch.zeros((1, 56, 64), dtype=torch.complex64, device=DEV)
    with pytest.raises(ValueError):
        C.fft2d(x, axes=2)
    C.fft2d(x, axes=1)                                    # 56 is not transformed
    with pytest.raises(ValueError):
        C.fft2d(torch.zeros((1, 8, 70), dtype=torch.complex64, device=DEV))


# ---- 3. orientation maps ----

def _check_orientation(got, name):
    """the rule of tests/lghd_shape_cases.py::check_orientation on a committed test image"""
    _, _, _, m64, err32, want = _reference(name)
    check_orientation(got, name, m64, err32, want)


@pytest.mark.parametrize('name', ['noise_64x64', 'smooth_64x64', 'noise_96x120', 'smooth_96x120'])
def test_orientation_maps(C, name):
    """Noise and low-passed noise only.  Piecewise-constant images are excluded on purpose: their far-field responses are rounding
    noise in float64 too, so 20 to 60 % of their pixels sit within a few float32 FFT errors of a tie and no arg-max is defined."""
    _, u8, bank, *_ = _reference(name)
    got = C.orientation_maps(torch.from_numpy(u8[None]).to(DEV), torch.from_numpy(bank.astype(np.float32)).to(DEV))
    assert got.shape == (1, 4) + u8.shape and got.dtype == torch.uint8
    _check_orientation(got[0].cpu().numpy(), name)


def test_orientation_maps_batch_of_three(C):
    names = ['noise_48x80', 'smooth_48x80', 'noise_48x80']
    u8 = np.stack([_reference(n)[1] for n in names])
    bank = torch.from_numpy(_reference(names[0])[2].astype(np.float32)).to(DEV)
    got = C.orientation_maps(torch.from_numpy(u8).to(DEV), bank).cpu().numpy()
    for b, n in enumerate(names):
        _check_orientation(got[b], n)
    assert np.array_equal(got[0], got[2])


# ---- 4. descriptors ----

@pytest.mark.parametrize('name', ['noise_48x80', 'smooth_64x64', 'noise_96x120'])
def test_descriptors_count_the_gpu_orientation_map(C, name):
    image, u8, bank, *_ = _reference(name)
    H, W = u8.shape
    ori = C.orientation_maps(torch.from_numpy(u8[None]).to(DEV), torch.from_numpy(bank.astype(np.float32)).to(DEV))
    fast = R.valid_keypoints(R.fast_keypoints(u8), H, W)
    edge = np.array([[20, 20], [20, W - 20], [H - 20, 20], [H - 20, W - 20], [20, W // 2], [H // 2, 20], [H - 20, W // 2],
                     [H // 2, W - 20]])
    kp = np.concatenate([edge, fast])
    n, K = len(kp), len(kp) + 3                               # K no multiple of anything; the last rows lie beyond the count
    lists = np.zeros((1, K, 2), np.int32)
    lists[0, :n] = kp
    lists[0, n:] = [H // 2, W // 2]
    kp_t, cnt = torch.from_numpy(lists).to(DEV), torch.tensor([n], dtype=torch.int32, device=DEV)
    raw = C.describe(ori, kp_t, cnt, raw=True)[0].cpu().numpy()
    unit = C.describe(ori, kp_t, cnt)[0].cpu().numpy()
    want = R.patch_descriptors(ori[0].cpu().numpy(), kp)
    assert np.array_equal(raw[:n].astype(np.float64), want)
    assert not raw[n:].any() and not unit[n:].any()
    assert np.abs(unit[:n] - R.unit_rows(want)).max() <= 1e-6


@pytest.mark.parametrize('name', ['noise_48x80', 'smooth_96x120'])
def test_dense_map_sampled_like_the_reference_equals_describe(C, name):
    """forward's dense [1,384,H,W] map through utils.interpolate_descriptors (the reference's route) against describe(): unit rows
    with components <= 1 and a handful of fp32 roundings each, 1e-6 is about 4 x over 2.4e-7"""
    from multipoint_amd.models import ClassicDetectors
    from multipoint_amd.utils import utils as U
    image, u8, *_ = _reference(name)
    H, W = u8.shape
    net = ClassicDetectors({'method': 'LGHD'}).to(DEV).eval()
    out = net({'image': torch.from_numpy(image)[None, None].to(DEV)})
    assert out['prob'].shape == (1, 1, H, W) and out['orientation'].shape == (1, 4, H, W) and out['desc'].shape == (1, 384, H, W)
    kp = torch.nonzero(out['prob'][0, 0] > 0)
    want_kp = R.valid_keypoints(R.fast_keypoints(u8), H, W)
    assert np.array_equal(kp.cpu().numpy(), want_kp)
    n = len(want_kp)
    sampled = U.interpolate_descriptors(kp, out['desc'][0], H, W).cpu().numpy()
    direct = net.describe(out, kp.reshape(1, n, 2).to(torch.int32), torch.tensor([n], dtype=torch.int32, device=DEV))[0].cpu().numpy()
    assert sampled.shape == direct.shape == (n, 384)
    assert np.abs(sampled - direct).max() <= 1e-6
    assert np.abs(np.linalg.norm(direct.astype(np.float64), axis=1) - 1).max() <= 1e-6


def test_model_surface(C):
    from multipoint_amd.models import ClassicDetectors
    for method in ('SIFT', 'SURF'):
        with pytest.raises(NotImplementedError):
            ClassicDetectors({'method': method})
    with pytest.raises(ValueError):
        ClassicDetectors({'method': 'ORB'})
    assert ClassicDetectors.default_config == {'method': 'SURF', 'prob_smoothing': False, 'smoothing_kernel_size': 5,
                                               'min_keypoints': 100, 'image_H': 512, 'image_W': 640}
    net = ClassicDetectors({'method': 'LGHD'})
    net.load_state_dict({})
    assert net.init_random_weights(3) is net and net.to(DEV) is net and net.eval() is net
    with pytest.raises(ValueError):
        net({'image': torch.zeros((1, 1, 56, 70), device=DEV)})                # 7 divides both sizes
    flat = net({'image': torch.full((1, 1, 48, 64), 0.5, device=DEV)})          # no keypoint: the reference's [1,1,H,W] zeros
    assert flat['desc'].shape == (1, 1, 48, 64) and not flat['desc'].any() and not flat['prob'].any()
    with pytest.raises(ValueError):
        ClassicDetectors({'method': 'LGHD', 'image_H': 512, 'image_W': 640})({'image': torch.zeros((1, 1, 48, 64), device=DEV)})
    # B > 1: no dense map; smoothing behind zero padding
    images = torch.from_numpy(np.stack([R.make_image('noise', s, 48, 80) for s in (11, 21)]))[:, None].to(DEV)
    out = net({'image': images})
    assert 'desc' not in out and out['orientation'].shape == (2, 4, 48, 80)
    smooth = ClassicDetectors({'method': 'LGHD', 'prob_smoothing': True, 'smoothing_kernel_size': 5})({'image': images})['prob']
    from multipoint_amd.utils.homographies import get_gaussian_filter
    want = torch.nn.functional.conv2d(torch.nn.functional.pad(out['prob'].cpu(), (2, 2, 2, 2)), get_gaussian_filter(5).cpu())
    assert smooth.shape == out['prob'].shape and (smooth.cpu() - want).abs().max() <= 1e-6
