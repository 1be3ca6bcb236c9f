"""Inputs of the LGHD shape tests (tests/test_lghd_shapes_host.py on the CPU, tests/test_gpu_lghd_shapes.py on the kernels of
csrc/fft.hip and csrc/lghd.hip) and the answers of the numpy restatement tests/lghd_restatement.py for them.  Plain numpy,
seeded; every reference is built once per process (functools.lru_cache) and must not be written to.

  supported_lengths       the 131 line lengths 2^a 3^b 5^c in [8, 4096]
  length_groups           those lengths in groups of 11, the parametrisation of the FFT sweep
  FFT_SWEEP_BOUND         the sweep's bound on error / error of np.fft in float32, from the host emulation of the pass
  FRAMES / reference      the orientation frames, the smallest that reach each launch shape of fft.hip, and their float64 answers
  check_orientation       the rule an orientation map is held to (tests/test_gpu_lghd.py uses it too)
  COLUMN_WIDTHS ...       the shapes of the FFT sweep, the 2-D transforms, the batches and the FAST frames
"""
import functools

import numpy as np

import lghd_restatement as R

MIN_N, MAX_N = 8, 4096


def supported_lengths():
    out = []
    for n in range(MIN_N, MAX_N + 1):
        m = n
        for r in (2, 3, 5):
            while m % r == 0:
                m //= r
        if m == 1:
            out.append(n)
    return out


def length_groups(size=11):
    """the 131 lengths in ascending groups of `size` (the last one shorter): one parametrised test each"""
    ls = supported_lengths()
    return [ls[i:i + size] for i in range(0, len(ls), size)]


# ---- the FFT sweep ----
# error / error of np.fft in float32, both against np.fft in float64 and relative to the largest float64 magnitude.  The bound of
# the seven lengths of tests/test_gpu_lghd.py is 8.  For all 131 it is max(8, ceil(2 * worst_host)), where worst_host is the
# largest ratio of the host emulation of the pass (tests/fft_host_harness.cpp) over both builds (with and without contracted
# multiply-adds), all lengths, both directions and bundles of 1 and 4 lines: tests/test_lghd_shapes_host.py measures it and
# asserts that the constant below is that formula's value.  The factor 2 covers the device's contraction and instruction order.
FFT_SWEEP_BOUND = 15           # worst_host = 7.02 (n = 3645, 4 lines, inverse, no contraction; 6.00 with contraction)
HOST_CSHIFTS = (0, 2)
HOST_THREADS = 256
HAND_LENGTHS = (8, 9, 25, 30)
COLUMN_WIDTHS = (19, 3)        # 19: a partial last bundle at 16, 8, 4 and 2 columns; 3: narrower than every bundle but the last
NARROW_LENGTHS = (8, 512, 1024, 4096)      # width 3 runs at one length per bundle width
ROW_LINES = (2, 3)             # the sweep along rows transforms (2, 3, n)
PLANES_2D = [(3, 9, 15), (2, 27, 25), (2, 1024, 8), (1, 8, 4096)]


def complex_noise(seed, shape):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def fft_errors(got, x, axes, inverse):
    """(max |got - float64|, max |np.fft float32 - float64|) of one unnormalised transform of the complex64 array x along `axes`,
    both relative to the largest float64 magnitude"""
    f = (lambda a: np.fft.ifftn(a, axes=axes, norm='forward')) if inverse else (lambda a: np.fft.fftn(a, axes=axes))
    want = f(x.astype(np.complex128))
    single = f(x)
    assert single.dtype == np.complex64 and want.dtype == np.complex128
    top = np.abs(want).max()
    return np.abs(got - want).max() / top, np.abs(single - want).max() / top


def column_bundle(n):
    """(columns per bundle, threads) of launch_lines for a column pass of length n: 16 columns while two buffers fit 128 KiB of
    LDS, 512 threads above 64 KiB"""
    c = 16
    while c > 1 and 2 * 8 * n * c > 128 * 1024:
        c //= 2
    return c, 512 if 2 * 8 * n * c > 64 * 1024 else 256


# ---- orientation frames ----
SEED = 7
# (name, kind, seed, H, W)
FRAMES = [(k + '_%dx%d' % (H, W), k, SEED, H, W) for k, H, W in [
    ('noise', 8, 8),                                  # the minimum length: fewer elements than threads
    ('noise', 9, 15), ('noise', 27, 25),              # only radices 3 and 5
    ('noise', 45, 75), ('smooth', 45, 75),
    ('noise', 16, 320), ('smooth', 16, 320),          # ARGMAX slots 0 and 1
    ('noise', 8, 4096),                               # all 16 slots; a 64 KiB row bundle, still 256 threads
    ('noise', 512, 24),                               # a 128 KiB column bundle, 512 threads, a last bundle of 8 columns
    ('noise', 640, 16),                               # 8 columns per bundle
    ('noise', 2048, 12),                              # 4 columns per bundle
    ('noise', 4096, 9),                               # 2 columns per bundle, the last one a single column
    ('noise', 512, 640), ('smooth', 512, 640)]]       # the model's default frame: slots 0 to 2, 128 KiB column bundles
FRAME_NAMES = [f[0] for f in FRAMES]
FRAME_SIZES = sorted({(f[3], f[4]) for f in FRAMES})


@functools.lru_cache(maxsize=None)
def bank(H, W):
    return R.filter_bank(H, W)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(u8, bank float64, float64 magnitudes, err32, float64 orientation maps) of a frame of FRAMES"""
    _, kind, seed, H, W = next(f for f in FRAMES if f[0] == name)
    u8 = R.quantize(R.make_image(kind, seed, H, W))
    b = bank(H, W)
    m64 = R.responses(u8, b)
    err32 = np.abs(R.responses(u8, b, single=True) - m64).max()
    return u8, b, m64, err32, R.orientation_maps(m64)


def check_orientation(got, name, m64, err32, want):
    """Every pixel whose float64 top-two magnitude gap is at least tau = 16 err32 carries the float64 arg-max; at most 1 % of a
    scale's pixels lie below tau (a condition on the input, tests/test_lghd_host.py and tests/test_lghd_shapes_host.py assert
    it without a GPU)."""
    gap = R.top_two_gap(m64)
    decided = gap >= 16 * err32
    assert np.all((~decided).reshape(4, -1).mean(1) <= 0.01)
    wrong = got != want
    print(name, 'pixels that differ from float64: %d, all with a gap below %.3g err32' % (wrong.sum(), (gap[wrong] / err32).max(initial=0)))
    assert got.max() <= 5
    assert not np.any(wrong & decided)


CONSTANT_SIZES = [(64, 64), (16, 512)]     # powers of two: every non-DC bin of a constant image is exactly zero


# ---- batches ----
BATCH_FRAME = (48, 80)
# the three 48 x 80 images of tests/test_gpu_lghd.py, then fresh seeds: 9 frames are chunks of 4, 4 and 1
BATCH_IMAGES = [('noise', 11), ('smooth', 12), ('noise', 21), ('noise', 31), ('smooth', 32), ('noise', 33), ('smooth', 34),
                ('noise', 35), ('noise', 36)]


@functools.lru_cache(maxsize=None)
def batch_u8():
    H, W = BATCH_FRAME
    return np.stack([R.quantize(R.make_image(k, s, H, W)) for k, s in BATCH_IMAGES])


def image_bytes(H, W):
    """what mp_lghd_orientation needs per image: the spectrum and the 24 filtered planes, complex fp32"""
    return 25 * H * W * 2 * 4


# ---- descriptors of a batch ----
DESCRIBE_K = 11
DESCRIBE_COUNTS = (11, 0, 25)              # 25 > K is clamped to K


def describe_lists():
    """int32 [3][11][2] (y, x) on the 48 x 80 frame: the edge keypoints of tests/test_gpu_lghd.py mixed with rows whose patch
    leaves the frame (y = 19, x = W - 19, y = H - 19, negative coordinates)"""
    H, W = BATCH_FRAME
    edge = [[20, 20], [20, W - 20], [H - 20, 20], [H - 20, W - 20], [20, W // 2], [H // 2, 20], [H - 20, W // 2], [H // 2, W - 20]]
    out = np.zeros((3, DESCRIBE_K, 2), np.int32)
    out[0] = [edge[0], [19, 30], edge[1], edge[2], [H // 2, W - 19], edge[3], edge[4], [-5, -7], edge[5], edge[6], edge[7]]
    out[1] = edge + edge[:3]               # count 0: none of them is read
    out[2] = [[H // 2, -1], edge[7], edge[6], [19, W - 19], edge[5], edge[4], [H - 19, W // 2], edge[3], [-2 ** 31, 30], edge[1],
              [24, 41]]
    return out


def patch_inside(y, x):
    H, W = BATCH_FRAME
    return R.HALF <= y <= H - R.HALF and R.HALF <= x <= W - R.HALF


# ---- FAST around the 64 x 4 block ----
FAST_FRAMES = [(7, 7), (6, 40), (40, 6), (9, 65), (13, 129), (5, 64)]      # 7 x 7: one tested pixel; 6 x 40, 40 x 6, 5 x 64: none


def fast_frame(H, W):
    return np.random.default_rng(1000 * H + W).integers(0, 256, (H, W)).astype(np.uint8)
