"""The inputs of the RIFT tests (tests/test_rift_host.py checks their premises on the CPU, tests/test_gpu_rift.py and
tests/test_gpu_rift_e2e.py run the kernels on them)."""
import functools

import numpy as np

import lghd_restatement as L
import rift_restatement as R

# (name, kind, seed, H, W) for lghd_restatement.make_image: the frames whose maps are compared against float64.  48 x 80 and
# 64 x 64 are lghd_restatement.IMAGES'; 45 x 75 has radices 3 and 5 only and an odd pixel count (the median is one element);
# 16 x 640 is one wide row bundle (three pixels per thread in the row pass); 96 x 128 and 160 x 192 hold patches of 48 and 96.
# Piecewise-constant scenes stay out: their far-field responses are rounding noise in float64 too.
MAP_FRAMES = [im for im in L.IMAGES if im[3:] in ((48, 80), (64, 64))] + [
    ('noise_45x75', 'noise', 21, 45, 75), ('smooth_45x75', 'smooth', 22, 45, 75), ('smooth_96x128', 'smooth', 23, 96, 128),
    ('smooth_160x192', 'smooth', 24, 160, 192), ('noise_16x640', 'noise', 25, 16, 640), ('smooth_16x640', 'smooth', 26, 16, 640)]

# (name, value, H, W): constant frames.  Line lengths 2^a 3^b only: the fp32 radix-5 butterfly of mp_fft.h does not cancel a
# constant line exactly (its two cosine constants do not sum to -1/2 in fp32), so on a length with a factor 5 a constant frame's
# off-DC spectrum is rounding noise instead of 0.  The all-zero frame is exact at any length.
CONSTANT_FRAMES = [('zero_48x80', 0, 48, 80), ('zero_45x75', 0, 45, 75), ('const_64x64', 137, 64, 64), ('const_48x96', 255, 48, 96)]

# frames FAST alone runs on (DESIGN.md 3.11's list): no interior, one interior row / column, a partial 64 x 4 block
DETECT_FRAMES = [(7, 7), (6, 40), (40, 6), (9, 65)]

AMBIGUOUS_CAP = 0.01            # share of pixels whose float64 top-two gap of sumA is below 16 float32 errors, per frame


@functools.lru_cache(maxsize=None)
def map_frame(name):
    _, kind, seed, H, W = next(im for im in MAP_FRAMES if im[0] == name)
    return L.quantize(L.make_image(kind, seed, H, W))


@functools.lru_cache(maxsize=None)
def restated_maps(name):
    """(float64 run, float32 run) of rift_restatement.phase_congruency on a map frame: computed once, shared, never modified"""
    return R.phase_congruency(map_frame(name)), R.phase_congruency(map_frame(name), single=True)


def ambiguous(name):
    """bool [H][W]: the float64 top-two gap of sumA is below 16 float32 errors of sumA (rule 3 of tests/test_gpu_rift.py)"""
    f64, f32 = restated_maps(name)
    return R.top_two_gap(f64['sumA']) < 16 * np.abs(f32['sumA'] - f64['sumA']).max()


@functools.lru_cache(maxsize=None)
def restated_pair(i):
    """per side of planted pair i: (keypoints (y, x), unit rows float64 [n][216]) of the float64 restatement"""
    return tuple(R.restated_side(im, PAIR_FAST_THRESHOLD, PAIR_PATCH)[:2] for im in planted_pair(i))


def constant_frame(name):
    _, value, H, W = next(c for c in CONSTANT_FRAMES if c[0] == name)
    return np.full((H, W), value, np.uint8)


# ---- planted pairs: one analytic scene seen through a similarity, so that no frame is resampled from another ----
PAIR_H, PAIR_W = 160, 192
# (rotation in degrees, scale, (shift x, shift y)): the optical -> thermal map, about the frame centre
PAIRS = [(2.0, 1.03, (5.5, -3.25)), (-3.0, 0.97, (-7.0, 4.5)), (0.0, 1.00, (9.0, 6.0))]
# scene seeds, chosen on the CPU so that a float64 least-squares similarity through the restatement's correct matches stays under
# 0.5 px at the frame corners with a margin (0.25, 0.16, 0.16 px; of the seeds 41 .. 52 about half do)
PAIR_SEEDS = (50, 46, 46)
PAIR_PATCH, PAIR_FAST_THRESHOLD = 48, 6
# mutual nearest neighbours of the float64 restatement within 3 px of the planted map, of all its mutual nearest neighbours
# (tests/test_rift_host.py regenerates and asserts them)
RESTATED_CORRECT = (129, 145, 155)
RESTATED_MUTUAL = (144, 166, 167)


def planted_matrix(i):
    """3 x 3, on (x, y, 1): optical pixel -> thermal pixel"""
    deg, s, (tx, ty) = PAIRS[i]
    c, sn = s * np.cos(np.radians(deg)), s * np.sin(np.radians(deg))
    cx, cy = (PAIR_W - 1) / 2.0, (PAIR_H - 1) / 2.0
    return np.array([[c, -sn, cx - c * cx + sn * cy + tx], [sn, c, cy - sn * cx - c * cy + ty], [0, 0, 1.0]])


def _scene(seed, x, y):
    """160 anisotropic Gaussian blobs (sigma 2 .. 9 px, signed amplitudes) summed and passed through 1 / (1 + exp(-6 v)), at the
    scene coordinates (x, y) (= optical pixel coordinates)"""
    rng = np.random.default_rng(seed)
    n = 160
    bx, by = rng.uniform(-30, PAIR_W + 30, n), rng.uniform(-30, PAIR_H + 30, n)
    s1, s2 = rng.uniform(2, 9, n), rng.uniform(2, 9, n)
    ang = rng.uniform(0, np.pi, n)
    amp = rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n)
    v = np.zeros(x.shape)
    for j in range(n):
        dx, dy = x - bx[j], y - by[j]
        u, w = dx * np.cos(ang[j]) + dy * np.sin(ang[j]), -dx * np.sin(ang[j]) + dy * np.cos(ang[j])
        v += amp[j] * np.exp(-0.5 * ((u / s1[j]) ** 2 + (w / s2[j]) ** 2))
    return 1.0 / (1.0 + np.exp(-6.0 * v))


@functools.lru_cache(maxsize=None)
def planted_pair(i):
    """(optical, thermal) float32 [160][192] in [0, 1]: thermal = 1 - v^0.7 of the scene behind planted_matrix(i)"""
    yy, xx = np.mgrid[0:PAIR_H, 0:PAIR_W].astype(np.float64)
    optical = _scene(PAIR_SEEDS[i], xx, yy)
    inv = np.linalg.inv(planted_matrix(i))
    thermal = 1.0 - _scene(PAIR_SEEDS[i], inv[0, 0] * xx + inv[0, 1] * yy + inv[0, 2], inv[1, 0] * xx + inv[1, 1] * yy + inv[1, 2]) ** 0.7
    return optical.astype(np.float32), thermal.astype(np.float32)


def planted_error(i, kp_optical, kp_thermal):
    """distance in px between the planted image of the optical keypoints (y, x rows) and the thermal keypoints"""
    A = planted_matrix(i)
    o, t = np.asarray(kp_optical, np.float64), np.asarray(kp_thermal, np.float64)
    px = A[0, 0] * o[:, 1] + A[0, 1] * o[:, 0] + A[0, 2]
    py = A[1, 0] * o[:, 1] + A[1, 1] * o[:, 0] + A[1, 2]
    return np.hypot(px - t[:, 1], py - t[:, 0])


def corner_error(i, matrix):
    """largest distance in px between `matrix` and the planted map at the four frame corners"""
    c = np.array([[0, 0, 1], [PAIR_W - 1, 0, 1], [0, PAIR_H - 1, 1], [PAIR_W - 1, PAIR_H - 1, 1.0]]).T
    a, b = planted_matrix(i) @ c, np.asarray(matrix, np.float64) @ c
    return np.hypot(a[0] / a[2] - b[0] / b[2], a[1] / a[2] - b[1] / b[2]).max()
