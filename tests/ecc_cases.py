"""Cases of the ECC tests: the planted cross-spectral pairs of registration_cases (thermal = 1 - cut^0.7, contrast inverted) with
starts a known distance off, a smooth analytic pair, and the restatement's own float32-against-float64 difference.

An alignment transform maps thermal pixels to optical ones: the inverse of registration_cases' planted matrix.  Errors are
registration_cases.corner_error of the inverse, in thermal pixels."""
import functools

import numpy as np

import ecc_restatement as E
import registration_cases as RC

NAMES = tuple(RC.CASES)
# corner error of the two starts of every case (the issue's bands: 2-4 px and 5-9.5 px)
START_ERROR = {'near': 3.0, 'far': 7.0}
# the fixture condition of the similarity model: both starts end within this of the planted transform ...
SIMILARITY_CAP = 1.0
# ... and within this of each other (a tenth of the cap; the iteration stops at |d rho| < 1e-8 there)
SAME_POINT = 0.1
FIXTURE_EPS = 1e-8
# The cases that meet the fixture condition under the restatement: all seven (tests/test_ecc_host.py asserts it for each).
FIXTURES = NAMES
# What the restatement reaches (corner error, px) from both starts at FIXTURE_EPS, recorded and no criterion of quality:
# similarity / affine / homography.  The perspective entries are poorly determined by 72 x 96 and 96 x 128 frames.
REACHED = {
    'same_size_rot': (0.110, 0.252, 0.735),
    'same_size_scale_up': (0.075, 0.090, 0.273),
    'same_size_scale_down': (0.041, 0.054, 0.113),
    'small_thermal_rig': (0.654, 0.911, 1.815),
    'small_thermal_rot': (0.377, 0.668, 1.787),
    'small_thermal_far': (0.129, 0.225, 0.442),
    'same_size_far_shift': (0.484, 0.633, 2.247),
}


@functools.lru_cache(maxsize=None)
def pair(name):
    """(optical float32 [96][128], thermal float32, T 3x3 thermal -> optical)"""
    optical, thermal, T = RC.case(name)
    return optical, thermal, np.linalg.inv(T)


def error(T, name):
    """Corner error in thermal pixels of an alignment transform of a case."""
    return RC.corner_error(np.linalg.inv(np.asarray(T, np.float64).reshape(3, 3)), RC.case(name)[2])


def perturbed(T, hw, t):
    """T with a similarity of strength t about the template's centre in front of it: t degrees, scale 1 + t / 100, shift
    (1.5 t, -t) px."""
    H, W = hw
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    a, s = np.radians(t), 1.0 + 0.01 * t
    c, d = s * np.cos(a), s * np.sin(a)
    S = np.array([[c, -d, cx - c * cx + d * cy + 1.5 * t], [d, c, cy - d * cx - c * cy - t], [0.0, 0.0, 1.0]])
    return np.asarray(T, np.float64) @ S


def _start_at(T, hw, target, err):
    """T perturbed until err(.) is `target` (bisection over the strength)."""
    lo, hi = 0.0, 8.0
    assert err(perturbed(T, hw, hi)) > target
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if err(perturbed(T, hw, mid)) < target:
            lo = mid
        else:
            hi = mid
    return perturbed(T, hw, hi)


@functools.lru_cache(maxsize=None)
def start(name, level):
    """The start of a case: the planted transform perturbed until its corner error is START_ERROR[level]."""
    _, thermal, T = pair(name)
    return _start_at(T, thermal.shape, START_ERROR[level], lambda M: error(M, name))


def cli_error(T):
    """Corner error in thermal pixels of an alignment transform of registration_cases.cli_pairs()."""
    return RC.corner_error(np.linalg.inv(np.asarray(T, np.float64).reshape(3, 3)), RC.cli_pairs()[2])


def cli_start(target=6.0):
    """The shared start of the command-line pairs, `target` px off."""
    return _start_at(np.linalg.inv(RC.cli_pairs()[2]), RC.GROUP['thermal_hw'], target, cli_error)


def corner_distance(Ta, Tb, hw):
    """Largest distance, in image pixels, between the images of the template's corners under two alignment transforms."""
    H, W = hw
    c = np.array([[0, 0, 1], [W - 1, 0, 1], [0, H - 1, 1], [W - 1, H - 1, 1]], np.float64).T
    a, b = np.asarray(Ta, np.float64).reshape(3, 3) @ c, np.asarray(Tb, np.float64).reshape(3, 3) @ c
    return float(np.max(np.hypot(*(a[:2] / a[2] - b[:2] / b[2]))))


@functools.lru_cache(maxsize=None)
def restated(name, level, model, maxiter=50, eps=1e-6, f32=False, feature='gradient'):
    optical, thermal, _ = pair(name)
    return E.refine(optical, thermal, start(name, level), model, feature, 5, eps, maxiter, 0.25, f32)


def noise_floor(name, level, model, maxiter):
    """How far fp32 per-pixel terms move the restatement's own trajectory: the corner distance, in optical pixels, between its
    float32-mode and its float64 iterate after maxiter updates at eps = 0."""
    a = restated(name, level, model, maxiter, 0.0, False)
    b = restated(name, level, model, maxiter, 0.0, True)
    return corner_distance(a['transform'], b['transform'], pair(name)[1].shape)


def gaussians(hw, T=None, seed=7, n=12, gain=1.0, bias=0.0):
    """A smooth analytic frame: a sum of n Gaussians (sigma 5-12 px) evaluated at the pixel centres mapped through T."""
    H, W = hw
    rng = np.random.RandomState(seed)
    cx, cy = rng.uniform(0, 128, n), rng.uniform(0, 96, n)
    sg, am = rng.uniform(5, 12, n), rng.uniform(0.3, 1.0, n)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    if T is not None:
        x, y = E.warp(T, x, y)
    v = np.zeros((H, W))
    for i in range(n):
        v += am[i] * np.exp(-((x - cx[i]) ** 2 + (y - cy[i]) ** 2) / (2 * sg[i] ** 2))
    return (gain * v + bias).astype(np.float32)
