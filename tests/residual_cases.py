"""Cases of the residual-field tests.

Planted pairs: an analytic scene -- ecc_cases.gaussians for the coarse layer, a denser sum of small Gaussians of the same form for
the detail a 32-pixel window needs -- evaluated at displaced coordinates for the optical frame, contrast inverted for the thermal
one.  Convention of the field: thermal[p] ~ optical[p + d].

Shape cases: the frames and parameters at which the kernel is compared with the restatement, their masks, and the restatement's own
float32-against-float64 difference from which the comparison's tolerance is taken."""
import functools

import numpy as np

import ecc_cases as EC
import ecc_restatement as E
import residual_restatement as R

HW = (96, 128)
PARAMS = dict(w=32, s=16, r=8, min_valid=0.5, var_floor=1e-8)
# the confidence rule the planted tests use (utils.residual.RESIDUAL_THRESHOLDS' defaults)
MIN_RHO, MIN_MARGIN = 0.5, 0.05


def scene(hw, dy=0.0, dx=0.0, seed=11, n=260):
    """S(y - dy, x - dx) on the pixel grid, float64.  optical = scene(d), thermal = 1 - scene(0) plants
    thermal[p] ~ optical[p + d]."""
    H, W = hw
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    y, x = y - dy, x - dx
    T = np.array([[1.0, 0, -float(dx)], [0, 1.0, -float(dy)], [0, 0, 1.0]])
    coarse = EC.gaussians(hw, T, seed=seed).astype(np.float64)
    rng = np.random.RandomState(seed + 1)
    cy, cx = rng.uniform(-8, H + 8, n), rng.uniform(-8, W + 8, n)
    sg, am = rng.uniform(1.5, 3.5, n), rng.uniform(0.2, 1.0, n) * rng.choice([-1.0, 1.0], n)
    fine = np.zeros((H, W))
    for i in range(n):
        fine += am[i] * np.exp(-((x - cx[i]) ** 2 + (y - cy[i]) ** 2) / (2 * sg[i] ** 2))
    return 0.1 * coarse + 0.4 + 0.2 * fine


def _frames(dy, dx, right=None):
    """optical displaced by (dy, dx) -- in the columns `right` only when given, by nothing elsewhere -- and the inverted thermal"""
    optical = scene(HW, dy, dx)
    if right is not None:
        optical = np.where(right, optical, scene(HW))
    optical = np.clip(optical, 0, 1).astype(np.float32)
    thermal = (1.0 - np.clip(scene(HW), 0, 1)).astype(np.float32)
    return optical, thermal


TWO_REGION = (2.5, -1.25)


@functools.lru_cache(maxsize=None)
def planted(kind):
    """(optical_aligned float32 [96][128], thermal float32, truth): truth(y, x) -> (dy, dx) at a window centre, or None where
    a window straddles two regions."""
    if kind == 'integer':
        o, t = _frames(2.0, -3.0)
        return o, t, lambda y, x: (2.0, -3.0)
    if kind == 'fractional':
        o, t = _frames(1.5, -0.25)
        return o, t, lambda y, x: (1.5, -0.25)
    assert kind == 'two_region'
    H, W = HW
    right = np.tile(np.arange(W) >= W // 2, (H, 1))
    o, t = _frames(TWO_REGION[0], TWO_REGION[1], right)
    half = PARAMS['w'] // 2 + PARAMS['r'] + 4                          # a window whose search region crosses the seam has no truth

    def truth(y, x):
        if abs(x - W // 2) < half:
            return None
        return TWO_REGION if x >= W // 2 else (0.0, 0.0)
    return o, t, truth


def features(frame, f32=True):
    """The feature frame the kernel sees: utils.ecc.ecc_features(frame, 'gradient', 5), restated (float32 with f32)."""
    return np.asarray(E.features(frame, 5, 'gradient', f32), np.float32)


def confident(field):
    with np.errstate(invalid='ignore'):
        return (field['status'] == R.OK) & (field['rho'] >= MIN_RHO) & (field['rho'] - field['second'] >= MIN_MARGIN)


def planted_errors(field, truth, w=PARAMS['w']):
    """(errors of the confident windows that have a truth, in pixels (Euclidean); their number; all windows).  field: one frame's
    arrays (gy, gx, ...)."""
    conf = confident(field)
    errs = []
    for i in range(conf.shape[0]):
        for j in range(conf.shape[1]):
            if not conf[i, j]:
                continue
            y, x = field['origin'][i, j] + w // 2
            tr = truth(int(y), int(x))
            if tr is not None:
                errs.append(float(np.hypot(field['d'][i, j, 0] - tr[0], field['d'][i, j, 1] - tr[1])))
    return np.array(errs), len(errs), conf.size


# What the float64 restatement reaches on the planted pairs (largest error of a confident window with a truth, px), measured on
# the CPU and recorded in DESIGN.md 3.23; the tests assert MARGIN times these, on the restatement and on the GPU alike.  The
# error is the bias of a three-point parabola on a correlation peak that is not a parabola, not arithmetic.
REACHED = {'fractional': 0.151, 'two_region': 0.151}
PLANTED_MARGIN = 1.5
# fewest confident windows with a truth a planted case must have (of 24; two_region: of the 8 whose search region and feature
# support stay clear of the seam).  Measured: all of them.
MIN_CONFIDENT = {'integer': 20, 'fractional': 20, 'two_region': 6}

# ---------------------------------------------------------------------------------------------------------------------------
# kernel-against-restatement shapes: (H, W, w, s, r)
# ---------------------------------------------------------------------------------------------------------------------------
SHAPES = ((24, 24, 8, 4, 1), (33, 47, 8, 5, 3), (40, 56, 16, 8, 4), (50, 66, 24, 7, 2), (96, 128, 32, 16, 8), (96, 128, 48, 24, 8),
          (96, 128, 64, 16, 8))
MASKS = ('none', 'shared', 'per_frame')
FRAMES = 3
MIN_VALID, VAR_FLOOR = 0.5, 1e-8
# A window whose two best restated scores are closer than DELTA may legitimately pick another integer peak: a score is a ratio of
# sums of products that float32 rounds by at most 2^-24 ~ 6e-8 relative each, and centring (sum of squares minus n mean^2, with
# mean^2 a few times the variance for a non-negative feature) amplifies that by about ten: 1e-6 at the worst, DELTA ten times that.
DELTA = 1e-5
LEFT_OUT_CAP = 0.02                                                    # windows inside DELTA: at most 2 % of a case
# The restatement's own f32=True against float64 difference over all shape cases, measured on the CPU (test_residual_host.py
# asserts that it stays below): sub-pixel d in pixels, and rho / rho0 / second.  The GPU comparison allows MARGIN times these.
F32_DIFFERENCE = {'d': 1e-6, 'score': 4e-7}                             # measured: 4.8e-7 px and 2.7e-7
MARGIN = 4.0


@functools.lru_cache(maxsize=None)
def shape_frames(shape):
    """(fo, ft) float32 [FRAMES][H][W]: non-negative feature-like frames with a planted shift per frame plus noise, so that peaks
    are distinct, some at the search border."""
    H, W, w, s, r = shape
    rng = np.random.RandomState(1000 + H * 7 + w)
    pad = r + 1
    fo = np.empty((FRAMES, H, W), np.float32)
    ft = np.empty((FRAMES, H, W), np.float32)
    for b in range(FRAMES):
        base = rng.rand(H + 2 * pad, W + 2 * pad)
        base = 0.25 * (base + np.roll(base, 1, 0) + np.roll(base, 1, 1) + np.roll(base, (1, 1), (0, 1)))      # a little smooth
        dy, dx = ((0, 0), (min(r, 2), -min(r, 1)), (-r, r - 1))[b]                                          # frame 2: at the edge
        fo[b] = base[pad:pad + H, pad:pad + W]
        ft[b] = base[pad + dy:pad + dy + H, pad + dx:pad + dx + W] + 0.15 * rng.rand(H, W)
    ft[1, :r + w, :r + w] = 0.25                                       # frame 1: the first window's template is flat
    return fo, ft


@functools.lru_cache(maxsize=None)
def shape_mask(shape, kind):
    """None, (H, W) or (FRAMES, H, W) uint8: random blobs that leave some windows with too few pixels and most with enough."""
    H, W, w, s, r = shape
    if kind == 'none':
        return None
    rng = np.random.RandomState(2000 + H + w)
    n = 1 if kind == 'shared' else FRAMES
    m = np.ones((n, H, W), np.uint8)
    for b in range(n):
        for _ in range(3):
            y, x = rng.randint(0, H), rng.randint(0, W)
            hh, ww = rng.randint(w // 2, w + r + 1), rng.randint(w // 2, w + r + 1)
            m[b, y:y + hh, x:x + ww] = 0
        m[b, rng.randint(0, H, 12), rng.randint(0, W, 12)] = 0                                               # and single pixels
    return m[0] if kind == 'shared' else m


@functools.lru_cache(maxsize=None)
def restated(shape, kind, f32=True):
    """The restatement's field of all FRAMES frames of a shape case (computed once per session and shared)."""
    H, W, w, s, r = shape
    fo, ft = shape_frames(shape)
    return R.batch(fo, ft, shape_mask(shape, kind), w=w, s=s, r=r, min_valid=MIN_VALID, var_floor=VAR_FLOOR, f32=f32)


def decided(ref):
    """bool mask of the windows whose integer peak is determined beyond DELTA (or that have no peak at all)."""
    with np.errstate(invalid='ignore'):
        return ~(ref['gap'] <= DELTA)


def max_difference(a, b, sel):
    """(largest |d| difference, largest score difference) over the selected windows; NaN must meet NaN, -inf meet -inf."""
    out = []
    for keys in (('d',), ('rho', 'rho0', 'second')):
        worst = 0.0
        for k in keys:
            x, y = a[k][sel], b[k][sel]
            same = (np.isnan(x) & np.isnan(y)) | (x == y)
            assert (np.isfinite(x) == np.isfinite(y)).all(), k
            if (~same).any():
                worst = max(worst, float(np.abs(x[~same] - y[~same]).max()))
        out.append(worst)
    return tuple(out)
