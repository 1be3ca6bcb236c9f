"""The committed cases of the SIFT tests (tests/test_sift_host.py, tests/test_gpu_sift.py): frames, seeded structured images, and
the float32 noise floor of the restatement on them, from which the GPU tests' tolerances and their near-tie exclusion rule are
derived (4 x the floor: headroom for a different but fixed summation order and another libm)."""
import functools

import numpy as np

import sift_restatement as R

# 40 x 56; 33 x 47: odd sizes (the decimation and the reflected border at every octave); 96 x 120; 16 x 16: the smallest admitted
# frame.  Its doubled base is 32 x 32, so the 5-pixel border leaves 22 x 22 pixels of octave 0 and 6 x 6 of octave 1 in which an
# extremum CAN survive (the structured image has one); only octaves 2 and 3 (8 x 8, 4 x 4) lie inside the border entirely.  The
# count of this frame therefore equals the restatement's, and is 0 without an error on a frame without extrema (a constant one)
FRAMES = ((40, 56), (33, 47), (96, 120), (16, 16))
HEADROOM = 4.0


def structured_image(H, W, seed):
    """float32 [H,W] in [0, 1]: Gaussian blobs of both signs, filled rectangles and a ramp (noise alone gives few stable extrema)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = 0.35 + 0.25 * (x / W) + 0.1 * (y / H)
    for _ in range(max(6, H * W // 100)):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        s = rng.uniform(0.8, 4.0)
        img += rng.choice((-1.0, 1.0)) * rng.uniform(0.15, 0.45) * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))
    for _ in range(max(2, H * W // 1200)):
        y0, x0 = rng.integers(0, H - 4), rng.integers(0, W - 4)
        hh, ww = rng.integers(3, max(4, H // 3)), rng.integers(3, max(4, W // 3))
        img[y0:y0 + hh, x0:x0 + ww] += rng.choice((-1.0, 1.0)) * rng.uniform(0.1, 0.3)
    img += rng.normal(0, 0.01, (H, W))
    return np.clip(img, 0.0, 1.0).astype(np.float32)


def case_image(H, W, index=0):
    return structured_image(H, W, seed=1000 * H + W + 7919 * index)


def quantise(image):
    """(image * 255.0).astype(np.uint8) in float32, as mp_lghd_quantize does"""
    return (image.astype(np.float32) * np.float32(255.0)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def stored_pyramids(H, W, index=0):
    """the float64 model's pyramids rounded to the stored format (float32): the common input of the later stages' two modes"""
    gauss, _ = R.scale_space(quantise(case_image(H, W, index)), np.float64)
    gauss = [g.astype(np.float32) for g in gauss]
    return gauss, [g[1:] - g[:-1] for g in gauss]


FIELDS = ('x', 'y', 'size', 'response')
MARGINS = ('offset', 'contrast', 'edge', 'radius', 'sample', 'histogram')


def _circ(a, b):
    d = abs(float(a) - float(b)) % 360.0
    return min(d, 360.0 - d)


def stage_differences(gauss, dog, cands, dtype=np.float32):
    """float32-mode against float64-mode refinement + orientation on the same pyramids: the largest difference of every record field
    (candidates that agree in fate, position and bins) and of every decision quantity (all candidates that reach it)"""
    val = dict.fromkeys(FIELDS + ('angle',), 0.0)
    dec = dict.fromkeys(MARGINS, 0.0)
    for cd in cands:
        a, b = R.detect_candidate(gauss, dog, cd, np.float64), R.detect_candidate(gauss, dog, cd, dtype)
        for name in MARGINS:
            # the decision quantities themselves differ by what their margins differ by, as long as both sit on the same side
            if name in a['margins'] and name in b['margins'] and np.isfinite(a['margins'][name]) and np.isfinite(b['margins'][name]) \
                    and a['fate'] == b['fate'] and a.get('bins') == b.get('bins'):
                dec[name] = max(dec[name], abs(a['margins'][name] - b['margins'][name]))
        if a['fate'] == 'kept' and b['fate'] == 'kept' and (a['r'], a['c'], a['layer'], a['bins']) == (b['r'], b['c'], b['layer'], b['bins']):
            for name in FIELDS:
                val[name] = max(val[name], abs(float(a[name]) - float(b[name])) / (1.0 if name in ('x', 'y') else abs(float(a[name]))))
            for ra, rb in zip(a['records'], b['records']):
                val['angle'] = max(val['angle'], _circ(ra[3], rb[3]))
    return val, dec


@functools.lru_cache(maxsize=None)
def noise_floor():
    """(tolerances, exclusion thresholds): HEADROOM x the largest float32-against-float64 difference over the committed cases.
    x, y absolute (pixels of the doubled base), size and response relative, angle in degrees; thresholds per margin name."""
    val = dict.fromkeys(FIELDS + ('angle',), 0.0)
    dec = dict.fromkeys(MARGINS, 0.0)
    for H, W in FRAMES:
        gauss, dog = stored_pyramids(H, W)
        v, d = stage_differences(gauss, dog, R.candidates(dog))
        val = {k: max(val[k], v[k]) for k in val}
        dec = {k: max(dec[k], d[k]) for k in dec}
    return {k: HEADROOM * v for k, v in val.items()}, {k: HEADROOM * v for k, v in dec.items()}


def excluded(res, eps):
    """the near-tie exclusion rule: a candidate is left out of the fate / position / bins comparison when one of the decisions its
    float64 evaluation went through lies within the threshold of flipping"""
    return any(res['margins'][name] < eps[name] for name in MARGINS if name in res['margins'])
