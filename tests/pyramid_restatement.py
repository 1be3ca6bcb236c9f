"""numpy float32 restatement of the image pyramid and the staged mutual-information alignment (reference
create_dataset/align_images.py:151-248, helper_functions/align.py:446-613), the model csrc/pyramid.hip and
multipoint_amd.utils.alignment's staged procedure are tested against:

  gaussian_weights       cv2.getGaussianKernel(k, 0, CV_32F): OpenCV's fixed tables up to k = 7, the formula above
  gaussian_blur          cv2.GaussianBlur(frame, (k, k), 0) on a float32 frame (sepFilter2D's float path, BORDER_REFLECT_101)
                         and, with decimate, the reference's [::2, ::2] of it
  frames_to_float        the reference's conversions of 8- and 16-bit frames
  pyramid_levels         sizes and kernel sizes of the levels
  scale_transform        the eight in-place multiplications that take a transform to a level's size and back
  align_images           align.py:446-613 for one pair over mi_restatement, with any Nelder-Mead
  staged                 align_images_mutual_information for one pair
"""
import math

import numpy as np

import mi_restatement as R
from photometric_restatement import border_interpolate, gaussian_kernel

F32 = np.float32
SMALL = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
         7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}


def gaussian_weights(k):
    if k % 2 == 0 or k < 1:
        raise ValueError('k must be odd and positive')
    if k <= 7:
        return np.array(SMALL[k], F32)
    return gaussian_kernel(k)


def gaussian_blur(frame, k, decimate=False):
    """Row filter with the taps summed left to right, then the symmetric column filter: centre tap, then
    ky[r+j] * (S[+j] + S[-j]) for j = 1..r; every product and sum rounded to float32."""
    x = np.asarray(frame, F32)
    H, W = x.shape
    w = gaussian_weights(k)
    r = k // 2
    assert r < min(H, W)
    cols = np.array([border_interpolate(p, W) for p in range(-r, W + r)], np.int64)
    rows = np.array([border_interpolate(p, H) for p in range(-r, H + r)], np.int64)
    t = w[0] * x[:, cols[0:W]]
    for j in range(1, k):
        t = t + w[j] * x[:, cols[j:j + W]]
    assert t.dtype == F32
    out = w[r] * t[rows[r:r + H], :]
    for j in range(1, r + 1):
        out = out + w[r + j] * (t[rows[r + j:r + j + H], :] + t[rows[r - j:r - j + H], :])
    assert out.dtype == F32
    return np.ascontiguousarray(out[::2, ::2]) if decimate else out


def frames_to_float(frames):
    a = np.asarray(frames)
    if a.dtype == np.uint16:
        return a.astype(F32) / F32(65535.0)
    assert a.dtype == np.uint8
    f = a.astype(F32) / F32(255.0)
    if a.ndim == 4:                                                   # BGR -> grey
        return (F32(0.114) * f[..., 0] + F32(0.587) * f[..., 1]) + F32(0.299) * f[..., 2]
    return f


def pyramid_levels(H, W, filter_size, n_levels):
    """[(height, width, ksize)] of the levels in the order they are built (half size first)"""
    out, ratio = [], 1.0
    for _ in range(n_levels):
        ratio *= 0.5
        k = int(math.ceil(filter_size * ratio))
        if k % 2 == 0:
            k += 1
        H, W = len(range(0, H, 2)), len(range(0, W, 2))
        out.append((H, W, k))
    return out


def scale_transform(T, level_shape, full_shape, down):
    t = np.array(T, np.float64).reshape(3, 3).copy()
    ratio_x = float(level_shape[0]) / float(full_shape[0])
    ratio_y = float(level_shape[1]) / float(full_shape[1])
    if down:
        t[0, 1:] *= ratio_x
        t[1:, 0] /= ratio_x
        t[1, 0] *= ratio_y
        t[1, 2] *= ratio_y
        t[0, 1] /= ratio_y
        t[2, 1] /= ratio_y
    else:
        t[0, 1:] /= ratio_x
        t[1:, 0] *= ratio_x
        t[1, 0] /= ratio_y
        t[1, 2] /= ratio_y
        t[0, 1] *= ratio_y
        t[2, 1] *= ratio_y
    return t


def _minimize(func, x0, minimizer):
    """(x, success): scipy's Nelder-Mead when `minimizer` is scipy.optimize.minimize, the restated one for None"""
    if minimizer is None:
        r = R.nelder_mead(func, x0, xatol=1e-6, fatol=1e-6)
        return r['x'], r['success']
    r = minimizer(func, x0, method='Nelder-Mead', options={'adaptive': False, 'xatol': 1e-6, 'fatol': 1e-6})
    return r.x, bool(r.success)


def align_images(optical, thermal, T_init, params, filter_images=False, minimizer=None):
    """align.py:446-613 for a grey float32 pair and a 3x3 transform, without the geometric checks.
    Returns (transform or None, type or None)."""
    optical, thermal = np.asarray(optical, F32), np.asarray(thermal, F32)
    T_init = np.array(T_init, np.float64).reshape(3, 3)
    if filter_images:
        k = params['alignment/filter_size']
        optical, thermal = gaussian_blur(optical, k), gaussian_blur(thermal, k)
    sizes = list(params['alignment/bin_sizes'])
    normalized = bool(params.get('alignment/normalized_mi', False))
    sigma = params.get('alignment/smoothing_sigma', 0)
    H, W = thermal.shape
    cands = []
    if params.get('alignment/accept_init', False):
        cands.append(('init', T_init))
    if params.get('alignment/run_optimization', True):
        for n in sizes:
            x, ok = _minimize(lambda v: R.negative_mi(v, optical, thermal, T_init, n, False, normalized, sigma),
                              T_init.ravel(), minimizer)
            T = np.asarray(x, np.float64).reshape(3, 3)
            a = R.negative_mi(T_init, optical, thermal, T_init, 100, False, normalized, sigma)
            b = R.negative_mi(T, optical, thermal, T_init, 100, False, normalized, sigma)
            valid = abs(a - b) < params['alignment/check/both/max_diff_mi']
            if params.get('alignment/check/invalid_pixels', False):
                valid = valid and R.warp_image(optical, T, H, W).min() != -1.0
            if valid and ok:
                cands.append(('bin' + str(n) + ('_normalized' if normalized else '') + '_s' + str(sigma), T))
    if not cands:
        return None, None
    scores = np.array([[R.negative_mi(T, optical, thermal, T_init, n) for n in sizes] for _, T in cands])
    method = params.get('alignment/ranking_method', 'sum')
    if method == 'sum':
        total = np.zeros(len(cands))
        for j in range(len(sizes)):
            total = total + scores[:, j]
        best = int(np.argmin(total))
    elif method == 'order':
        ranking = np.zeros(len(cands))
        for j in range(len(sizes)):
            ranking += scores[:, j].argsort(kind='stable')
        best = int(np.argmin(ranking))
    else:
        raise ValueError('Unknown ranking_method')
    return cands[best][1].copy(), cands[best][0]


def staged(optical, thermal, t_init, params, minimizer=None, align=None):
    """align_images_mutual_information (align_images.py:151-248) for one grey float32 pair, statement by statement.
    Returns (success, transform, type, stages); stages = [(name, shape, start, type, success)]."""
    if align is None:
        def align(o, t, T, p, filter_images):
            return align_images(o, t, T, p, filter_images, minimizer)
    t_init = np.array(t_init, np.float64).reshape(3, 3)
    transformation = np.copy(t_init)
    success, stages = True, []

    def run(name, o, t, T, filter_images):
        start = np.copy(T)
        new, kind = align(o, t, T, params, filter_images)
        stages.append((name, tuple(o.shape), start, kind, new is not None))
        return new is not None, new, kind

    kind = None
    if params.get('use_image_pyramid', False):
        opt_levels, th_levels = [optical], [thermal]
        ratio = 1.0
        for i in range(params.get('alignment/n_pyramid_levels', 2)):
            ratio *= 0.5
            k = int(np.ceil(params.get('alignment/filter_size', 5) * ratio))
            if k % 2 == 0:
                k += 1
            opt_levels.insert(0, gaussian_blur(opt_levels[0], k, True))
            th_levels.insert(0, gaussian_blur(th_levels[0], k, True))
        opt_levels.pop()
        th_levels.pop()
        for i, (o, t) in enumerate(zip(opt_levels, th_levels)):
            transformation = scale_transform(transformation, o.shape, optical.shape, True)
            success, new, kind = run('pyramid%d' % (len(opt_levels) - i), o, t, transformation, False)
            transformation = scale_transform(new, o.shape, optical.shape, False) if success else np.copy(t_init)
    if params.get('use_smoothing_stage', False):
        success, new, kind = run('smoothing', optical, thermal, transformation, True)
        if success:
            transformation = new
    if not success:
        transformation = np.copy(t_init)
    is_t_init = transformation == t_init
    success, new, kind = run('final', optical, thermal, transformation, False)
    if not success and not is_t_init.all():
        success, new, kind = run('retry', optical, thermal, t_init, False)
    return success, new, kind, stages


def displaced_pair(seed, H=96, W=128):
    """A pair whose start is about 10.5 px off (four-corner error): optical = blob_image(seed, H, W, 150, 2.0, 6.0), thermal =
    4 (w - 0.45)^2 of its warp w under T_true.  Returns optical, thermal, T_true, T_init."""
    optical = R.blob_image(seed, H, W, 150, 2.0, 6.0)
    T_true = np.array([[0.94, 0.012, 6.0], [-0.01, 0.95, 4.0], [1.5e-5, -1e-5, 1.0]])
    w = R.warp_image(optical, T_true, H, W)
    assert w.min() >= 0.0
    thermal = (4.0 * (w.astype(np.float64) - 0.45) ** 2).astype(F32)
    T_init = T_true + np.array([[0.004, 0.0, 8.0], [0.0, -0.003, -6.4], [0.0, 0.0, 0.0]])
    return optical, thermal, T_true, T_init


PARAMS = {'alignment/bin_sizes': [16, 32, 64], 'alignment/normalized_mi': True, 'alignment/smoothing_sigma': 0,
          'alignment/check/both/max_diff_mi': 0.5, 'alignment/accept_init': True, 'alignment/ranking_method': 'sum',
          'alignment/filter_size': 5, 'alignment/n_pyramid_levels': 1, 'use_image_pyramid': True, 'use_smoothing_stage': False}
