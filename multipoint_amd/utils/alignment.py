"""Intensity-based alignment of an optical frame on a thermal one by (normalised) mutual information: the alignment core of
the reference's dataset tooling (create_dataset/helper_functions/align.py) on the GPU (csrc/mutual_info.hip).

The reference's names keep their argument order: warp_image, mutual_information_2d, calculate_negative_mutual_information,
refine_alignment.  Images are fp32 CUDA tensors; a `transform` is a 3x3 float64 matrix (numpy array or tensor) that maps
thermal (destination) pixel coordinates to optical (source) ones, exactly as in the reference, and transforms are returned
as float64 numpy arrays.  negative_mutual_information_batch, refine_alignment_batch and the batched align_images have no
counterpart in the reference.

The staged procedure of the reference's create_dataset/align_images.py (ImageAligner.align_images_mutual_information, lines
151-248) is align_images_mutual_information: an image pyramid from gaussian_blur (csrc/pyramid.hip), an optional stage on
blurred frames and the full-resolution stage, for one pair or a batch that moves through the stages in lockstep.  The
reference pyramids the uint8 BGR optical image (OpenCV's fixed-point 8-bit blur) and converts every level to grey; here the
fp32 grey frame is pyramided.  Both are linear: only the 8-bit rounding of each level differs.

Import this module as multipoint_amd.utils.alignment: its refine_alignment is NOT the guided refine_alignment that
multipoint_amd.utils exports.

The motion model of the optimiser (extension): refine_alignment_batch(model=...) and the yaml key
alignment/model search over the nine matrix entries ('homography', the default and the reference's perspective path), over
(angle, scale, dx, dy) ('similarity', the reference's decomposed form) or over the six entries of the top two rows ('affine').
Every model is a 3x3 matrix under the same perspective warp; model_parameters and model_transform go between the two forms.

Not implemented (NotImplementedError): 2x3 affine transforms and `decompose_transformation` (cv2.warpAffine is another
fixed-point path that has no restatement here), and the geometric part of check_perspective_transformation
(cv2.decomposeHomographyMat).
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from .evaluation import decompose_similarity, transform_model

__all__ = ['warp_image', 'mutual_information_2d', 'calculate_negative_mutual_information', 'refine_alignment',
           'negative_mutual_information_batch', 'refine_alignment_batch', 'align_images', 'joint_histograms',
           'rank_candidates', 'check_perspective_transformation', 'alignment_type_name', 'gaussian_blur', 'frames_to_float',
           'gaussian_weights', 'pyramid_levels', 'scale_transform', 'run_alignment_stages',
           'align_images_mutual_information', 'MODEL_PARAMETERS', 'default_limit', 'model_parameters', 'model_transform',
           'check_affine_geometry']

_AFFINE = ('2x3 affine transforms are not implemented: cv2.warpAffine is a different fixed-point path than '
           'cv2.warpPerspective and has no restatement in this project')


def _transforms(t):
    """any array-like of 3x3 matrices (or flat 9-vectors) -> float64 numpy (n, 9); affine and decomposed forms are refused."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    t = np.asarray(t, np.float64)
    if t.shape[-2:] == (2, 3) or (t.ndim == 1 and t.size == 6):
        raise NotImplementedError(_AFFINE)
    if t.ndim == 1 and t.size == 4:
        raise NotImplementedError('decomposed (angle, scale, dx, dy) transforms are affine: ' + _AFFINE)
    if t.size % 9 != 0 or (t.ndim >= 2 and t.shape[-2:] != (3, 3) and t.shape[-1] != 9):
        raise ValueError('Unknown transformation shape: %s' % (t.shape,))
    return np.ascontiguousarray(t.reshape(-1, 9))


def _frames(x, name):
    """(H, W), (B, H, W) or (B, 1, H, W) fp32 CUDA tensor -> contiguous (B, H, W)."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError('%s must be a CUDA tensor (multipoint_amd computes on the GPU only)' % name)
    if x.dim() == 2:
        x = x[None]
    elif x.dim() == 4:
        if x.shape[1] != 1:
            raise ValueError('%s must have one channel, got %s' % (name, tuple(x.shape)))
        x = x[:, 0]
    elif x.dim() != 3:
        raise ValueError('%s must be (H, W), (B, H, W) or (B, 1, H, W), got %s' % (name, tuple(x.shape)))
    return x.to(torch.float32).contiguous()


def _ints(v):
    v = [int(i) for i in v]
    return (ctypes.c_int * len(v))(*v)


class _Call:
    """The arguments every entry point shares, and a workspace of the size the library asks for."""

    def __init__(self, optical, thermal, pair_index, bins, n_evals=None, smoothing=False):
        self.optical, self.thermal = _frames(optical, 'optical'), _frames(thermal, 'thermal')
        if self.optical.shape[0] != self.thermal.shape[0]:
            raise ValueError('optical and thermal must hold the same number of frames')
        if self.optical.device != self.thermal.device:
            raise ValueError('optical and thermal must be on the same device')
        self.dev = self.optical.device
        self.h = _lib.get_handle(self.dev)
        self.B, self.Ho, self.Wo = self.optical.shape
        self.H, self.W = self.thermal.shape[1:]
        self.pair, self.bins = [int(p) for p in pair_index], [int(b) for b in bins]
        n_evals = len(self.pair) if n_evals is None else n_evals
        maps = len(set(zip(self.pair, self.bins)))
        need = _lib.c_ll()
        rc = self.h.lib.mp_mi_workspace_bytes(n_evals, self.B, max(maps, 1), self.H, self.W, min(max(self.bins + [1]), 256),
                                              int(smoothing), ctypes.byref(need))
        if rc != _lib.MP_OK:
            raise ValueError('mutual information: unsupported sizes (%d evaluations of %d pairs at %dx%d)'
                             % (n_evals, self.B, self.H, self.W))
        self.workspace = torch.empty(need.value, dtype=torch.uint8, device=self.dev)
        self.stream = _lib.stream_ptr(self.dev)

    def head(self):
        return (self.h.ptr, _lib.ptr(self.optical), self.Ho, self.Wo, _lib.ptr(self.thermal), self.H, self.W, self.B)

    def tail(self):
        return (_lib.ptr(self.workspace), self.workspace.numel(), self.stream)


def joint_histograms(optical, thermal, pair_index, bins, transforms, strategy=0, return_warped=False):
    """The joint histograms of the evaluations (pair_index[e], bins[e], transforms[e]): a list of (n, 2n) int64 CPU tensors,
    the (E, 2) fp32 min / max of the warped frames and, if asked for, the warped frames (E, H, W).  strategy 0 chooses the
    histogram kernel by bin count, 1 / 2 force the LDS-privatised / the global-atomics one."""
    T = _transforms(transforms)
    c = _Call(optical, thermal, pair_index, bins)
    E = len(c.pair)
    if T.shape[0] != E or len(c.bins) != E:
        raise ValueError('one pair index, bin count and transform per evaluation')
    Td = torch.from_numpy(T).to(c.dev)
    total = sum(2 * n * n for n in c.bins if 1 <= n <= 256)
    counts = torch.empty(max(total, 1), dtype=torch.int32, device=c.dev)
    minmax = torch.empty((E, 2), dtype=torch.float32, device=c.dev)
    warped = torch.empty((E, c.H, c.W), dtype=torch.float32, device=c.dev) if return_warped else None
    c.h.check(c.h.lib.mp_mi_joint_histogram(*c.head(), _ints(c.pair), _ints(c.bins), _lib.ptr(Td), E, int(strategy),
                                            _lib.ptr(counts), _lib.ptr(minmax), _lib.ptr(warped), *c.tail()))
    flat = counts.cpu().to(torch.int64) & 0xffffffff
    out, at = [], 0
    for n in c.bins:
        out.append(flat[at:at + 2 * n * n].reshape(n, 2 * n))
        at += 2 * n * n
    return out, minmax, warped


def _objective(optical, thermal, pair_index, bins, transforms, init_transforms, normalized_mi, smoothing_sigma):
    """values (E,) float64 CUDA tensor of the evaluations (pair_index[e], bins[e], transforms[e])."""
    T = _transforms(transforms)
    c = _Call(optical, thermal, pair_index, bins, smoothing=smoothing_sigma > 0)
    E = len(c.pair)
    if T.shape[0] != E or len(c.bins) != E:
        raise ValueError('one pair index, bin count and transform per evaluation')
    Td = torch.from_numpy(T).to(c.dev)
    Ti = None
    if init_transforms is not None:
        Ti = _transforms(init_transforms)
        if Ti.shape[0] != E:
            raise ValueError('one initial transform per evaluation')
        Ti = torch.from_numpy(Ti).to(c.dev)
    values = torch.empty(E, dtype=torch.float64, device=c.dev)
    c.h.check(c.h.lib.mp_mi_objective(*c.head(), _ints(c.pair), _ints(c.bins), _lib.ptr(Td), E, float(smoothing_sigma),
                                      int(bool(normalized_mi)), _lib.ptr(Ti), _lib.ptr(values), *c.tail()))
    return values


def negative_mutual_information_batch(optical, thermal, transforms, bins, init_transforms=None, regularize=False,
                                      normalized_mi=False, smoothing_sigma=0):
    """The objective for E transforms of each of B pairs in one launch: optical (B, 1, Ho, Wo), thermal (B, 1, H, W),
    transforms (B, E, 3, 3); bins an int or one int per transform (E); init_transforms (B, 3, 3) or (B, E, 3, 3) for the
    regulariser.  Returns a (B, E) float64 CUDA tensor."""
    t = transforms.detach().cpu().numpy() if isinstance(transforms, torch.Tensor) else np.asarray(transforms, np.float64)
    if t.ndim != 4 or t.shape[2:] != (3, 3):
        if t.ndim == 4 and t.shape[2:] == (2, 3):
            raise NotImplementedError(_AFFINE)
        raise ValueError('transforms must be (B, E, 3, 3), got %s' % (t.shape,))
    B, E = t.shape[:2]
    bins = [int(bins)] * E if np.ndim(bins) == 0 else [int(b) for b in bins]
    if len(bins) != E:
        raise ValueError('bins must be one int or one per transform')
    init = None
    if regularize:
        if init_transforms is None:
            raise ValueError('the regulariser needs init_transforms')
        init = _transforms(init_transforms).reshape(B, -1, 9)
        init = np.broadcast_to(init, (B, E, 9)).reshape(-1, 9)
    pair = np.repeat(np.arange(B), E)
    v = _objective(optical, thermal, pair, bins * B, t.reshape(-1, 9), init, normalized_mi, smoothing_sigma)
    return v.reshape(B, E)


def warp_image(image, transform, height, width):
    """cv2.warpPerspective(image, inv(transform), (width, height), borderValue=-1.0) (align.py:13-50) for one frame (H, W) or a
    batch (B, 1, H, W) with one transform for all frames or one per frame.  Returns a tensor of the input's rank."""
    T = _transforms(transform)
    img = _frames(image, 'image')
    B = img.shape[0]
    if T.shape[0] not in (1, B):
        raise ValueError('one transform, or one per frame')
    T = np.broadcast_to(T, (B, 9)).copy()
    dummy = torch.zeros((B, int(height), int(width)), dtype=torch.float32, device=img.device)
    _, _, warped = joint_histograms(img, dummy, range(B), [1] * B, T, return_warped=True)
    if image.dim() == 2:
        return warped[0]
    return warped[:, None] if image.dim() == 4 else warped


def _sample_grid(n):
    """rows x cols = n with both sides within the warp's 32767 limit (the samples are laid out as a frame)."""
    if n <= 32767:
        return 1, n
    for cols in range(32767, 0, -1):
        if n % cols == 0 and n // cols <= 32767:
            return n // cols, cols
    raise ValueError('cannot lay %d samples out as a frame of at most 32767 x 32767' % n)


def mutual_information_2d(x, y, sigma=5, bins=100, normalized=False):
    """(Normalised) mutual information of two equally long sample vectors from their n x 2n joint histogram (align.py:52-100).
    x, y: fp32 CUDA tensors of any shape with the same number of elements.  Returns a float.
    The samples are laid out as a frame of at most 32767 x 32767 for the identity warp: a 2-D input keeps its shape, up to
    32767 samples form one row, more need a factorisation within those limits (ValueError otherwise, e.g. a large prime)."""
    if x.numel() != y.numel():
        raise ValueError('x and y must have the same number of samples')
    rows, cols = (x.shape if x.dim() == 2 and max(x.shape) <= 32767 else _sample_grid(x.numel()))
    # the identity warp copies x bit for bit (every coordinate lands on a pixel centre with weight 1)
    v = _objective(x.reshape(rows, cols), y.reshape(rows, cols), [0], [bins], np.eye(3), None, normalized, sigma)
    return -float(v.item())


def calculate_negative_mutual_information(transform, optical, thermal, init_transform, bins, regularize=False,
                                          normalized_mi=False, smoothing_sigma=0):
    """Negative mutual information between the warped optical and the thermal frame (align.py:102-155), plus the Frobenius
    norm of init_transform - transform with `regularize`.  Returns a float."""
    _transforms(init_transform)
    v = _objective(optical, thermal, [0], [bins], transform, init_transform if regularize else None, normalized_mi,
                   smoothing_sigma)
    return float(v.item())


MODEL_PARAMETERS = {'homography': 9, 'similarity': 4, 'affine': 6}       # n: the simplex has n + 1 vertices


def default_limit(model):
    """scipy's default for maxiter and maxfun: 200 times the number of parameters of the motion model."""
    transform_model(model)
    return 200 * MODEL_PARAMETERS[model]


def model_parameters(T, model):
    """The parameter vector the optimiser searches from for a 3x3 matrix T (or (P, 3, 3) / (P, 9)) under a motion model, on
    the host in float64: (n,) for one matrix, (P, n) for several.
      'homography'  the nine entries as given (its scale is a parameter of its own: nothing is divided)
      'similarity'  (angle, scale, dx, dy) of T / T[2,2] as decompose_similarity gives them: angle = arctan2(T01, T00), scale =
                    hypot(T00, T01), dx = T02, dy = T12 -- ROW 0 and the translations; the second row is not read, so a matrix
                    that is no similarity is projected onto one
      'affine'      the six entries of the top two rows of T / T[2,2]
    ValueError: an unknown model, T[2,2] == 0 or a non-finite matrix under a constrained model."""
    transform_model(model)
    M = _transforms(T)
    shape = tuple(T.shape) if hasattr(T, 'shape') else np.shape(T)
    single = len(shape) == 1 or shape == (3, 3)
    if model == 'homography':
        out = M.copy()
    else:
        if not (np.isfinite(M).all() and (M[:, 8] != 0.0).all()):
            raise ValueError('model_parameters: need finite 3x3 matrices with T[2,2] != 0')
        if model == 'similarity':
            out = np.array([decompose_similarity(m.reshape(3, 3)) for m in M], np.float64).reshape(-1, 4)
        else:
            out = (M / M[:, 8:9])[:, :6].copy()
    return out[0] if single else out


def model_transform(params, model, device=None):
    """The 3x3 matrix of a parameter vector (n,) -> (3, 3), or of (P, n) -> (P, 3, 3), as float64 numpy: computed on the
    device by the function the optimiser's kernels use (mp_mi_model_transform).
      'similarity'  [[s cos a, s sin a, dx], [-s sin a, s cos a, dy], [0, 0, 1]] (utils.compose_similarity)
      'affine'      the six entries over the row (0, 0, 1);  'homography'  the nine entries
    Parameters are mapped as they are: a negative scale or an angle beyond pi is not clamped."""
    mid, n = transform_model(model), MODEL_PARAMETERS[model]
    p = params.detach().cpu().numpy() if isinstance(params, torch.Tensor) else params
    p = np.asarray(p, np.float64)
    if p.ndim not in (1, 2) or p.shape[-1] != n:
        raise ValueError('%s parameters must be (%d,) or (P, %d), got %s' % (model, n, n, p.shape))
    rows = np.ascontiguousarray(p.reshape(-1, n))
    dev = _lib.require_cuda(device)
    if rows.shape[0] == 0:
        return np.zeros((0, 3, 3))
    h = _lib.get_handle(dev)
    pd = torch.from_numpy(rows).to(dev)
    out = torch.empty((rows.shape[0], 9), dtype=torch.float64, device=dev)
    h.check(h.lib.mp_mi_model_transform(h.ptr, mid, _lib.ptr(pd), rows.shape[0], _lib.ptr(out), _lib.stream_ptr(dev)))
    out = out.cpu().numpy().reshape(-1, 3, 3)
    return out[0] if p.ndim == 1 else out


def refine_alignment_batch(optical, thermal, pair_index, bins, init_transforms, regularize=False, normalized_mi=False,
                           smoothing_sigma=0, xatol=1e-6, fatol=1e-6, maxiter=None, maxfun=None, chunk=32, model='homography'):
    """Nelder-Mead maximisation of the mutual information for a batch of problems (pair_index[q], bins[q],
    init_transforms[q]) as scipy runs it for the reference (align.py:202-207).  xatol, fatol, maxiter, maxfun: scalars or one
    value per problem (None: scipy's 200 * n).  The iterations are enqueued `chunk` at a time; between chunks one integer, the
    number of problems still running, is read back.
    model: what the simplex moves over -- the n = 9 entries of the matrix ('homography'), n = 4 (angle, scale, dx, dy)
    ('similarity') or the n = 6 entries of the top two rows ('affine'); the start is model_parameters(init_transforms, model),
    and with `regularize` the distance is measured from the matrix of that start.
    Returns dict(transform (P, 3, 3), params (P, n), value (P,), nit, nfev, success) of numpy arrays -- params the best
    vertex, transform its matrix -- plus 'rounds', the number of objective launches that were enqueued (a multiple of
    `chunk`)."""
    mid, n = transform_model(model), MODEL_PARAMETERS[model]
    T = _transforms(init_transforms)
    P = T.shape[0]
    pair, bins = [int(p) for p in pair_index], [int(b) for b in bins]
    if len(pair) != P or len(bins) != P:
        raise ValueError('one pair index, bin count and initial transform per problem')

    def per(v, default):
        v = default if v is None else v
        return [v] * P if np.ndim(v) == 0 else list(v)
    if maxiter is None and maxfun is None:
        maxiter = maxfun = default_limit(model)
    big = 2 ** 31 - 1
    it, fn, xa, fa = per(maxiter, big), per(maxfun, big), per(xatol, 1e-6), per(fatol, 1e-6)
    S = _lib.MP_MI_SLOTS
    c = _Call(optical, thermal, pair, bins, n_evals=S * P, smoothing=smoothing_sigma > 0)
    problems = (_lib.MiProblem * P)(*[_lib.MiProblem(pair[q], bins[q], int(min(it[q], big)), int(min(fn[q], big)),
                                                     float(xa[q]), float(fa[q])) for q in range(P)])
    Xd = torch.from_numpy(np.ascontiguousarray(model_parameters(T, model).reshape(P, n))).to(c.dev)
    lib = c.h.lib
    c.h.check(lib.mp_mi_refine_begin_model(*c.head(), problems, None, P, float(smoothing_sigma), int(bool(normalized_mi)),
                                           int(bool(regularize)), *c.tail(), mid, _lib.ptr(Xd)))
    live = torch.zeros(1, dtype=torch.int32, device=c.dev)
    rounds = 0
    while True:
        c.h.check(lib.mp_mi_refine_step(c.h.ptr, _lib.ptr(c.workspace), int(chunk), _lib.ptr(live), c.stream))
        rounds += int(chunk)
        if int(live.item()) == 0:
            break
    out_T = torch.empty((P, 9), dtype=torch.float64, device=c.dev)
    out_X = torch.empty((P, n), dtype=torch.float64, device=c.dev)
    value = torch.empty(P, dtype=torch.float64, device=c.dev)
    nit, nfev, ok = (torch.empty(P, dtype=torch.int32, device=c.dev) for _ in range(3))
    c.h.check(lib.mp_mi_refine_result_model(c.h.ptr, _lib.ptr(c.workspace), _lib.ptr(out_T), _lib.ptr(value), _lib.ptr(nit),
                                            _lib.ptr(nfev), _lib.ptr(ok), c.stream, _lib.ptr(out_X)))
    return {'transform': out_T.cpu().numpy().reshape(P, 3, 3), 'params': out_X.cpu().numpy(), 'value': value.cpu().numpy(),
            'nit': nit.cpu().numpy(), 'nfev': nfev.cpu().numpy(), 'success': ok.cpu().numpy().astype(bool), 'rounds': rounds}


def refine_alignment(optical, thermal, init_transform, decompose_transformation, regularize, bins=256, normalized_mi=False,
                     smoothing_sigma=0):
    """Refine the alignment by maximising the mutual information between the optical and the thermal frame
    (align.py:157-215).  Returns (transform (3, 3) float64 numpy array, success)."""
    # (decompose_transformation: the reference only decomposes 2x3 transforms and ignores the flag for a 3x3 one; so does
    # this -- a 2x3 transform, decomposed or not, is refused by _transforms)
    T = _transforms(init_transform)
    r = refine_alignment_batch(optical, thermal, [0], [bins], T, regularize, normalized_mi, smoothing_sigma)
    return r['transform'][0], bool(r['success'][0])


def check_perspective_transformation(*args, **kwargs):
    raise NotImplementedError('the geometric checks of check_perspective_transformation (rotation and translation limits) '
                              'decompose the homography with cv2.decomposeHomographyMat, which has no restatement in this '
                              'project; align_images applies the mutual-information check only')


AFFINE_CHECK_KEYS = ('alignment/check/both/max_diff_dx', 'alignment/check/both/max_diff_dy',
                     'alignment/check/affine/max_diff_scale', 'alignment/check/affine/max_diff_rotation',
                     'alignment/check/affine/max_diff_shear')


def check_affine_geometry(init_transformation, transformation, params):
    """The geometric part of the reference's check_affine_transformation (align.py:391-404, :423-429) on the top two rows of
    two 3x3 matrices with last row (0, 0, 1) (each divided by its [2,2] first), in numpy float64: |d dx|, |d dy| below
    alignment/check/both/max_diff_dx, .../max_diff_dy; |d s_x|, |d s_y| below alignment/check/affine/max_diff_scale; |d rot|,
    |d shear| below .../max_diff_rotation, .../max_diff_shear (degrees), with rot = arctan2(T01, T00), shear = arctan2(T11, T10)
    - pi / 2 - rot, s_x = sqrt(T10^2 + T00^2), s_y = sqrt(T11^2 + T01^2) cos(shear).  A missing key is a KeyError naming it.
    Returns a bool."""
    lim = {k: params[k] for k in AFFINE_CHECK_KEYS}

    def parts(T):
        T = np.asarray(T, np.float64).reshape(3, 3)
        T = T / T[2, 2]
        rot = np.arctan2(T[0, 1], T[0, 0])
        shear = np.arctan2(T[1, 1], T[1, 0]) - np.pi * 0.5 - rot
        s_x = np.sqrt(T[1, 0] ** 2 + T[0, 0] ** 2)
        s_y = np.sqrt(T[1, 1] ** 2 + T[0, 1] ** 2) * np.cos(shear)
        return rot, shear, s_x, s_y, T[0, 2], T[1, 2]
    a, b = parts(init_transformation), parts(transformation)
    return bool(abs(a[4] - b[4]) < lim['alignment/check/both/max_diff_dx'] and
                abs(a[5] - b[5]) < lim['alignment/check/both/max_diff_dy'] and
                abs(b[2] - a[2]) < lim['alignment/check/affine/max_diff_scale'] and
                abs(b[3] - a[3]) < lim['alignment/check/affine/max_diff_scale'] and
                abs(b[0] - a[0]) < np.radians(lim['alignment/check/affine/max_diff_rotation']) and
                abs(b[1] - a[1]) < np.radians(lim['alignment/check/affine/max_diff_shear']))


def alignment_type_name(bins, normalized_mi, smoothing_sigma, model=None):
    """wrapper_refine_alignement's name of a perspective alignment (align.py:249-259); a constrained motion model
    ('similarity', 'affine') is appended as '_<model>'."""
    name = 'bin' + str(bins) + ('_normalized' if normalized_mi else '') + '_s' + str(smoothing_sigma)
    return name if model in (None, 'homography') else name + '_' + str(model)


def rank_candidates(scores, method):
    """Index of the best candidate from scores[candidate][bin size] (negative mutual information: smaller is better),
    align.py:568-594 as written: 'sum' adds a candidate's scores; 'order' adds, per bin size, the argsort() of the
    candidates' scores -- the indices that would sort them, not the candidates' ranks -- and takes the smallest total."""
    s = np.asarray(scores, np.float64)
    if s.ndim != 2 or s.shape[0] < 1:
        raise ValueError('scores must be (candidates, bin sizes)')
    if method == 'sum':
        total = np.zeros(s.shape[0])
        for k in range(s.shape[1]):
            total = total + s[:, k]
        return int(np.argmin(total))
    if method == 'order':
        ranking = np.zeros(s.shape[0])
        for k in range(s.shape[1]):
            ranking += s[:, k].argsort(kind='stable')
        return int(np.argmin(ranking))
    raise ValueError('Unknown ranking_method')


def gaussian_weights(ksize):
    """getGaussianKernel(ksize, 0, CV_32F) as the library's blur uses it: float32 numpy (ksize,).  Needs no GPU."""
    w = (ctypes.c_float * 31)()
    if _lib.load_library().mp_gaussian_weights(int(ksize), w) != _lib.MP_OK:
        raise ValueError('ksize must be odd and in [1, 31], got %s' % (ksize,))
    return np.array(w[:int(ksize)], np.float32)


def gaussian_blur(frames, ksize, decimate=False):
    """cv2.GaussianBlur(frame, (ksize, ksize), 0) of fp32 CUDA frames (H, W), (B, H, W) or (B, 1, H, W): the float path of
    sepFilter2D with BORDER_REFLECT_101, bit for bit (include/multipoint_hip.h states the arithmetic).  decimate=True returns
    the blurred frames' [::2, ::2] -- (H + 1) // 2 x (W + 1) // 2 -- and computes only those pixels.  Returns a new tensor of
    the input's rank.  ValueError: an even ksize or one outside [1, 31], ksize // 2 >= min(H, W)."""
    x = _frames(frames, 'frames')
    B, H, W = x.shape
    shape = (B, (H + 1) // 2, (W + 1) // 2) if decimate else (B, H, W)
    out = torch.empty(shape, dtype=torch.float32, device=x.device)
    h = _lib.get_handle(x.device)
    h.check(h.lib.mp_gaussian_blur(h.ptr, _lib.ptr(x), B, H, W, int(ksize), int(bool(decimate)), _lib.ptr(out),
                                   _lib.stream_ptr(x.device)))
    if frames.dim() == 2:
        return out[0]
    return out[:, None] if frames.dim() == 4 else out


def frames_to_float(frames, device=None, single_bgr=False):
    """8- and 16-bit frames as the reference turns them into fp32: uint8 (B, H, W) -> / 255 (align.py:485 for a grey frame),
    uint8 BGR (B, H, W, 3) -> / 255, then cv2.COLOR_BGR2GRAY, uint16 (B, H, W) -> / 65535 (align_images.py:161).  frames: a
    numpy array or a CUDA tensor; one grey frame may come as (H, W); a 3-D uint8 array is a batch of grey frames unless
    single_bgr says it is ONE (H, W, 3) BGR frame.  Returns a (B, H, W) fp32 CUDA tensor, (H, W) for one frame."""
    if isinstance(frames, np.ndarray):
        a = np.ascontiguousarray(frames)
        if a.dtype == np.uint16:
            x = torch.from_numpy(a.view(np.int16)).to(_lib.require_cuda(device)).view(torch.uint16)
        elif a.dtype == np.uint8:
            x = torch.from_numpy(a).to(_lib.require_cuda(device))
        else:
            raise ValueError('frames must be uint8 or uint16, got %s' % a.dtype)
    else:
        x = frames
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError('frames must be a numpy array or a CUDA tensor (multipoint_amd computes on the GPU only)')
        if x.dtype not in (torch.uint8, torch.uint16):
            raise ValueError('frames must be uint8 or uint16, got %s' % x.dtype)
        x = x.contiguous()
    bgr = x.dtype == torch.uint8 and x.dim() >= 3 and x.shape[-1] == 3 and (x.dim() == 4 or single_bgr)
    single = x.dim() == (3 if bgr else 2)
    if single:
        x = x[None]
    if x.dim() != (4 if bgr else 3):
        raise ValueError('frames must be (B, H, W), (B, H, W, 3) BGR or one frame of either, got %s' % (tuple(x.shape),))
    mode = _lib.MP_FRAMES_U16 if x.dtype == torch.uint16 else _lib.MP_FRAMES_BGR8 if bgr else _lib.MP_FRAMES_U8
    B, H, W = x.shape[:3]
    out = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
    h = _lib.get_handle(x.device)
    h.check(h.lib.mp_frames_to_float(h.ptr, _lib.ptr(x), mode, B, H, W, _lib.ptr(out), _lib.stream_ptr(x.device)))
    return out[0] if single else out


def align_images(optical, thermal, init_transform, params, geometric_checks=False, filter_images=False, stats=None):
    """The reference's align_images (align.py:446-613) for B pairs at once: every bin size of every pair is one Nelder-Mead
    problem of one batch; a result is a candidate when the solver succeeded and the mutual information at 100 bins moved
    by less than alignment/check/both/max_diff_mi (and, with alignment/check/invalid_pixels, no border pixel entered the
    frame); the initial transform is a candidate with alignment/accept_init; every candidate is scored under every bin size in
    one objective call and ranked by alignment/ranking_method.

    optical (Ho, Wo) or (B, 1, Ho, Wo), thermal (H, W) or (B, 1, H, W), init_transform (3, 3) or (B, 3, 3).
    alignment/model (extension; 'homography' by default, 'similarity', 'affine'): the motion model the optimiser searches in
    (refine_alignment_batch); with another one than the default the candidates' types end in '_<model>'.  The 'init'
    candidate stays the given matrix.
    geometric_checks=True asks for the rotation / translation limits of check_perspective_transformation as well, which are
    not implemented: with the homography it raises NotImplementedError (the default applies the mutual-information check
    only).  With a constrained model it applies check_affine_geometry -- the limits of the reference's
    check_affine_transformation -- to every optimised candidate; a missing limit is a KeyError naming the key.
    alignment/ecc/enable (extension, absent by default): each pair gets one more candidate of type
    'ecc_<feature>_<model>' from utils.ecc.refine_alignment_ecc_batch started at its initial transform -- alignment/ecc/feature
    ('gradient'), alignment/ecc/filter_size (5), alignment/ecc/model (alignment/model), alignment/ecc/eps (1e-6),
    alignment/ecc/max_iterations (50) -- under the same checks and the same ranking; stats['ecc_rounds'] grows by its iterations.
    filter_images=True blurs both frames with gaussian_blur(., alignment/filter_size) first (align.py:487-489).
    Returns (transform, type, candidates) for one pair, lists of them for a batch; transform and type are None where no
    candidate is valid.  A candidate is dict(type, transform, mi={bins: score}, value, init_value, nit, nfev).  stats: a dict
    whose 'rounds' grows by the objective launches the optimisation enqueued (refine_alignment_batch)."""
    model = params.get('alignment/model', 'homography')
    transform_model(model)
    if geometric_checks:
        if model == 'homography':
            check_perspective_transformation()
        for key in AFFINE_CHECK_KEYS:
            params[key]
    if params.get('alignment/decomposed_transformation', False):
        raise NotImplementedError('alignment/decomposed_transformation: ' + _AFFINE)
    single = optical.dim() == 2
    opt, th = _frames(optical, 'optical'), _frames(thermal, 'thermal')
    if filter_images:
        opt, th = gaussian_blur(opt, params['alignment/filter_size']), gaussian_blur(th, params['alignment/filter_size'])
    B = opt.shape[0]
    T0 = np.broadcast_to(_transforms(init_transform), (B, 9)) if _transforms(init_transform).shape[0] == 1 \
        else _transforms(init_transform)
    if T0.shape[0] != B:
        raise ValueError('one initial transform, or one per pair')
    sizes = [int(b) for b in params['alignment/bin_sizes']]
    normalized = bool(params.get('alignment/normalized_mi', False))
    sigma = params.get('alignment/smoothing_sigma', 0)
    cands = [[] for _ in range(B)]
    if params.get('alignment/accept_init', False):
        for b in range(B):
            cands[b].append({'type': 'init', 'transform': T0[b].reshape(3, 3).copy()})
    if params.get('alignment/run_optimization', True) and sizes:
        pair = [b for b in range(B) for _ in sizes]
        r = refine_alignment_batch(opt, th, pair, sizes * B, T0[pair], False, normalized, sigma, model=model)
        if stats is not None:
            stats['rounds'] = stats.get('rounds', 0) + r['rounds']
        # the check of check_perspective_transformation that needs no decomposition: |MI(init) - MI(new)| at 100 bins
        P = len(pair)
        both = np.concatenate([T0[pair], r['transform'].reshape(P, 9)])
        mi100 = _objective(opt, th, pair * 2, [100] * (2 * P), both, None, normalized, sigma).cpu().numpy()
        own = _objective(opt, th, pair, sizes * B, T0[pair], None, normalized, sigma).cpu().numpy()
        inside = np.ones(P, bool)
        if params.get('alignment/check/invalid_pixels', False):
            _, mm, _ = joint_histograms(opt, th, pair, [1] * P, r['transform'])
            inside = mm[:, 0].cpu().numpy() != -1.0
        for q in range(P):
            valid = abs(mi100[q] - mi100[P + q]) < params['alignment/check/both/max_diff_mi'] and inside[q]
            if valid and geometric_checks:
                valid = check_affine_geometry(T0[pair[q]], r['transform'][q], params)
            if valid and r['success'][q]:
                cands[pair[q]].append({'type': alignment_type_name(sizes[q % len(sizes)], normalized, sigma, model),
                                       'transform': r['transform'][q].copy(), 'value': float(r['value'][q]),
                                       'init_value': float(own[q]), 'nit': int(r['nit'][q]), 'nfev': int(r['nfev'][q])})
    if params.get('alignment/ecc/enable', False):
        _ecc_candidates(opt, th, T0, params, model, normalized, sigma, geometric_checks, cands, stats)
    # the ranking scores are the plain negative mutual information, as align.py:531-535 and :551-555 call it
    flat =[(b, c) for b in range(B) for c in cands[b]]
    if flat and sizes:
        pair = [b for b, _ in flat for _ in sizes]
        Ts = np.stack([c['transform'].reshape(9) for _, c in flat for _ in sizes])
        sc = _objective(opt, th, pair, sizes * len(flat), Ts, None, False, 0).cpu().numpy().reshape(len(flat), len(sizes))
        for (_, c), row in zip(flat, sc):
            c['mi'] = {n: float(v) for n, v in zip(sizes, row)}
    best_T, best_type = [], []
    for b in range(B):
        if not cands[b]:
            best_T.append(None); best_type.append(None)
            continue
        i = rank_candidates([[c['mi'][n] for n in sizes] for c in cands[b]], params.get('alignment/ranking_method', 'sum'))
        best_T.append(cands[b][i]['transform']); best_type.append(cands[b][i]['type'])
    if single:
        return best_T[0], best_type[0], cands[0]
    return best_T, best_type, cands


def _ecc_candidates(opt, th, T0, params, model, normalized, sigma, geometric_checks, cands, stats):
    """alignment/ecc/enable (extension): one more candidate per pair, 'ecc_<feature>_<model>', from the ECC
    refinement of utils.ecc started at the pair's T0.  It passes the checks of the optimised candidates -- the solver's success,
    |MI(init) - MI(new)| at 100 bins below alignment/check/both/max_diff_mi, alignment/check/invalid_pixels, and with
    geometric_checks and a constrained model check_affine_geometry -- and is ranked with them."""
    from .ecc import refine_alignment_ecc_batch
    feature = params.get('alignment/ecc/feature', 'gradient')
    ecc_model = params.get('alignment/ecc/model', model)
    B = opt.shape[0]
    pair = list(range(B))
    r = refine_alignment_ecc_batch(opt, th, pair, T0, model=ecc_model, feature=feature,
                                   ksize=params.get('alignment/ecc/filter_size', 5), eps=params.get('alignment/ecc/eps', 1e-6),
                                   maxiter=params.get('alignment/ecc/max_iterations', 50))
    if stats is not None:
        stats['ecc_rounds'] = stats.get('ecc_rounds', 0) + r['rounds']
    both = np.concatenate([T0, r['transform'].reshape(B, 9)])
    mi100 = _objective(opt, th, pair * 2, [100] * (2 * B), both, None, normalized, sigma).cpu().numpy()
    inside = np.ones(B, bool)
    if params.get('alignment/check/invalid_pixels', False):
        _, mm, _ = joint_histograms(opt, th, pair, [1] * B, r['transform'])
        inside = mm[:, 0].cpu().numpy() != -1.0
    for b in range(B):
        valid = abs(mi100[b] - mi100[B + b]) < params['alignment/check/both/max_diff_mi'] and inside[b]
        if valid and geometric_checks and ecc_model in ('similarity', 'affine'):
            valid = check_affine_geometry(T0[b], r['transform'][b], params)
        if valid and r['success'][b]:
            cands[b].append({'type': 'ecc_%s_%s' % (feature, ecc_model), 'transform': r['transform'][b].copy(),
                             'value': float(r['rho'][b]), 'nit': int(r['nit'][b]), 'converged': bool(r['converged'][b])})


# ---- the staged procedure of create_dataset/align_images.py:151-248 ----
def pyramid_levels(H, W, filter_size, n_levels):
    """The pyramid align_images.py:163-171 builds from an H x W frame, in the order it is built (finest first): a list of
    (height, width, ksize), level i (1-based) being the [::2, ::2] of level i - 1 blurred with ksize =
    ceil(filter_size * 0.5 ** i), plus 1 if that is even.  The stages run the list backwards (coarsest first)."""
    out, ratio = [], 1.0
    for _ in range(int(n_levels)):
        ratio *= 0.5
        k = int(np.ceil(filter_size * ratio))
        if k % 2 == 0:
            k += 1
        H, W = (H + 1) // 2, (W + 1) // 2
        out.append((H, W, k))
    return out


def scale_transform(T, level_shape, full_shape, down):
    """A full-size transform at a pyramid level's size (down=True) or back (down=False): the eight in-place multiplications
    of align_images.py:178-186 / :199-205 as written, in their order -- ratio_x from the ROW counts, ratio_y from the column
    counts.  For frames with even sides this is S T S^-1 with S = diag(r, r, 1).  Returns a new (3, 3) float64 array."""
    T = np.array(T, np.float64).reshape(3, 3)
    ratio_x = float(level_shape[0]) / float(full_shape[0])
    ratio_y = float(level_shape[1]) / float(full_shape[1])
    if down:
        T[0, 1:] *= ratio_x
        T[1:, 0] /= ratio_x
        T[1, 0] *= ratio_y
        T[1, 2] *= ratio_y
        T[0, 1] /= ratio_y
        T[2, 1] /= ratio_y
    else:
        T[0, 1:] /= ratio_x
        T[1:, 0] *= ratio_x
        T[1, 0] /= ratio_y
        T[1, 2] /= ratio_y
        T[0, 1] *= ratio_y
        T[2, 1] *= ratio_y
    return T


def run_alignment_stages(optical, thermal, t_init, params, align, blur):
    """The stage sequence of ImageAligner.align_images_mutual_information (align_images.py:151-248) for B pairs in lockstep,
    over an injected aligner and blur (align_images and gaussian_blur on the GPU; the tests drive it with stand-ins):

      align(optical, thermal, transforms (n, 3, 3), params, filter_images) -> (transforms, types, candidates), lists of n,
          a transform None where the pair has no valid candidate
      blur(frames, ksize, decimate) -> frames

    optical, thermal: arrays or tensors (B, H, W) that a list of indices can select from; t_init (B, 3, 3).
      pyramid    (use_image_pyramid) both frames blurred and decimated alignment/n_pyramid_levels times; coarsest level first,
                 the full size excluded: the transform is scaled down from full size, aligned there and scaled back up; a pair
                 that fails a level goes back to its t_init
      smoothing  (use_smoothing_stage) one full-size call with filter_images=True; failure: back to t_init
      final      the full-size call; a pair that fails it and did not start from its t_init is tried again from there -- one
                 call over those pairs only
    Every stage is ONE call of `align` with a start per pair.  Returns per pair (success, transform, type, candidates, stages);
    stages lists dict(name, shape (of the optical frame), start, type, success) for each stage the pair went through: name
    'pyramid<i>' (level i of pyramid_levels, 1 = half size), 'smoothing', 'final', 'retry'.
    alignment/model reaches `align` with the other keys.  scale_transform is the same for every model: on a level with an odd
    side the scaled start of a similarity is not exactly one, and the optimiser's start is what model_parameters reads from it
    -- row 0 and the translations."""
    transform_model(params.get('alignment/model', 'homography'))
    if not params.get('perspective', True):
        raise NotImplementedError('perspective: false -- ' + _AFFINE)
    if params.get('alignment/decomposed_transformation', False):
        raise NotImplementedError('alignment/decomposed_transformation: ' + _AFFINE)
    T0 = np.array(t_init, np.float64).reshape(-1, 3, 3)
    B = T0.shape[0]
    if optical.shape[0] != B or thermal.shape[0] != B:
        raise ValueError('one optical frame, thermal frame and initial transform per pair')
    T = T0.copy()
    success = np.ones(B, bool)
    stages = [[] for _ in range(B)]
    last = [(None, None, [])] * B
    full = tuple(optical.shape[-2:])

    def stage(name, opt, th, index, start, filter_images):
        Ts, kinds, cands = align(opt, th, start, params, filter_images)
        for j, b in enumerate(index):
            stages[b].append({'name': name, 'shape': tuple(opt.shape[-2:]), 'start': start[j].copy(), 'type': kinds[j],
                              'success': Ts[j] is not None})
            last[b] = (Ts[j], kinds[j], cands[j])
        return Ts

    everyone = list(range(B))
    if params.get('use_image_pyramid', False):
        plan = pyramid_levels(full[0], full[1], params.get('alignment/filter_size', 5), params.get('alignment/n_pyramid_levels', 2))
        levels = []
        o, t = optical, thermal
        for i, (_, _, k) in enumerate(plan):
            o, t = blur(o, k, True), blur(t, k, True)
            levels.insert(0, (i + 1, o, t))
        for i, o, t in levels:
            shape = tuple(o.shape[-2:])
            start = np.stack([scale_transform(T[b], shape, full, True) for b in everyone])
            Ts = stage('pyramid%d' % i, o, t, everyone, start, False)
            for b in everyone:
                success[b] = Ts[b] is not None
                T[b] = scale_transform(Ts[b], shape, full, False) if success[b] else T0[b]
    if params.get('use_smoothing_stage', False):
        Ts = stage('smoothing', optical, thermal, everyone, T.copy(), True)
        for b in everyone:
            success[b] = Ts[b] is not None
            if success[b]:
                T[b] = Ts[b]
    for b in everyone:
        if not success[b]:
            T[b] = T0[b]
    from_init = [bool((T[b] == T0[b]).all()) for b in everyone]
    Ts = stage('final', optical, thermal, everyone, T.copy(), False)
    again = [b for b in everyone if Ts[b] is None and not from_init[b]]
    if again:
        stage('retry', optical[again], thermal[again], again, T0[again].copy(), False)
    return [(last[b][0] is not None, last[b][0], last[b][1], last[b][2], stages[b]) for b in everyone]


def align_images_mutual_information(optical, thermal, t_init, params, stats=None):
    """ImageAligner.align_images_mutual_information (create_dataset/align_images.py:151-248) on fp32 grey frames, for one pair
    -- optical (Ho, Wo), thermal (H, W), t_init (3, 3) -- or B pairs -- (B, 1, Ho, Wo) or (B, Ho, Wo), (B, 1, H, W) or (B, H, W),
    t_init (3, 3) or (B, 3, 3): run_alignment_stages over align_images and gaussian_blur.  params: the reference's yaml keys --
    use_image_pyramid, use_smoothing_stage (both default off), alignment/n_pyramid_levels (2), alignment/filter_size (5) and
    what align_images reads, alignment/model among them; `perspective: false` and alignment/decomposed_transformation raise
    NotImplementedError;
    alignment/use_multiprocess, alignment/optimization_timeout, show_results and verbose are accepted and ignored.
    Returns (success, transform, type, candidates, stages) for one pair, a list of them for a batch; transform and type
    are None without success.  stats: see align_images."""
    single = optical.dim() == 2
    opt, th = _frames(optical, 'optical'), _frames(thermal, 'thermal')
    B = opt.shape[0]
    T0 = _transforms(t_init)
    if T0.shape[0] == 1:
        T0 = np.broadcast_to(T0, (B, 9))
    if T0.shape[0] != B or th.shape[0] != B:
        raise ValueError('one initial transform, or one per pair')

    def align(o, t, T, p, filter_images):
        return align_images(o, t, T, p, filter_images=filter_images, stats=stats)
    out = run_alignment_stages(opt, th, T0.reshape(B, 3, 3), params, align, gaussian_blur)
    return out[0] if single else out
