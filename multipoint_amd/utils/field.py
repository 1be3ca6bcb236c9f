"""Local alignment correction: fit a smooth displacement field to the windows of a local residual field
(utils.residual), sample the optical frame through it, measure again and iterate.  The kernels are csrc/field.hip.  An extension: the
reference models a pair with one global transform and leaves what remains to the reviewer.

    field_geometry(field)                                   -> (y0, x0, step) of the lattice of window centres
    field_weights(field, min_rho, min_margin, mode)         -> float64 (B, gy, gx): 1 (or rho) on confident windows, 0 elsewhere
    fit_displacement_field(field, weights, smoothness, ...) -> (u float64 (B, gy, gx, 2), info) on the host
    warp_by_field(src, u, geometry, ...)                    -> the frames sampled at p + u(p), CUDA tensors
    never_worse(first, final, ...)                          -> (applied, reason) for one frame's first and last summary
    correct_locally(optical_aligned, thermal, rounds=3, ...)   the loop, with the never-worse rule

Convention, as in utils.residual: thermal[p] ~ optical_aligned[p + d], so the corrected frame is optical_aligned[p + u(p)].

Every default below (smoothness 0.25, min_initial_px 0.25, keep_confident 0.8, linear extrapolation, three rounds) is a guess from
one planted 96 x 128 trial; no recording was available to set them on, and nothing here is a claim about real recordings.  A residual
of `radius` pixels or more shows as RES_AT_EDGE in the measurement, is never confident and is therefore not corrected."""
import ctypes

import numpy as np
import torch

from .. import _lib
from .alignment import _frames
from .residual import RESIDUAL_THRESHOLDS, VAR_FLOOR, confident_windows, residual_field, summarize_residual_field

__all__ = ['field_geometry', 'field_weights', 'fit_displacement_field', 'warp_by_field', 'never_worse', 'correct_locally',
           'FIELD_OK', 'FIELD_NO_DATA', 'FIELD_ALL_REJECTED', 'FIELD_MAX_ITER', 'FIELD_DEFAULTS']

FIELD_OK, FIELD_NO_DATA, FIELD_ALL_REJECTED, FIELD_MAX_ITER = 0, 1, 2, 3            # MP_FIELD_*
# guesses, all of them
FIELD_DEFAULTS = {'smoothness': 0.25, 'min_initial_px': 0.25, 'keep_confident': 0.8, 'extrapolate': 'linear', 'rounds': 3}
_EXTRAPOLATE = {'clamp': 0, 'linear': 1}


def field_geometry(field):
    """(y0, x0, step) of a residual_field dict: node (i, j) of the lattice is the centre of window (i, j), origin + (window - 1) / 2,
    and neighbouring nodes are `stride` pixels apart."""
    origin = np.asarray(field['origin'], np.float64)
    half = (int(field['window']) - 1) / 2.0
    return float(origin[0, 0, 0]) + half, float(origin[0, 0, 1]) + half, float(int(field['stride']))


def field_weights(field, min_rho=RESIDUAL_THRESHOLDS['min_rho'], min_margin=RESIDUAL_THRESHOLDS['min_margin'], mode='binary'):
    """float64 (B, gy, gx): 1 ('binary') or rho ('rho') on the confident windows (the rule of confident_windows), 0 elsewhere."""
    if mode not in ('binary', 'rho'):
        raise ValueError("mode must be 'binary' or 'rho', got %r" % (mode,))
    conf = confident_windows(field, min_rho, min_margin)
    if mode == 'binary':
        return conf.astype(np.float64)
    return np.where(conf, np.asarray(field['rho'], np.float64), 0.0)


def _check_fit(smoothness, robust_px, rounds, tol, max_iter, nodes):
    smoothness, tol, rounds = float(smoothness), float(tol), int(rounds)
    robust_px = 0.0 if robust_px is None else float(robust_px)
    max_iter = min(1 << 20, 4 * nodes + 64) if max_iter is None else int(max_iter)
    if not (smoothness > 0.0 and np.isfinite(smoothness)):
        raise ValueError('smoothness must be positive and finite, got %s' % (smoothness,))
    if not (robust_px >= 0.0 and np.isfinite(robust_px)):
        raise ValueError('robust_px must be finite and not negative (None or 0: off), got %s' % (robust_px,))
    if not (tol >= 0.0 and np.isfinite(tol)):
        raise ValueError('tol must be finite and not negative, got %s' % (tol,))
    if not 0 <= rounds <= 16:
        raise ValueError('rounds must be in [0, 16], got %s' % (rounds,))
    if not 1 <= max_iter <= 1 << 20:
        raise ValueError('max_iter must be in [1, 2^20], got %s' % (max_iter,))
    return smoothness, robust_px, rounds, tol, max_iter


def fit_displacement_field(field, weights=None, smoothness=FIELD_DEFAULTS['smoothness'], robust_px=None, rounds=2, tol=1e-12,
                           max_iter=None, device=None):
    """The smooth field of a lattice of measured displacements, solved on the GPU (mp_field_fit, include/multipoint_hip.h): per
    frame and axis the minimiser of sum_k w_k (u_k - d_k)^2 + smoothness sum_edges (u_k - u_l)^2 over the 4-neighbour lattice.

    field: a residual_field dict, or its d alone (B, gy, gx, 2) -- then weights must be given.  weights (B, gy, gx), >= 0; None:
    field_weights(field) with its defaults.  d is not read where the weight is 0 (NaN is fine there).  robust_px (None or 0: off)
    and rounds: after each of the first `rounds` solves the weights become w0 (1 - (e / robust_px)^2)^2 of the residual e = |u - d|,
    0 from robust_px on, and the system is solved again from the previous solution.  tol: the conjugate gradients stop at
    |r| <= tol |b|; max_iter: None is 4 nodes + 64.

    Returns (u float64 (B, gy, gx, 2), info) as numpy: info has status (B,) (FIELD_OK, FIELD_NO_DATA: no weight, u = 0;
    FIELD_ALL_REJECTED: a robust round left no weight, the solution before it is kept; FIELD_MAX_ITER), iterations and residual of
    the last solve, nonzero (nodes with a weight in the returned solution's system), nonfinite (weighted nodes whose d was not
    finite: taken as weight 0) and weight (B, gy, gx), the final weights."""
    if isinstance(field, dict):
        d = np.asarray(field['d'], np.float64)
        w = field_weights(field) if weights is None else np.asarray(weights, np.float64)
    else:
        d = np.asarray(field, np.float64)
        if weights is None:
            raise ValueError('weights must be given with a bare array of displacements')
        w = np.asarray(weights, np.float64)
    if d.ndim != 4 or d.shape[3] != 2 or w.shape != d.shape[:3]:
        raise ValueError('d must be (B, gy, gx, 2) and weights (B, gy, gx), got %s and %s' % (d.shape, w.shape))
    B, gy, gx = w.shape
    smoothness, robust_px, rounds, tol, max_iter = _check_fit(smoothness, robust_px, rounds, tol, max_iter, gy * gx)
    dev = _lib.require_cuda(device)
    h = _lib.get_handle(dev)
    size = _lib.c_ll()
    if h.lib.mp_field_fit_workspace(B, gy, gx, ctypes.byref(size)) != _lib.MP_OK:
        raise ValueError('field fit: B must be in [1, 65535] and the lattice sides in [1, 256], got %d frames of %d x %d' % (B, gy, gx))
    dd = torch.from_numpy(np.ascontiguousarray(d)).to(dev)
    ww = torch.from_numpy(np.ascontiguousarray(w)).to(dev)
    ws = torch.empty((max(size.value, 16) + 7) // 8, dtype=torch.float64, device=dev)
    out_u = torch.empty((B, gy, gx, 2), dtype=torch.float64, device=dev)
    out_i = torch.empty((B, 4), dtype=torch.int32, device=dev)
    out_r = torch.empty((B,), dtype=torch.float64, device=dev)
    out_w = torch.empty((B, gy, gx), dtype=torch.float64, device=dev)
    h.check(h.lib.mp_field_fit(h.ptr, _lib.ptr(dd), _lib.ptr(ww), B, gy, gx, smoothness, robust_px, rounds, tol, max_iter, _lib.ptr(ws),
                               ws.numel() * 8, _lib.ptr(out_u), _lib.ptr(out_i), _lib.ptr(out_r), _lib.ptr(out_w),
                               _lib.stream_ptr(dev)))
    i = out_i.cpu().numpy()
    info = {'status': i[:, 0].copy(), 'iterations': i[:, 1].copy(), 'nonzero': i[:, 2].copy(), 'nonfinite': i[:, 3].copy(),
            'residual': out_r.cpu().numpy(), 'weight': out_w.cpu().numpy()}
    return out_u.cpu().numpy(), info


def warp_by_field(src, u, geometry, shape=None, homography=None, extrapolate=FIELD_DEFAULTS['extrapolate'], return_valid=False):
    """Frames sampled through a displacement field (mp_field_warp): dst[b][p] = src[q] bilinearly, q = p + u_b(p), or with
    `homography` q = H_b (p + u_b(p)) -- H (3, 3) or (B, 3, 3), row-major on (x, y, 1), maps the displaced output position into the
    source, so the RAW optical frame can be sampled once instead of an already warped one a second time.

    src: fp32 CUDA (Hs, Ws), (n, Hs, Ws) or (n, 1, Hs, Ws) with n 1 or B; u: float64 (B, gy, gx, 2) or (gy, gx, 2), numpy or CUDA;
    geometry: (y0, x0, step) as field_geometry gives it; shape: (H, W) of the output (None: the source's); extrapolate: 'linear'
    continues the border cells' slope outside the lattice, 'clamp' holds the border value.  Taps outside the source read 0.
    Returns dst fp32 (B, H, W), with return_valid also uint8 (B, H, W): 1 where every tap that counts lies inside the source."""
    s = _frames(src, 'src')
    if extrapolate not in _EXTRAPOLATE:
        raise ValueError("extrapolate must be 'clamp' or 'linear', got %r" % (extrapolate,))
    uu = u if isinstance(u, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(u, np.float64)))
    if uu.dim() == 3:
        uu = uu[None]
    if uu.dim() != 4 or uu.shape[3] != 2:
        raise ValueError('u must be (B, gy, gx, 2) or (gy, gx, 2), got %s' % (tuple(uu.shape),))
    uu = uu.to(device=s.device, dtype=torch.float64).contiguous()
    B, gy, gx = uu.shape[:3]
    n_src, Hs, Ws = s.shape
    if n_src not in (1, B):
        raise ValueError('src must hold one frame or one per field, got %d for %d' % (n_src, B))
    H, W = (Hs, Ws) if shape is None else (int(shape[0]), int(shape[1]))
    y0, x0, step = (float(v) for v in geometry)
    hom = None
    if homography is not None:
        hm = homography if isinstance(homography, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(homography,
                                                                                                                      np.float64)))
        hm = hm.to(device=s.device, dtype=torch.float64).reshape(-1, 9)
        if hm.shape[0] not in (1, B):
            raise ValueError('homography must be (3, 3) or (B, 3, 3), got %s' % (tuple(homography.shape),))
        hom = hm.expand(B, 9).contiguous()
    dst = torch.empty((B, H, W), dtype=torch.float32, device=s.device)
    valid = torch.empty((B, H, W), dtype=torch.uint8, device=s.device) if return_valid else None
    h = _lib.get_handle(s.device)
    h.check(h.lib.mp_field_warp(h.ptr, _lib.ptr(s), n_src, Hs, Ws, _lib.ptr(uu), gy, gx, y0, x0, step, _EXTRAPOLATE[extrapolate],
                                _lib.ptr(hom), B, H, W, _lib.ptr(dst), _lib.ptr(valid), _lib.stream_ptr(s.device)))
    return (dst, valid) if return_valid else dst


def never_worse(first, final, min_coverage=RESIDUAL_THRESHOLDS['min_coverage'], min_initial_px=FIELD_DEFAULTS['min_initial_px'],
                keep_confident=FIELD_DEFAULTS['keep_confident']):
    """(applied, reason) for one frame from its first and last summary (summarize_residual_field).  The correction is applied only
    if the first coverage reaches min_coverage ('coverage' otherwise: too few windows to fit anything to), the first median
    magnitude is at least min_initial_px ('aligned': nothing to correct), the final median magnitude is smaller than the first
    ('not_improved') and the final measurement keeps at least keep_confident of the first one's confident windows
    ('lost_windows').  NaN fails every comparison; the reason of an applied frame is 'applied'."""
    if first['confident'] == 0 or not first['coverage'] >= float(min_coverage):
        return False, 'coverage'
    if not first['median_mag'] >= float(min_initial_px):
        return False, 'aligned'
    if not final['median_mag'] < first['median_mag']:
        return False, 'not_improved'
    if not final['confident'] >= float(keep_confident) * first['confident']:
        return False, 'lost_windows'
    return True, 'applied'


def correct_locally(optical_aligned, thermal, rounds=FIELD_DEFAULTS['rounds'], window=32, stride=16, radius=8, feature='gradient',
                    ksize=5, optical_mask=None, min_valid=0.5, var_floor=VAR_FLOOR, min_rho=RESIDUAL_THRESHOLDS['min_rho'],
                    min_margin=RESIDUAL_THRESHOLDS['min_margin'], tol_px=RESIDUAL_THRESHOLDS['tol_px'], weight_mode='binary',
                    smoothness=FIELD_DEFAULTS['smoothness'], robust_px=None, robust_rounds=2,
                    extrapolate=FIELD_DEFAULTS['extrapolate'], min_coverage=RESIDUAL_THRESHOLDS['min_coverage'],
                    min_initial_px=FIELD_DEFAULTS['min_initial_px'], keep_confident=FIELD_DEFAULTS['keep_confident'],
                    optical_source=None, homography=None):
    """Correct what one global transform leaves of aligned pairs (frames as in residual_field): `rounds` times, measure the
    residual field of the current optical frame against the thermal one, fit an increment to its confident windows
    (fit_displacement_field) and add it node by node to the accumulated field, U <- U + increment.  That is first-order
    composition -- the increment is measured at p but belongs to p + U(p); the difference is the field's gradient times the
    increment, second order for a smooth field, and the next round measures it.  The frame of every round is the INPUT sampled
    once through U (warp_by_field), never a warped frame warped again; with optical_source (the raw optical frames) and homography
    (thermal pixel -> raw optical pixel, (3, 3) or (B, 3, 3)) the raw frame is sampled at H (p + U(p)) directly, and optical_aligned
    is only measured in round 0.  From round 1 on the pixels without content (valid = 0) are masked out of the measurement,
    together with optical_mask (as in residual_field) if given.

    The never-worse rule (never_worse) decides per frame from the first and the last of the rounds + 1 measurements; a frame
    that is not corrected comes back with its input bits, valid = 1, U = 0 and the reason.

    Returns a dict: corrected fp32 CUDA (B, H, W), valid uint8 CUDA (B, H, W), U float64 numpy (B, gy, gx, 2), geometry (y0, x0,
    step), summaries (rounds + 1 lists of one summarize_residual_field dict per frame), applied (list of bool), reason (list of
    str) and fields (the first and the last residual_field dict)."""
    rounds = int(rounds)
    if rounds < 1:
        raise ValueError('rounds must be at least 1, got %s' % (rounds,))
    o, t = _frames(optical_aligned, 'optical_aligned'), _frames(thermal, 'thermal')
    if o.shape != t.shape or o.device != t.device:
        raise ValueError('optical_aligned and thermal must have one shape and device, got %s and %s' % (tuple(o.shape), tuple(t.shape)))
    if (optical_source is None) != (homography is None):
        raise ValueError('optical_source and homography go together')
    B, H, W = t.shape
    src = o if optical_source is None else _frames(optical_source, 'optical_source')
    from .ecc import _mask_tensor
    given = None if optical_mask is None else _mask_tensor(optical_mask, 'optical_mask', t.device)

    def measure(frames, mask):
        f = residual_field(frames, t, window, stride, radius, feature, ksize, mask, min_valid, var_floor)
        return f, summarize_residual_field(f, min_rho, min_margin, tol_px)
    field, summary = measure(o, given)
    first_field, summaries = field, [summary]
    geometry = field_geometry(field)
    U = np.zeros(field['d'].shape, np.float64)
    current, valid = o, torch.ones((B, H, W), dtype=torch.uint8, device=t.device)
    for _ in range(rounds):
        delta, _info = fit_displacement_field(field, field_weights(field, min_rho, min_margin, weight_mode), smoothness, robust_px,
                                              robust_rounds, device=t.device)
        U += delta
        current, valid = warp_by_field(src, U, geometry, (H, W), homography, extrapolate, True)
        field, summary = measure(current, valid if given is None else valid * given)
        summaries.append(summary)
    applied, reason = [], []
    for b in range(B):
        a, why = never_worse(summaries[0][b], summaries[-1][b], min_coverage, min_initial_px, keep_confident)
        applied.append(a)
        reason.append(why)
    keep = torch.tensor(applied, dtype=torch.bool, device=t.device)[:, None, None]
    corrected = torch.where(keep, current, o)
    valid = torch.where(keep, valid, torch.ones_like(valid))
    U[~np.asarray(applied, bool)] = 0.0
    return {'corrected': corrected, 'valid': valid, 'U': U, 'geometry': geometry, 'summaries': summaries, 'applied': applied,
            'reason': reason, 'fields': (first_field, field)}
