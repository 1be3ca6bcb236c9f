"""Local residual field: a displacement and a confidence for every window of an ALIGNED pair, measured on the
GPU (csrc/residual.hip) on the gradient-magnitude features of utils.ecc, reduced on the host to a few robust numbers per pair and
to a proposed decision for check_alignment.py.  An extension: the reference reviews every pair by eye.

    residual_field(optical_aligned, thermal, window=32, stride=16, radius=8, ...)   -> dict of numpy arrays
    residual_field_from_features(optical_feat, thermal_feat, mask=None, ...)        the same on given feature frames
    confident_windows(field, min_rho, min_margin)                                   -> bool (B, gy, gx)
    summarize_residual_field(field, min_rho, min_margin, tol_px)                    -> one dict per frame
    propose_decision(summary, thresholds)                                           -> 'a', 'r' or '?'

Convention: thermal[p] ~ optical_aligned[p + d], d = (dy, dx) in pixels: the residual misalignment of the optical frame at that
window.  The proposal is a sorting aid, not a verdict: every default threshold below is a guess (no recording was available to set
them on), and propose_decision never decides a pair whose windows are mostly featureless."""
import ctypes

import numpy as np
import torch

from .. import _lib
from .alignment import _frames
from .ecc import _mask_tensor, ecc_features, ecc_mask_radii, grow_mask

__all__ = ['residual_field', 'residual_field_from_features', 'confident_windows', 'summarize_residual_field', 'propose_decision',
           'RES_OK', 'RES_FEW_VALID', 'RES_FLAT', 'RES_AT_EDGE', 'RESIDUAL_WINDOWS', 'RESIDUAL_THRESHOLDS']

RES_OK, RES_FEW_VALID, RES_FLAT, RES_AT_EDGE = 0, 1, 2, 3                          # MP_RES_*
RESIDUAL_WINDOWS = (8, 16, 24, 32, 48, 64)
# guesses, all of them: the confidence rule of a window and the decision rule of a pair
RESIDUAL_THRESHOLDS = {'min_rho': 0.5, 'min_margin': 0.05, 'tol_px': 1.5, 'min_coverage': 0.25, 'accept_median_px': 1.0,
                       'accept_p90_px': 2.0, 'reject_median_px': 2.5}
# variance floor of a window side, in squared feature units: frames are in [0, 1], so one grey level of an 8-bit source is 1 / 255
# and its central difference at most half of that; a window whose gradient magnitude varies by less than a twentieth of this
# ((0.05 * 0.5 / 255)^2 ~ 1e-8) carries quantisation noise, not structure.  A guess like the thresholds above.
VAR_FLOOR = 1e-8


def _check_parameters(window, stride, radius, min_valid, var_floor):
    window, stride, radius = int(window), int(stride), int(radius)
    min_valid, var_floor = float(min_valid), float(var_floor)
    if window not in RESIDUAL_WINDOWS:
        raise ValueError('window must be one of %s, got %s' % (RESIDUAL_WINDOWS, window))
    if stride < 1:
        raise ValueError('stride must be positive, got %s' % (stride,))
    if not 1 <= radius <= 8:
        raise ValueError('radius must be in [1, 8], got %s' % (radius,))
    if not 0.0 < min_valid <= 1.0:
        raise ValueError('min_valid must be in (0, 1], got %s' % (min_valid,))
    if not (var_floor >= 0.0 and np.isfinite(var_floor)):
        raise ValueError('var_floor must be finite and not negative, got %s' % (var_floor,))
    return window, stride, radius, min_valid, var_floor


def residual_field_from_features(optical_feat, thermal_feat, mask=None, window=32, stride=16, radius=8, min_valid=0.5,
                                 var_floor=VAR_FLOOR):
    """The residual field of feature frames (fp32 CUDA (H, W), (B, H, W) or (B, 1, H, W), e.g. ecc_features' output) with a
    use-mask on the optical side ((H, W) shared or (B, H, W), bool or uint8, nonzero = use; taken as it is) or None.  Returns the
    dict of residual_field.  ValueError: what mp_residual_field refuses (include/multipoint_hip.h)."""
    window, stride, radius, min_valid, var_floor = _check_parameters(window, stride, radius, min_valid, var_floor)
    fo, ft = _frames(optical_feat, 'optical_feat'), _frames(thermal_feat, 'thermal_feat')
    if fo.shape != ft.shape or fo.device != ft.device:
        raise ValueError('the two feature stacks must have one shape and device, got %s and %s' % (tuple(fo.shape), tuple(ft.shape)))
    B, H, W = ft.shape
    m = None
    if mask is not None:
        m = _mask_tensor(mask, 'mask', ft.device)
        if tuple(m.shape[1:]) != (H, W) or m.shape[0] not in (1, B) or m.device != ft.device:
            raise ValueError('mask must be (H, W) or (B, H, W) = %s on the frames\' device, got %s' % ((B, H, W), tuple(m.shape)))
    h = _lib.get_handle(ft.device)
    gy, gx = _lib.c_int(), _lib.c_int()
    if h.lib.mp_residual_grid(H, W, window, stride, radius, ctypes.byref(gy), ctypes.byref(gx)) != _lib.MP_OK:
        raise ValueError('residual field: a %d x %d frame holds no window of %d + 2 x %d pixels (frames are 8 x 8 to 4096 x 4096)'
                         % (H, W, window, radius))
    gy, gx = gy.value, gx.value
    out_d = torch.empty((B, gy, gx, 5), dtype=torch.float64, device=ft.device)
    out_i = torch.empty((B, gy, gx, 2), dtype=torch.int32, device=ft.device)
    h.check(h.lib.mp_residual_field(h.ptr, _lib.ptr(fo), _lib.ptr(ft), _lib.ptr(m), 1 if m is None else m.shape[0], B, H, W, window,
                                    stride, radius, min_valid, var_floor, _lib.ptr(out_d), _lib.ptr(out_i),
                                    _lib.stream_ptr(ft.device)))
    d, i = out_d.cpu().numpy(), out_i.cpu().numpy()
    ys, xs = radius + stride * np.arange(gy), radius + stride * np.arange(gx)
    return {'d': np.ascontiguousarray(d[..., 0:2]), 'rho': np.ascontiguousarray(d[..., 2]), 'rho0': np.ascontiguousarray(d[..., 3]),
            'second': np.ascontiguousarray(d[..., 4]), 'n': np.ascontiguousarray(i[..., 0]), 'status': np.ascontiguousarray(i[..., 1]),
            'origin': np.stack(np.meshgrid(ys, xs, indexing='ij'), -1), 'window': window, 'stride': stride, 'radius': radius}


def residual_field(optical_aligned, thermal, window=32, stride=16, radius=8, feature='gradient', ksize=5, optical_mask=None,
                   min_valid=0.5, var_floor=VAR_FLOOR):
    """The local residual field of aligned pairs: frames as in utils.ecc (fp32 CUDA (H, W), (B, H, W) or (B, 1, H, W), both of one
    size), features from ecc_features(., feature, ksize).  optical_mask ((H, W) for all pairs or (B, H, W), nonzero = use) marks
    the pixels of the ALIGNED optical frame that hold image content; its excluded set is grown by ecc_mask_radii(feature,
    ksize)[1] first, so that no kept feature saw an excluded pixel.

    Windows of window x window pixels (8, 16, 24, 32, 48 or 64) start at radius + i * stride in both axes while the search region
    of +-radius (1..8) stays inside the frame.  For every displacement the zero-mean normalised cross-correlation is taken over the
    window pixels the mask keeps; it is undefined with fewer than min_valid * window^2 of them, or when a side's centred sum of
    squares is <= var_floor times their number.

    Returns numpy arrays: d (B, gy, gx, 2) = (dy, dx) of the best displacement with a per-axis parabola refinement, rho (its
    score), rho0 (the score at d = 0), second (the best score outside the 3 x 3 block around the peak, -inf if none), n (pixels
    used at the peak), status (RES_OK, RES_FEW_VALID, RES_FLAT, RES_AT_EDGE; d and the scores are NaN for the middle two) and
    origin (gy, gx, 2), the (y, x) of every window's first pixel; window, stride and radius are carried along as ints."""
    _check_parameters(window, stride, radius, min_valid, var_floor)
    o, t = _frames(optical_aligned, 'optical_aligned'), _frames(thermal, 'thermal')
    if o.shape != t.shape or o.device != t.device:
        raise ValueError('optical_aligned and thermal must have one shape and device, got %s and %s'
                         % (tuple(o.shape), tuple(t.shape)))
    m = None
    if optical_mask is not None:
        m = _mask_tensor(optical_mask, 'optical_mask', t.device)
        if tuple(m.shape[1:]) != tuple(t.shape[1:]) or m.shape[0] not in (1, t.shape[0]):
            raise ValueError('optical_mask must be (H, W) or (B, H, W) = %s, got %s' % (tuple(t.shape), tuple(m.shape)))
        m = grow_mask(m, ecc_mask_radii(feature, ksize)[1])
    return residual_field_from_features(ecc_features(o, feature, ksize), ecc_features(t, feature, ksize), m, window, stride, radius,
                                        min_valid, var_floor)


def confident_windows(field, min_rho=RESIDUAL_THRESHOLDS['min_rho'], min_margin=RESIDUAL_THRESHOLDS['min_margin']):
    """bool (B, gy, gx): status RES_OK, rho >= min_rho and rho - second >= min_margin."""
    rho, second = np.asarray(field['rho'], np.float64), np.asarray(field['second'], np.float64)
    with np.errstate(invalid='ignore'):
        return (np.asarray(field['status']) == RES_OK) & (rho >= float(min_rho)) & (rho - second >= float(min_margin))


def summarize_residual_field(field, min_rho=RESIDUAL_THRESHOLDS['min_rho'], min_margin=RESIDUAL_THRESHOLDS['min_margin'],
                             tol_px=RESIDUAL_THRESHOLDS['tol_px']):
    """One dict per frame, float64 on the host: windows, confident (counts), coverage = confident / windows, median_d [dy, dx]
    (component-wise over the confident windows), median_mag and p90_mag (median and 90th percentile, numpy's linear method, of
    |d|), outlier_share (confident windows with |d| > tol_px over confident), at_edge (windows with RES_AT_EDGE) and median_rho0
    (over the windows whose rho0 is defined).  A frame without a confident window has NaN in the d terms and outlier_share."""
    conf = confident_windows(field, min_rho, min_margin)
    d = np.asarray(field['d'], np.float64)
    status, rho0 = np.asarray(field['status']), np.asarray(field['rho0'], np.float64)
    nan = float('nan')
    out = []
    for b in range(conf.shape[0]):
        c = conf[b]
        windows, confident = int(c.size), int(c.sum())
        r0 = rho0[b][np.isfinite(rho0[b])]
        s = {'windows': windows, 'confident': confident, 'coverage': confident / windows if windows else 0.0,
             'median_d': [nan, nan], 'median_mag': nan, 'p90_mag': nan, 'outlier_share': nan,
             'at_edge': int((status[b] == RES_AT_EDGE).sum()), 'median_rho0': float(np.median(r0)) if r0.size else nan}
        if confident:
            dc = d[b][c]
            mag = np.hypot(dc[:, 0], dc[:, 1])
            s.update(median_d=[float(np.median(dc[:, 0])), float(np.median(dc[:, 1]))], median_mag=float(np.median(mag)),
                     p90_mag=float(np.percentile(mag, 90)), outlier_share=float((mag > float(tol_px)).sum()) / confident)
        out.append(s)
    return out


def propose_decision(summary, thresholds=None):
    """'a', 'r' or '?' for one frame's summary: '?' when coverage < min_coverage (the pre-screen never decides a featureless
    pair); 'a' when median_mag <= accept_median_px and p90_mag <= accept_p90_px; 'r' when median_mag >= reject_median_px; '?'
    otherwise (NaN compares false everywhere).  thresholds: a dict with those four keys; missing ones come from
    RESIDUAL_THRESHOLDS."""
    t = dict(RESIDUAL_THRESHOLDS)
    t.update(thresholds or {})
    if not summary['coverage'] >= float(t['min_coverage']) or summary['confident'] == 0:
        return '?'
    if summary['median_mag'] <= float(t['accept_median_px']) and summary['p90_mag'] <= float(t['accept_p90_px']):
        return 'a'
    if summary['median_mag'] >= float(t['reject_median_px']):
        return 'r'
    return '?'
