"""numpy restatement of the pooled ECC refinement, written from its specification: the model csrc/ecc_pooled.hip
and multipoint_amd.utils.ecc's pooled entries are tested against.  Per-pixel terms, raw sums and their order are those of
ecc_restatement (float64, with its f32 mode); this file adds the masks, the per-pair centring and inclusion, the group solve and
the rejection round.

  mask_radii, grow    the radii a mask's excluded set is grown by, and the growth (a Chebyshev ball is a box)
  static_mask         min == max over the frames of a camera
  pair_sums           the raw sums of one pair over its valid and unmasked pixels
  centred, included   the per-pair quantities and the inclusion rule
  group_solve         one decision of a group from its pairs' sums
  refine_group        the whole iteration of one group
  estimate            refine_group and the rejection round
"""
import numpy as np

import ecc_restatement as E

OK, FEW_VALID, NOT_POSITIVE, LAMBDA, NONFINITE = E.OK, E.FEW_VALID, E.NOT_POSITIVE, E.LAMBDA, E.NONFINITE


def mask_radii(feature='gradient', ksize=5):
    """(R_t, R_o): ksize // 2 for the blur, + 1 for the gradient; the image one more (the packed plane's central differences)."""
    rt = ksize // 2 + (1 if feature == 'gradient' else 0)
    return rt, rt + 1


def grow(mask, R):
    """A use-mask (nonzero = use) with its excluded set grown to every pixel within Chebyshev distance R of an excluded pixel,
    clipped at the frame; uint8 0 / 1."""
    keep = np.asarray(mask) != 0
    H, W = keep.shape
    out = np.ones((H, W), bool)
    for y, x in zip(*np.nonzero(~keep)):
        out[max(y - R, 0):y + R + 1, max(x - R, 0):x + R + 1] = False
    return out.astype(np.uint8)


def static_mask(frames):
    """Use-mask of a camera from its float frames [n][H][W]: 0 where the value is equal in every frame."""
    f = np.asarray(frames)
    return (f.min(axis=0) != f.max(axis=0)).astype(np.uint8)


def kept_pixels(T, template_hw, image_hw, tkeep=None, okeep=None):
    """Among the valid template pixels of E.coordinates, in np.nonzero order: which ones the masks keep.  tkeep [H][W] and okeep
    [Ho][Wo] are GROWN use-masks; an image sample is skipped when any of its four bilinear taps is excluded."""
    H, W = template_hw
    Ho, Wo = image_hw
    xs, ys, _, valid = E.coordinates(T, H, W, Ho, Wo)
    yy, xx = np.nonzero(valid)
    keep = np.ones(len(yy), bool)
    if tkeep is not None:
        keep &= np.asarray(tkeep)[yy, xx] != 0
    if okeep is not None:
        o = np.asarray(okeep) != 0
        x0, y0 = np.floor(xs[valid]).astype(np.int64), np.floor(ys[valid]).astype(np.int64)
        keep &= o[y0, x0] & o[y0, x0 + 1] & o[y0 + 1, x0] & o[y0 + 1, x0 + 1]
    return keep


def pair_sums(planes, template, T, model, tkeep=None, okeep=None, f32=False, magnitudes=False):
    """E.sums over the kept set."""
    w, r, G, wm, gm = E.pixel_terms(planes, template, T, model, f32)
    keep = kept_pixels(T, template.shape, planes[0].shape, tkeep, okeep)
    s = E._assemble(w[keep], r[keep], G[:, keep])
    if not magnitudes:
        return s
    m = E._assemble(wm[keep], np.abs(r[keep]), gm[:, keep])
    m[0] = 0.0
    return s, m


def centred(s, K):
    """dict(n, ww, rr, corr, A [K][K], ip [K], tp [K]) of one pair's sums."""
    n, (Sw, Sr, Sww, Srr, Swr), SG, A, SGw, SGr = E.unpack(np.asarray(s, np.float64), K)
    with np.errstate(all='ignore'):
        mw, mr = Sw / n, Sr / n
        return dict(n=n, ww=Sww - n * mw * mw, rr=Srr - n * mr * mr, corr=Swr - n * mw * mr, A=A, ip=SGw - mw * SG,
                    tp=SGr - mr * SG)


def included(s, q, M, min_valid, active=True):
    return bool(active and q['n'] >= min_valid * M and np.isfinite(s).all() and q['ww'] > 0 and q['rr'] > 0)


def group_solve(pair_sums_list, T, model, M, rho_prev=np.nan, eps=1e-6, min_valid=0.25, active=None):
    """One decision of a group from the raw sums of its pairs (in pair order): (status or None while running, T_next, rho,
    converged, rho_i [P] with NaN for a pair that is not included, included [P])."""
    K = E.PARAMS[model]
    P = len(pair_sums_list)
    active = [True] * P if active is None else list(active)
    q = [centred(s, K) for s in pair_sums_list]
    inc = np.array([included(pair_sums_list[i], q[i], M, min_valid, active[i]) for i in range(P)], bool)
    rho_i = np.array([q[i]['corr'] / (np.sqrt(q[i]['ww']) * np.sqrt(q[i]['rr'])) if inc[i] else np.nan for i in range(P)])
    if not inc.any():
        return FEW_VALID, T, np.nan, False, rho_i, inc
    WW = RR = C = 0.0
    A, ip, tp = np.zeros((K, K)), np.zeros(K), np.zeros(K)
    for i in np.nonzero(inc)[0]:                               # ascending pair index
        WW, RR, C = WW + q[i]['ww'], RR + q[i]['rr'], C + q[i]['corr']
        A, ip, tp = A + q[i]['A'], ip + q[i]['ip'], tp + q[i]['tp']
    with np.errstate(all='ignore'):
        rho = C / (np.sqrt(WW) * np.sqrt(RR))
    if not np.isfinite(rho):
        return NONFINITE, T, np.nan, False, rho_i, inc
    if abs(rho - rho_prev) < eps:
        return OK, T, rho, True, rho_i, inc
    L = E.cholesky(A)
    if L is None:
        return NOT_POSITIVE, T, rho, False, rho_i, inc
    y, z = np.linalg.solve(L, ip), np.linalg.solve(L, tp)
    lam_n, lam_d = WW - y @ y, C - z @ y
    if not (np.isfinite(lam_n) and np.isfinite(lam_d)):
        return NONFINITE, T, rho, False, rho_i, inc
    if lam_d <= 0.0:
        return LAMBDA, T, rho, False, rho_i, inc
    dp = np.linalg.solve(L.T, (lam_n / lam_d) * z - y)
    Tn = E.updated(T, dp, model)
    if not np.isfinite(Tn).all():
        return NONFINITE, T, rho, False, rho_i, inc
    return None, Tn, rho, False, rho_i, inc


def refine_group(planes, templates, T0, model='similarity', eps=1e-6, maxiter=50, min_valid=0.25, f32=False, tkeep=None,
                 okeep=None, active=None, history=None, start=True):
    """The refinement of one group: planes [P] of (f, gx, gy), templates [P]; tkeep / okeep grown use-masks or None.  Returns
    dict(transform, rho, nit, success, converged, status, rho_pair, valid_pair, included); history receives (T, rho)."""
    T = E.start_transform(T0, model) if start else np.array(T0, np.float64).reshape(3, 3)
    HW = templates[0].shape[0] * templates[0].shape[1]
    M = HW if tkeep is None else int(np.count_nonzero(tkeep))
    rho_prev, rho_last, nit = np.nan, np.nan, 0
    while True:
        sums = [pair_sums(planes[i], templates[i], T, model, tkeep, okeep, f32) for i in range(len(planes))]
        status, Tn, rho, conv, rho_i, inc = group_solve(sums, T, model, M, rho_prev, eps, min_valid, active)
        if np.isfinite(rho):
            rho_last = rho
        if history is not None:
            history.append((T.copy(), rho))
        out = dict(rho=rho_last, rho_pair=rho_i, valid_pair=np.array([s[0] for s in sums]), included=inc)
        if status is not None:
            return dict(out, transform=T, nit=nit, success=status == OK, converged=conv, status=status)
        T, rho_prev, nit = Tn, rho, nit + 1
        if nit >= maxiter:
            return dict(out, transform=T, nit=nit, success=True, converged=False, status=OK)


def estimate(planes, templates, T0, model='similarity', eps=1e-6, maxiter=50, min_valid=0.25, f32=False, tkeep=None, okeep=None,
             active=None, reject_ratio=0.5):
    """refine_group and the rejection round: the result of the last run with `rejected` [P] and `first`, the first run's."""
    P = len(planes)
    active = np.ones(P, bool) if active is None else np.asarray(active, bool)
    first = refine_group(planes, templates, T0, model, eps, maxiter, min_valid, f32, tkeep, okeep, active)
    first = dict(first, rejected=np.zeros(P, bool), first=None)
    inc = first['included']
    if reject_ratio == 0.0 or not first['success'] or not inc.any():
        return first
    m = float(np.median(first['rho_pair'][inc]))
    if not m > 0.0:
        return first
    stay = inc & (np.where(inc, first['rho_pair'], -np.inf) >= reject_ratio * m)
    if not stay.any() or (stay == active).all():
        return first
    second = refine_group(planes, templates, first['transform'], model, eps, maxiter, min_valid, f32, tkeep, okeep, stay,
                          start=False)
    return dict(second, rejected=active & ~stay, first=first)
