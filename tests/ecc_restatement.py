"""numpy restatement of the ECC direct alignment, written from its specification: the model csrc/ecc.hip and
multipoint_amd.utils.ecc are tested against.  Everything is float64 except the template-to-image coordinates, which repeat the
kernel's fp32 fused multiply-adds (so that both sides agree on which pixels are valid and on the bilinear weights); f32=True
additionally rounds every per-pixel term (the samples and the Jacobian columns) as the kernel does, which measures how far fp32
terms move a trajectory (ecc_cases.noise_floor).

  features          blur (pyramid_restatement.gaussian_blur, bit-exact float32) and the gradient magnitude
  central           central differences with BORDER_REFLECT_101
  coordinates       xs, ys, den and the valid mask of every template pixel
  jacobian          d xs / d p_k, d ys / d p_k of a motion model
  sums              the S sums of one problem, and the magnitude sums an error bound is taken against
  solve             one Gauss-Newton decision from the sums
  refine            the whole iteration
"""
import numpy as np

from pyramid_restatement import gaussian_blur

F32 = np.float32
PARAMS = {'translation': 2, 'similarity': 4, 'affine': 6, 'homography': 8}
OK, FEW_VALID, NOT_POSITIVE, LAMBDA, NONFINITE = 0, 1, 2, 3, 4


def n_sums(K):
    return 6 + K + K * (K + 1) // 2 + 2 * K


def central(f):
    """(gx, gy) = 0.5 (f[x+1] - f[x-1]), 0.5 (f[y+1] - f[y-1]) with BORDER_REFLECT_101, in f's dtype."""
    H, W = f.shape
    xp = np.r_[1:W, W - 2]
    xm = np.r_[1, 0:W - 1]
    yp = np.r_[1:H, H - 2]
    ym = np.r_[1, 0:H - 1]
    half = f.dtype.type(0.5)
    return half * (f[:, xp] - f[:, xm]), half * (f[yp, :] - f[ym, :])


def features(frame, ksize=5, feature='gradient', f32=False):
    """The feature frame of a float32 frame: float64 (float32 with f32: the kernel's operations, one fused multiply-add)."""
    x = np.asarray(frame, F32)
    b = gaussian_blur(x, ksize) if ksize > 1 else x
    if feature == 'intensity':
        return b if f32 else b.astype(np.float64)
    assert feature == 'gradient'
    gx, gy = central(b)                                   # float32, as the kernel rounds them
    gx, gy = gx.astype(np.float64), gy.astype(np.float64)
    if f32:
        return np.sqrt(F32(gx * gx + (gy * gy).astype(F32).astype(np.float64)))
    return np.sqrt(gx * gx + gy * gy)


def image_planes(feat, f32=False):
    """(f, gx, gy) of the optical feature frame."""
    f = np.asarray(feat, F32 if f32 else np.float64)
    gx, gy = central(f)
    return f, gx, gy


def fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def coordinates(T, H, W, Ho, Wo):
    """fp32 (xs, ys, den) of every template pixel [H][W] and the valid mask: the kernel's fused multiply-adds and divisions."""
    m = np.asarray(T, np.float64).reshape(9).astype(F32)
    y, x = np.mgrid[0:H, 0:W]
    x, y = x.astype(F32), y.astype(F32)
    with np.errstate(all='ignore'):
        X = fma32(m[0], x, fma32(m[1], y, m[2]))
        Y = fma32(m[3], x, fma32(m[4], y, m[5]))
        D = fma32(m[6], x, fma32(m[7], y, m[8]))
        xs, ys = X / D, Y / D
        x0, y0 = np.floor(xs), np.floor(ys)
        valid = (x0 >= 0) & (y0 >= 0) & (x0 <= Wo - 2) & (y0 <= Ho - 2)
    return xs, ys, D, valid


def warp(T, x, y):
    """float64 image coordinates of template points under T."""
    T = np.asarray(T, np.float64).reshape(3, 3)
    den = T[2, 0] * x + T[2, 1] * y + T[2, 2]
    return (T[0, 0] * x + T[0, 1] * y + T[0, 2]) / den, (T[1, 0] * x + T[1, 1] * y + T[1, 2]) / den


def jacobian(model, x, y, xs, ys, den):
    """(dxs [K][...], dys [K][...]): the derivatives of the image coordinates by the model's parameters."""
    one, zero = np.ones_like(x), np.zeros_like(x)
    if model == 'translation':
        return np.stack([one, zero]), np.stack([zero, one])
    if model == 'similarity':
        return np.stack([x, -y, one, zero]), np.stack([y, x, zero, one])
    if model == 'affine':
        return np.stack([x, y, one, zero, zero, zero]), np.stack([zero, zero, zero, x, y, one])
    assert model == 'homography'
    return (np.stack([x, y, one, zero, zero, zero, -xs * x, -xs * y]) / den,
            np.stack([zero, zero, zero, x, y, one, -ys * x, -ys * y]) / den)


def parameters(T, model):
    T = np.asarray(T, np.float64).reshape(3, 3)
    if model == 'translation':
        return np.array([T[0, 2], T[1, 2]])
    if model == 'similarity':
        return np.array([T[0, 0], T[1, 0], T[0, 2], T[1, 2]])
    if model == 'affine':
        return T[:2].reshape(6).copy()
    return T.reshape(9)[:8].copy()


def updated(T, dp, model):
    """T with the additive update dp of the model's parameters."""
    T = np.array(T, np.float64).reshape(3, 3)
    if model == 'translation':
        T[0, 2] += dp[0]; T[1, 2] += dp[1]
    elif model == 'similarity':
        a, b = T[0, 0] + dp[0], T[1, 0] + dp[1]
        T[0, 0] = T[1, 1] = a
        T[0, 1], T[1, 0] = -b, b
        T[0, 2] += dp[2]; T[1, 2] += dp[3]
    elif model == 'affine':
        T[:2] += np.asarray(dp).reshape(2, 3)
    else:
        T.reshape(9)[:8] += dp
    return T


def start_transform(T0, model):
    """The start of a refinement: T0 / T0[2,2]; a similarity from (angle, scale, dx, dy) of row 0, an affine map from the top
    two rows (utils.alignment.model_parameters and model_transform on the host)."""
    T = np.array(T0, np.float64).reshape(3, 3)
    T = T / T[2, 2]
    if model == 'similarity':
        ang, sc = np.arctan2(T[0, 1], T[0, 0]), np.hypot(T[0, 0], T[0, 1])
        c, s = sc * np.cos(ang), sc * np.sin(ang)
        return np.array([[c, s, T[0, 2]], [-s, c, T[1, 2]], [0.0, 0.0, 1.0]])
    if model == 'affine':
        T[2] = (0.0, 0.0, 1.0)
    return T


def _taps(plane, x0, y0):
    return plane[y0, x0], plane[y0, x0 + 1], plane[y0 + 1, x0], plane[y0 + 1, x0 + 1]


def _lerp(t, fx, fy, f32):
    p00, p01, p10, p11 = t
    if f32:
        top = fma32(fx, p01 - p00, p00)
        bot = fma32(fx, p11 - p10, p10)
        return fma32(fy, bot - top, top)
    top = p00 + fx * (p01 - p00)
    bot = p10 + fx * (p11 - p10)
    return top + fy * (bot - top)


def pixel_terms(planes, template, T, model, f32=False):
    """Per valid pixel: w, r, G [K] (float64 arrays; with f32 every one of them rounded as the kernel rounds it), and the
    magnitudes wm, gm [K] a rounding-error bound is taken against: the largest |tap| in place of the interpolated value."""
    f, gxp, gyp = planes
    Ho, Wo = f.shape
    H, W = template.shape
    xs, ys, den, valid = coordinates(T, H, W, Ho, Wo)
    yy, xx = np.nonzero(valid)
    xs, ys, den = xs[valid], ys[valid], den[valid]
    x0f, y0f = np.floor(xs), np.floor(ys)
    fx, fy = xs - x0f, ys - y0f                                           # exact in fp32
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    ft = F32 if f32 else np.float64
    fx, fy, xs, ys, den = (v.astype(ft) for v in (fx, fy, xs, ys, den))
    x, y = xx.astype(ft), yy.astype(ft)
    tw, tx, ty = _taps(f, x0, y0), _taps(gxp, x0, y0), _taps(gyp, x0, y0)
    w, gx, gy = _lerp(tw, fx, fy, f32), _lerp(tx, fx, fy, f32), _lerp(ty, fx, fy, f32)
    r = np.asarray(template)[yy, xx]
    if f32:
        if model == 'translation':
            G = [gx, gy]
        elif model == 'similarity':
            G = [fma32(gx, x, gy * y), fma32(gy, x, -(gx * y)), gx, gy]
        elif model == 'affine':
            G = [gx * x, gx * y, gx, gy * x, gy * y, gy]
        else:
            inv = F32(1.0) / den
            a, c = gx * inv, gy * inv
            t = -fma32(a, xs, c * ys)
            G = [a * x, a * y, a, c * x, c * y, c, t * x, t * y]
        G = np.stack([np.asarray(g, F32) for g in G]).astype(np.float64)
    else:
        dxs, dys = jacobian(model, x, y, xs, ys, den)
        G = gx * dxs + gy * dys
    wm = np.max(np.abs(np.stack(tw)), axis=0).astype(np.float64)
    gxm = np.max(np.abs(np.stack(tx)), axis=0).astype(np.float64)
    gym = np.max(np.abs(np.stack(ty)), axis=0).astype(np.float64)
    d64 = [v.astype(np.float64) for v in (x, y, xs, ys, den)]
    dxs, dys = jacobian(model, *d64)
    gm = gxm * np.abs(dxs) + gym * np.abs(dys)
    return w.astype(np.float64), r.astype(np.float64), G, wm, gm


def _assemble(w, r, G):
    K = G.shape[0]
    out = [float(len(w)), w.sum(), r.sum(), (w * w).sum(), (r * r).sum(), (w * r).sum()]
    out += [G[k].sum() for k in range(K)]
    out += [(G[k] * G[l]).sum() for k in range(K) for l in range(k, K)]
    out += [(G[k] * w).sum() for k in range(K)]
    out += [(G[k] * r).sum() for k in range(K)]
    return np.array(out, np.float64)


def sums(planes, template, T, model, f32=False, magnitudes=False):
    """The sums of one problem in the kernel's order: n, w, r, ww, rr, wr, G_k, G_k G_l (k <= l, row by row), G_k w, G_k r.
    magnitudes: also the same sums over the terms' magnitudes (their first entry is 0: the count is exact)."""
    w, r, G, wm, gm = pixel_terms(planes, template, T, model, f32)
    s = _assemble(w, r, G)
    if not magnitudes:
        return s
    m = _assemble(wm, np.abs(r), gm)
    m[0] = 0.0
    return s, m


def cholesky(A):
    """Lower factor of a symmetric matrix, or None when a pivot is not positive (the kernel's rule)."""
    K = A.shape[0]
    L = np.zeros((K, K))
    for j in range(K):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0.0:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, K):
            L[i, j] = (A[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L


def unpack(s, K):
    """n, (Sw, Sr, Sww, Srr, Swr), SG [K], SGG [K][K], SGw [K], SGr [K] of a sums vector."""
    SG = s[6:6 + K]
    A = np.zeros((K, K))
    at = 6 + K
    for k in range(K):
        for l in range(k, K):
            A[k, l] = A[l, k] = s[at]
            at += 1
    return s[0], s[1:6], SG, A, s[at:at + K], s[at + K:at + 2 * K]


def solve(s, T, model, HW, rho_prev=np.nan, eps=1e-6, min_valid=0.25):
    """One decision: (status or None while running, T_next, rho, converged)."""
    K = PARAMS[model]
    n, (Sw, Sr, Sww, Srr, Swr), SG, A, SGw, SGr = unpack(np.asarray(s, np.float64), K)
    if n < min_valid * HW:
        return FEW_VALID, T, np.nan, False
    if not np.isfinite(s).all():
        return NONFINITE, T, np.nan, False
    with np.errstate(all='ignore'):
        mw, mr = Sw / n, Sr / n
        ww, rr, corr = Sww - n * mw * mw, Srr - n * mr * mr, Swr - n * mw * mr
        rho = corr / (np.sqrt(ww) * np.sqrt(rr))
    if not np.isfinite(rho):
        return NONFINITE, T, np.nan, False
    if abs(rho - rho_prev) < eps:
        return OK, T, rho, True
    ip, tp = SGw - mw * SG, SGr - mr * SG
    L = cholesky(A)
    if L is None:
        return NOT_POSITIVE, T, rho, False
    y, z = np.linalg.solve(L, ip), np.linalg.solve(L, tp)
    lam_n, lam_d = ww - y @ y, corr - z @ y
    if not (np.isfinite(lam_n) and np.isfinite(lam_d)):
        return NONFINITE, T, rho, False
    if lam_d <= 0.0:
        return LAMBDA, T, rho, False
    dp = np.linalg.solve(L.T, (lam_n / lam_d) * z - y)
    Tn = updated(T, dp, model)
    if not np.isfinite(Tn).all():
        return NONFINITE, T, rho, False
    return None, Tn, rho, False


def refine(optical, thermal, T0, model='similarity', feature='gradient', ksize=5, eps=1e-6, maxiter=50, min_valid=0.25,
           f32=False, history=None):
    """The whole refinement of one pair (float32 frames).  Returns dict(transform, rho, nit, success, converged, status);
    history: a list that receives (T, rho) of every evaluated iterate."""
    planes = image_planes(features(optical, ksize, feature, f32), f32)
    template = features(thermal, ksize, feature, f32)
    return refine_features(planes, template, T0, model, eps, maxiter, min_valid, f32, history)


def refine_features(planes, template, T0, model='similarity', eps=1e-6, maxiter=50, min_valid=0.25, f32=False, history=None):
    """refine() on given feature frames: planes = (f, gx, gy) of the image, template [H][W]."""
    T = start_transform(T0, model)
    HW = template.shape[0] * template.shape[1]
    rho_prev, rho_last, nit = np.nan, np.nan, 0
    while True:
        s = sums(planes, template, T, model, f32)
        status, Tn, rho, conv = solve(s, T, model, HW, rho_prev, eps, min_valid)
        if np.isfinite(rho):
            rho_last = rho
        if history is not None:
            history.append((T.copy(), rho))
        if status is not None:
            return {'transform': T, 'rho': rho_last, 'nit': nit, 'success': status == OK, 'converged': conv, 'status': status}
        T, rho_prev, nit = Tn, rho, nit + 1
        if nit >= maxiter:
            return {'transform': T, 'rho': rho_last, 'nit': nit, 'success': True, 'converged': False, 'status': OK}
