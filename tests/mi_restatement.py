"""numpy restatement of the mutual-information alignment (reference create_dataset/helper_functions/align.py:13-215), the
model the HIP kernels of multipoint_amd/csrc/mutual_info.hip are tested against:

  warp_image             cv2.warpPerspective(image, inv(T), (W, H), borderValue=-1.0), INTER_LINEAR, with a source of any size
  joint_histogram        np.histogram2d(x, y, bins=(n, 2n)) of float32 samples as numpy >= 2 computes it (float32 edges)
  gaussian_smooth        scipy.ndimage.gaussian_filter(jh, sigma, mode='constant')
  score                  mutual_information_2d's arithmetic behind the histogram
  negative_mi            calculate_negative_mutual_information
  nelder_mead            scipy.optimize.minimize(method='Nelder-Mead', options={'adaptive': False}) for any callable
"""
import numpy as np


def cv_invert3(M):
    """cv::invert of a 3x3 float64 matrix (closed-form adjugate); singular -> zeros."""
    S = np.asarray(M, np.float64).reshape(3, 3)
    d = (S[0, 0] * (S[1, 1] * S[2, 2] - S[1, 2] * S[2, 1]) - S[0, 1] * (S[1, 0] * S[2, 2] - S[1, 2] * S[2, 0]) +
         S[0, 2] * (S[1, 0] * S[2, 1] - S[1, 1] * S[2, 0]))
    if d == 0.0:
        return np.zeros((3, 3))
    d = 1.0 / d
    t = [(S[1, 1] * S[2, 2] - S[1, 2] * S[2, 1]) * d, (S[0, 2] * S[2, 1] - S[0, 1] * S[2, 2]) * d,
         (S[0, 1] * S[1, 2] - S[0, 2] * S[1, 1]) * d, (S[1, 2] * S[2, 0] - S[1, 0] * S[2, 2]) * d,
         (S[0, 0] * S[2, 2] - S[0, 2] * S[2, 0]) * d, (S[0, 2] * S[1, 0] - S[0, 0] * S[1, 2]) * d,
         (S[1, 0] * S[2, 1] - S[1, 1] * S[2, 0]) * d, (S[0, 1] * S[2, 0] - S[0, 0] * S[2, 1]) * d,
         (S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]) * d]
    return np.array(t, np.float64).reshape(3, 3)


def block_width(height, width):
    """The width of WarpPerspectiveInvoker's blocks for a destination of height x width."""
    return min(1024 // min(16, int(height)), int(width))


def fixed_point(Mi, height, width, split=True):
    """The source coordinates of every destination pixel in 1/32 px, (X, Y) as int64 (H, W), as WarpPerspectiveInvoker
    computes them: the sum over the block start xb and the offset x - xb in float64.  split=False puts xb = 0 everywhere
    (one block as wide as the frame), which is NOT OpenCV's arithmetic once the frame is wider than a block."""
    H, W = int(height), int(width)
    bw0 = block_width(H, W) if split else W
    ys, xs = np.mgrid[0:H, 0:W]
    xb = ((xs // bw0) * bw0).astype(np.float64)
    x1 = xs.astype(np.float64) - xb
    yf = ys.astype(np.float64)
    X0 = (Mi[0, 0] * xb + Mi[0, 1] * yf) + Mi[0, 2]
    Y0 = (Mi[1, 0] * xb + Mi[1, 1] * yf) + Mi[1, 2]
    W0 = (Mi[2, 0] * xb + Mi[2, 1] * yf) + Mi[2, 2]
    den = W0 + Mi[2, 0] * x1
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        w = np.where(den != 0, 32.0 / den, 0.0)
        fX = np.clip((X0 + Mi[0, 0] * x1) * w, -2147483648.0, 2147483647.0)
        fY = np.clip((Y0 + Mi[1, 0] * x1) * w, -2147483648.0, 2147483647.0)
    return np.rint(fX).astype(np.int64), np.rint(fY).astype(np.int64)


def warp_linear(src, Mi, height, width, border_value=-1.0, split=True):
    """OpenCV's WarpPerspectiveInvoker + remapBilinear<float> for the already inverted matrix Mi (destination -> source):
    coordinates in 1/32 px computed block-wise in float64 (block width from the DESTINATION size), four float32 taps weighted
    left to right, taps outside the source read `border_value`."""
    src = np.ascontiguousarray(src, dtype=np.float32)
    Hs, Ws = src.shape
    X, Y = fixed_point(Mi, height, width, split)
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    fx = ((X & 31).astype(np.float32) * np.float32(1.0 / 32)).astype(np.float32)
    fy = ((Y & 31).astype(np.float32) * np.float32(1.0 / 32)).astype(np.float32)
    ax, ay = (np.float32(1) - fx).astype(np.float32), (np.float32(1) - fy).astype(np.float32)
    w0, w1, w2, w3 = ay * ax, ay * fx, fy * ax, fy * fx

    def tap(yy, xx):
        ok = (xx >= 0) & (xx < Ws) & (yy >= 0) & (yy < Hs)
        return np.where(ok, src[np.clip(yy, 0, Hs - 1), np.clip(xx, 0, Ws - 1)], np.float32(border_value)).astype(np.float32)

    out = tap(sy, sx) * w0
    out = (out + tap(sy, sx + 1) * w1).astype(np.float32)
    out = (out + tap(sy + 1, sx) * w2).astype(np.float32)
    out = (out + tap(sy + 1, sx + 1) * w3).astype(np.float32)
    return out


def warp_image(image, transform, height, width, split=True):
    """align.py:13-50 for a 3x3 transform.  Both inverses are the closed-form one (the reference's first is np.linalg.inv)."""
    return warp_linear(image, cv_invert3(cv_invert3(transform)), height, width, -1.0, split)


def bin_edges(v, n):
    """np.linspace(min, max, n + 1) in float32, as np.histogramdd builds its edges for float32 samples under numpy >= 2."""
    a, b = np.float32(v.min()), np.float32(v.max())
    if a == b:
        a, b = np.float32(a - np.float32(0.5)), np.float32(b + np.float32(0.5))
    step = np.float32(np.float32(b - a) / np.float32(n))
    e = (np.arange(n + 1, dtype=np.float32) * step).astype(np.float32) + a
    e = e.astype(np.float32)
    e[n] = b
    return e


def bin_index(v, n):
    """bin = (number of edges <= v) - 1; samples equal to the last edge go to bin n - 1."""
    v = np.asarray(v, np.float32).ravel()
    e = bin_edges(v, n)
    k = np.searchsorted(e, v, side='right') - 1
    k[v == e[n]] -= 1
    return k


def joint_histogram(x, y, n):
    """(n, 2n) int64 counts of np.histogram2d(x, y, bins=(n, 2n))."""
    kx, ky = bin_index(x, n), bin_index(y, 2 * n)
    return np.bincount(kx * (2 * n) + ky, minlength=2 * n * n).reshape(n, 2 * n)


def gaussian_weights(sigma):
    r = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-r, r + 1)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return w / w.sum()


def gaussian_smooth(jh, sigma):
    """scipy.ndimage.gaussian_filter(jh, sigma, mode='constant'): axis 0, then axis 1, zeros outside."""
    w = gaussian_weights(sigma)
    r = (len(w) - 1) // 2
    out = np.asarray(jh, np.float64)
    for axis in (0, 1):
        n = out.shape[axis]
        pad = [(0, 0), (0, 0)]
        pad[axis] = (r, r)
        p = np.pad(out, pad)
        acc = np.zeros_like(out)
        for k in range(2 * r + 1):
            acc = acc + w[k] * np.take(p, np.arange(k, k + n), axis=axis)
        out = acc
    return out


def score(jh, normalized=False):
    """align.py:80-100 behind the (smoothed) histogram."""
    jh = np.asarray(jh, np.float64) + np.finfo(float).eps
    jh = jh / np.sum(jh)
    s1 = np.sum(jh, axis=0)
    s2 = np.sum(jh, axis=1)
    if normalized:
        return (np.sum(s1 * np.log(s1)) + np.sum(s2 * np.log(s2))) / np.sum(jh * np.log(jh)) - 1
    return np.sum(jh * np.log(jh)) - np.sum(s1 * np.log(s1)) - np.sum(s2 * np.log(s2))


def mutual_information_2d(x, y, sigma=5, bins=100, normalized=False):
    jh = joint_histogram(x, y, bins).astype(np.float64)
    if sigma > 0:
        jh = gaussian_smooth(jh, sigma)
    return score(jh, normalized)


def negative_mi(transform, optical, thermal, init_transform, bins, regularize=False, normalized_mi=False, smoothing_sigma=0):
    """align.py:102-155 for a 3x3 transform."""
    T = np.asarray(transform, np.float64).reshape(3, 3)
    h, w = thermal.shape
    warped = warp_image(optical, T, h, w)
    mi = mutual_information_2d(warped.ravel(), np.asarray(thermal, np.float32).ravel(), bins=bins, normalized=normalized_mi,
                               sigma=smoothing_sigma)
    if regularize:
        return -mi + np.sqrt(np.sum((np.asarray(init_transform, np.float64).reshape(3, 3) - T) ** 2))
    return -mi


def _argsort_stable(f):
    return np.argsort(f, kind='stable')


def nelder_mead(func, x0, xatol=1e-4, fatol=1e-4, maxiter=None, maxfun=None, shrinks=None):
    """scipy.optimize._optimize._minimize_neldermead with adaptive=False and no bounds, statement by statement; equal values
    keep their order when the simplex is sorted.  Returns dict(x, fun, nit, nfev, success, status).  `shrinks`: a list that
    receives the number of function calls made before each shrink began."""
    x0 = np.asarray(x0, np.float64).ravel().copy()
    N = len(x0)
    rho, chi, psi, sigma = 1.0, 2.0, 0.5, 0.5
    sim = np.empty((N + 1, N))
    sim[0] = x0
    for k in range(N):
        y = x0.copy()
        y[k] = (1 + 0.05) * y[k] if y[k] != 0 else 0.00025
        sim[k + 1] = y
    if maxiter is None and maxfun is None:
        maxiter, maxfun = N * 200, N * 200
    elif maxiter is None:
        maxiter = N * 200 if maxfun == np.inf else np.inf
    elif maxfun is None:
        maxfun = N * 200 if maxiter == np.inf else np.inf
    fcalls = [0]

    class TooMany(Exception):
        pass

    def f(x):
        if fcalls[0] >= maxfun:
            raise TooMany()
        fcalls[0] += 1
        return float(func(np.copy(x)))

    fsim = np.full((N + 1,), np.inf)
    try:
        for k in range(N + 1):
            fsim[k] = f(sim[k])
    except TooMany:
        pass
    ind = _argsort_stable(fsim)
    sim, fsim = np.take(sim, ind, 0), np.take(fsim, ind, 0)
    iterations = 1
    while fcalls[0] < maxfun and iterations < maxiter:
        try:
            if np.max(np.ravel(np.abs(sim[1:] - sim[0]))) <= xatol and np.max(np.abs(fsim[0] - fsim[1:])) <= fatol:
                break
            xbar = np.add.reduce(sim[:-1], 0) / N
            xr = (1 + rho) * xbar - rho * sim[-1]
            fxr = f(xr)
            doshrink = 0
            if fxr < fsim[0]:
                xe = (1 + rho * chi) * xbar - rho * chi * sim[-1]
                fxe = f(xe)
                if fxe < fxr:
                    sim[-1], fsim[-1] = xe, fxe
                else:
                    sim[-1], fsim[-1] = xr, fxr
            elif fxr < fsim[-2]:
                sim[-1], fsim[-1] = xr, fxr
            else:
                if fxr < fsim[-1]:
                    xc = (1 + psi * rho) * xbar - psi * rho * sim[-1]
                    fxc = f(xc)
                    if fxc <= fxr:
                        sim[-1], fsim[-1] = xc, fxc
                    else:
                        doshrink = 1
                else:
                    xcc = (1 - psi) * xbar + psi * sim[-1]
                    fxcc = f(xcc)
                    if fxcc < fsim[-1]:
                        sim[-1], fsim[-1] = xcc, fxcc
                    else:
                        doshrink = 1
                if doshrink:
                    if shrinks is not None:
                        shrinks.append(fcalls[0])
                    for j in range(1, N + 1):
                        sim[j] = sim[0] + sigma * (sim[j] - sim[0])
                        fsim[j] = f(sim[j])
            iterations += 1
        except TooMany:
            pass
        finally:
            ind = _argsort_stable(fsim)
            sim, fsim = np.take(sim, ind, 0), np.take(fsim, ind, 0)
    status = 1 if fcalls[0] >= maxfun else (2 if iterations >= maxiter else 0)
    return {'x': sim[0].copy(), 'fun': float(np.min(fsim)), 'nit': iterations, 'nfev': fcalls[0], 'success': status == 0,
            'status': status}


# ---- a synthetic pair with a known alignment (the recovery test) ----
def blob_image(seed, H, W, n=60, smin=2.5, smax=9.0):
    """a smooth structured frame in [0, 1]: a sum of seeded Gaussian blobs"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.zeros((H, W))
    for _ in range(n):
        cy, cx, s, a = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(smin, smax), rng.uniform(0.3, 1.0)
        img += a * np.exp(-((ys - cy) ** 2 + (xs - cx) ** 2) / (2 * s * s))
    return (img / img.max()).astype(np.float32)


def recovery_pair(seed=11, H=96, W=128):
    """optical, thermal, T_true, T_init: thermal = a non-monotone map of the optical frame warped by T_true (thermal -> optical,
    every thermal pixel inside the optical frame); T_init = T_true displaced by about 2 px."""
    optical = blob_image(seed, H, W, 300, 1.2, 4.0)
    T_true = np.array([[0.94, 0.012, 3.0], [-0.01, 0.95, 2.0], [1.5e-5, -1e-5, 1.0]])
    w = warp_image(optical, T_true, H, W)
    assert w.min() >= 0.0
    thermal = (4.0 * (w.astype(np.float64) - 0.45) ** 2).astype(np.float32)
    T_init = T_true + np.array([[0.004, 0.0, 1.6], [0.0, -0.003, -1.3], [0.0, 0.0, 0.0]])
    return optical, thermal, T_true, T_init


def corner_error(T, T_true, H, W):
    """mean distance between the four thermal corners mapped by T and by T_true"""
    c = np.array([[0, 0, 1], [W - 1, 0, 1], [0, H - 1, 1], [W - 1, H - 1, 1]], np.float64).T
    a, b = np.asarray(T, np.float64).reshape(3, 3) @ c, np.asarray(T_true, np.float64).reshape(3, 3) @ c
    return float(np.mean(np.linalg.norm(a[:2] / a[2] - b[:2] / b[2], axis=0)))
