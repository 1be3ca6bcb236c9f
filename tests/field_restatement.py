"""numpy restatement of the local alignment correction (include/multipoint_hip.h mp_field_fit / mp_field_warp),
written from its specification in float64: the model csrc/field.hip and multipoint_amd.utils.field are tested against.

  system        the dense matrix W + lambda L of one lattice
  effective     the weights as the fit takes them (zero where the weight or d is unusable) and the count of non-finite d
  dense_solve   numpy.linalg.solve of both axes
  pcg           the same Jacobi-preconditioned conjugate gradients as the kernel (order of operations, stopping rule, warm start)
  fit           the robust rounds around either solver
  interpolate   the field at pixel positions
  warp          frames sampled through a field, the fp32 blend reproduced in numpy.float32
"""
import numpy as np

F32 = np.float32
OK, NO_DATA, ALL_REJECTED, MAX_ITER = 0, 1, 2, 3
FAR = 2.0 ** 30


def degrees(gy, gx):
    i, j = np.mgrid[0:gy, 0:gx]
    return ((i > 0).astype(np.int64) + (j > 0) + (j < gx - 1) + (i < gy - 1)).astype(np.float64)


def system(w, lam):
    """dense (N, N) float64 W + lam L of a (gy, gx) weight lattice, nodes row-major"""
    gy, gx = w.shape
    N = gy * gx
    A = np.zeros((N, N))
    for i in range(gy):
        for j in range(gx):
            k = i * gx + j
            A[k, k] += w[i, j]
            for di, dj in ((0, 1), (1, 0)):
                if i + di < gy and j + dj < gx:
                    l = (i + di) * gx + (j + dj)
                    A[k, k] += lam
                    A[l, l] += lam
                    A[k, l] -= lam
                    A[l, k] -= lam
    return A


def effective(d, w):
    """(weights with zero where the weight is not positive and finite or d is not finite, d with zeros there, count of the nodes
    that have a usable weight and a non-finite d)"""
    w = np.asarray(w, np.float64)
    d = np.asarray(d, np.float64)
    with np.errstate(invalid='ignore'):
        usable = (w > 0) & np.isfinite(w)
    fin = np.isfinite(d).all(-1)
    keep = usable & fin
    return np.where(keep, w, 0.0), np.where(keep[..., None], d, 0.0), int((usable & ~fin).sum())


def dense_solve(d, w, lam):
    """u (gy, gx, 2) of (W + lam L) u = W d; w, d as effective() returns them, some w > 0"""
    A = system(w, lam)
    b = (w[..., None] * d).reshape(-1, 2)
    return np.linalg.solve(A, b).reshape(d.shape)


def _apply(p, w, lam, deg):
    """A p for p (gy, gx): neighbours added in the order up, left, right, down"""
    s = np.zeros_like(p)
    s[1:, :] += p[:-1, :]
    s[:, 1:] += p[:, :-1]
    s[:, :-1] += p[:, 1:]
    s[:-1, :] += p[1:, :]
    return (w + lam * deg) * p - lam * s


def pcg(d, w, lam, tol, max_iter, x0=None):
    """(u, iterations, relative residual, met): per axis stop at r^T r <= tol^2 b^T b, both axes share the iteration count"""
    gy, gx = w.shape
    deg = degrees(gy, gx)
    diag = w + lam * deg
    x = np.zeros(d.shape) if x0 is None else np.array(x0, np.float64)
    b = w[..., None] * d
    r = np.stack([b[..., a] - _apply(x[..., a], w, lam, deg) for a in range(2)], -1)
    p = r / diag[..., None]
    rz = [float((r[..., a] * p[..., a]).sum()) for a in range(2)]
    rr = [float((r[..., a] ** 2).sum()) for a in range(2)]
    bb = [float((b[..., a] ** 2).sum()) for a in range(2)]
    thr = [tol * tol * v for v in bb]
    dead = [False, False]
    it = 0
    while it < max_iter:
        act = [rr[a] > thr[a] and not dead[a] for a in range(2)]
        if not any(act):
            break
        for a in range(2):
            if not act[a]:
                continue
            q = _apply(p[..., a], w, lam, deg)
            pq = float((p[..., a] * q).sum())
            if not pq > 0.0:
                dead[a] = True
                continue
            alpha = rz[a] / pq
            x[..., a] += alpha * p[..., a]
            r[..., a] -= alpha * q
            z = r[..., a] / diag
            new = float((r[..., a] * z).sum())
            p[..., a] = z + (new / rz[a]) * p[..., a]
            rz[a], rr[a] = new, float((r[..., a] ** 2).sum())
        it += 1
    rel = max((np.sqrt(rr[a] / bb[a]) if bb[a] > 0 else (np.inf if rr[a] > 0 else 0.0)) for a in range(2))
    return x, it, float(rel), not any(rr[a] > thr[a] for a in range(2))


def robust_weights(u, d, w0, c):
    """w0 (1 - (e / c)^2)^2 for e = |u - d| < c, else 0"""
    e = np.sqrt((u[..., 0] - d[..., 0]) ** 2 + (u[..., 1] - d[..., 1]) ** 2)
    s = e / c
    g = 1.0 - s * s
    return np.where((w0 > 0) & (e < c), w0 * (g * g), 0.0), e


def fit(d, w, lam, robust_px=0.0, rounds=0, tol=1e-12, max_iter=None, solver='dense'):
    """One frame.  dict(u (gy, gx, 2), status, weight, nonzero, nonfinite, iterations, residual, solves): `solves` lists (weights,
    solution, residuals e the NEXT round's weights came from or None) of every solve, for the tests' bounds."""
    w0, dd, nonfinite = effective(d, w)
    gy, gx = w0.shape
    max_iter = 4 * gy * gx + 64 if max_iter is None else max_iter
    out = dict(u=np.zeros(dd.shape), status=NO_DATA, weight=w0, nonzero=int((w0 > 0).sum()), nonfinite=nonfinite, iterations=0,
               residual=0.0, solves=[])
    if out['nonzero'] == 0:
        return out
    wt = w0
    n_rounds = rounds if robust_px > 0 else 0
    for t in range(n_rounds + 1):
        if t > 0:
            nw, e = robust_weights(out['u'], dd, w0, robust_px)
            out['solves'][-1][2] = e
            if not (nw > 0).any():
                out['status'] = ALL_REJECTED
                break
            wt = nw
        if solver == 'dense':
            u, it, rel, met = dense_solve(dd, wt, lam), 0, 0.0, True
        else:
            u, it, rel, met = pcg(dd, wt, lam, tol, max_iter, out['u'])
        out.update(u=u, iterations=it, residual=rel, status=OK if met else MAX_ITER, weight=wt, nonzero=int((wt > 0).sum()))
        out['solves'].append([wt, u, None])
    return out


def _locate(v, origin, step, g, extrapolate):
    t = (np.asarray(v, np.float64) - origin) / step
    i = np.clip(np.floor(t), 0, max(g - 2, 0)).astype(np.int64)
    i1 = np.minimum(i + 1, g - 1)
    f = t - i
    if not extrapolate:
        f = np.clip(f, 0.0, 1.0)
    if g == 1:
        f = np.zeros_like(f)
    return i, i1, f


def interpolate(u, geometry, ys, xs, extrapolate=1):
    """(uy, ux) float64 (len(ys), len(xs)) of the field u (gy, gx, 2) at the pixel rows ys and columns xs"""
    y0, x0, step = geometry
    gy, gx = u.shape[:2]
    i, i1, fy = _locate(ys, y0, step, gy, extrapolate)
    j, j1, fx = _locate(xs, x0, step, gx, extrapolate)
    i, i1, fy, j, j1, fx = i[:, None], i1[:, None], fy[:, None], j[None], j1[None], fx[None]
    out = []
    with np.errstate(all='ignore'):
        for a in range(2):
            c = u[..., a]
            out.append((c[i, j] * (1.0 - fx) + c[i, j1] * fx) * (1.0 - fy) + (c[i1, j] * (1.0 - fx) + c[i1, j1] * fx) * fy)
    return out[0], out[1]


def warp(src, u, geometry, shape=None, hom=None, extrapolate=1):
    """(dst float32 (H, W), valid uint8 (H, W)) of one frame: src float32 (Hs, Ws), u (gy, gx, 2), hom (3, 3) or None"""
    src = np.asarray(src, F32)
    Hs, Ws = src.shape
    H, W = (Hs, Ws) if shape is None else shape
    ys, xs = np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64)
    uy, ux = interpolate(np.asarray(u, np.float64), geometry, ys, xs, extrapolate)
    with np.errstate(all='ignore'):
        qy, qx = ys[:, None] + uy, xs[None] + ux
        ok = np.isfinite(qy) & np.isfinite(qx)
        if hom is not None:
            h = np.asarray(hom, np.float64).reshape(9)
            X, Y, Z = (h[0] * qx + h[1] * qy) + h[2], (h[3] * qx + h[4] * qy) + h[5], (h[6] * qx + h[7] * qy) + h[8]
            ok &= np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & (Z > 0)
            qy, qx = Y / Z, X / Z
        ok &= (np.abs(qy) <= FAR) & (np.abs(qx) <= FAR)
    qy, qx = np.where(ok, qy, 0.0), np.where(ok, qx, 0.0)
    fy0, fx0 = np.floor(qy), np.floor(qx)
    iy, ix = fy0.astype(np.int64), fx0.astype(np.int64)
    fy, fx = (qy - fy0).astype(F32), (qx - fx0).astype(F32)
    wy, wx = (F32(1) - fy, fy), (F32(1) - fx, fx)
    padded = np.zeros((Hs + 2, Ws + 2), F32)
    padded[1:-1, 1:-1] = src
    tap, inside = {}, {}
    for a in range(2):
        for b in range(2):
            yy, xx = iy + a, ix + b
            inside[a, b] = (yy >= 0) & (yy < Hs) & (xx >= 0) & (xx < Ws)
            tap[a, b] = np.where(inside[a, b], padded[np.clip(yy, -1, Hs) + 1, np.clip(xx, -1, Ws) + 1], F32(0)).astype(F32)
    dst = (tap[0, 0] * wx[0] + tap[0, 1] * wx[1]) * wy[0] + (tap[1, 0] * wx[0] + tap[1, 1] * wx[1]) * wy[1]
    assert dst.dtype == F32
    valid = np.ones((H, W), bool)
    for a in range(2):
        for b in range(2):
            valid &= ~((wy[a] != 0) & (wx[b] != 0)) | inside[a, b]
    return np.where(ok, dst, F32(0)).astype(F32), (valid & ok).astype(np.uint8)
