"""numpy float64 restatement of the similarity / affine estimators (multipoint_amd/csrc/mp_transform.h): the same counter-based
sampling (oracle.mp_oracle._mix64), the same closed form and 3x3 elimination with the same bounds, the same forward test, the
lowest hypothesis index on ties, the same least-squares refit and the same round rule of the refinement.  Host code; the GPU
tests hold the kernels to it within 1e-6 max(1, |H|) (sums are added in another order here)."""
import numpy as np

from oracle import mp_oracle as _oracle

SAMPLE = {'similarity': 2, 'affine': 3}


def _f32(p):
    return np.asarray(p, dtype=np.float32).astype(np.float64).reshape(-1, 2)


def sample(seed, index, t, n, S):
    ctr = _oracle._mix64((seed ^ (index << 32) ^ t) & _oracle._M64)
    idx = []
    while len(idx) < S:
        ctr = _oracle._mix64(ctr)
        c = ctr % n
        if c not in idx:
            idx.append(c)
    return idx


def solve3(rows):
    """rows [3][5]: A | r0 | r1.  Gaussian elimination with partial pivoting, pivot bound 1e-10.  (z0, z1) or None."""
    a = np.array(rows, dtype=np.float64)
    for c in range(3):
        piv = c + int(np.argmax(np.abs(a[c:, c])))
        if not abs(a[piv, c]) >= 1e-10:
            return None
        if piv != c:
            a[[c, piv]] = a[[piv, c]]
        for r in range(c + 1, 3):
            a[r, c:] -= (a[r, c] / a[c, c]) * a[c, c:]
    z = np.zeros((3, 2))
    for c in (2, 1, 0):
        z[c] = (a[c, 3:] - a[c, c + 1:3] @ z[c + 1:]) / a[c, c]
    return z[:, 0], z[:, 1]


def minimal(model, a, b, idx):
    """The exact model through the sampled correspondences as m[6] (top two rows), or None for a degenerate sample."""
    if model == 'similarity':
        (x0, y0), (x1, y1) = a[idx[0]], a[idx[1]]
        (u0, v0), (u1, v1) = b[idx[0]], b[idx[1]]
        dx, dy, ex, ey = x1 - x0, y1 - y0, u1 - u0, v1 - v0
        dd = dx * dx + dy * dy
        if not dd >= 1e-10:
            return None
        p, q = (dx * ex + dy * ey) / dd, (dx * ey - dy * ex) / dd
        return np.array([p, -q, u0 - (p * x0 - q * y0), q, p, v0 - (q * x0 + p * y0)])
    z = solve3([[a[i, 0], a[i, 1], 1.0, b[i, 0], b[i, 1]] for i in idx])
    return None if z is None else np.concatenate(z)


def error2(m, a, b):
    du = m[0] * a[:, 0] + m[1] * a[:, 1] + m[2] - b[:, 0]
    dv = m[3] * a[:, 0] + m[4] * a[:, 1] + m[5] - b[:, 1]
    return du * du + dv * dv


def fit(model, a, b, inl):
    """Least squares over the set `inl` (bool mask), the device's formulas: m[6] or None when the set does not determine it."""
    pa, pb = a[inl], b[inl]
    ca, cb = pa.mean(0), pb.mean(0)
    x, y = (pa - ca).T
    u, v = (pb - cb).T
    if model == 'similarity':
        den = (x * x + y * y).sum()
        if not den >= 1e-10:
            return None
        p, q = (x * u + y * v).sum() / den, (x * v - y * u).sum() / den
        return np.array([p, -q, cb[0] - (p * ca[0] - q * ca[1]), q, p, cb[1] - (q * ca[0] + p * ca[1])])
    n = float(len(pa))
    z = solve3([[(x * x).sum(), (x * y).sum(), x.sum(), (x * u).sum(), (x * v).sum()],
                [(x * y).sum(), (y * y).sum(), y.sum(), (y * u).sum(), (y * v).sum()],
                [x.sum(), y.sum(), n, u.sum(), v.sum()]])
    if z is None:
        return None
    z0, z1 = z
    return np.array([z0[0], z0[1], cb[0] + z0[2] - (z0[0] * ca[0] + z0[1] * ca[1]),
                     z1[0], z1[1], cb[1] + z1[2] - (z1[0] * ca[0] + z1[1] * ca[1])])


def as_matrix(m):
    return np.array([[m[0], m[1], m[2]], [m[3], m[4], m[5]], [0.0, 0.0, 1.0]])


def ransac_transform(pts_optical_xy, pts_thermal_xy, model, reproj_threshold, max_iters, seed, index, full=False):
    """(H 3x3 float64 or None, inlier mask (n,) bool) of pair / group `index`; with full=True also the winning sample's
    model m[6] (None without a model)."""
    a, b = _f32(pts_optical_xy), _f32(pts_thermal_xy)
    n, S = len(a), SAMPLE[model]
    none = (None, np.zeros(n, bool), None) if full else (None, np.zeros(n, bool))
    if n < S + 1:
        return none
    thr2 = float(reproj_threshold) ** 2
    best_cnt, best_mask, best_m = 0, None, None
    for t in range(max_iters):
        m = minimal(model, a, b, sample(seed, index, t, n, S))
        if m is None:
            continue
        mk = error2(m, a, b) <= thr2
        if mk.sum() > best_cnt:
            best_cnt, best_mask, best_m = int(mk.sum()), mk, m
    if best_cnt < S + 1:
        return none
    m = fit(model, a, b, best_mask)
    if m is None:
        return none
    return (as_matrix(m), best_mask, best_m) if full else (as_matrix(m), best_mask)


def refine_transform(pts_optical_xy, pts_thermal_xy, model, H, reproj_threshold, rounds, marked=None):
    """The refinement's round rule.  Returns (H 3x3, mask (n,) bool, n_inliers, cost [2], refits done); all zero for an input
    that is all zeros, not finite or has h22 = 0, and when a marked set has fewer than S + 1 members.  marked: a list that
    receives every model m[6] a set was marked under."""
    a, b = _f32(pts_optical_xy), _f32(pts_thermal_xy)
    n, S = len(a), SAMPLE[model]
    h = np.asarray(H, np.float64).reshape(9)
    zero = (np.zeros((3, 3)), np.zeros(n, bool), 0, np.zeros(2), 0)
    if not np.isfinite(h).all() or not abs(h[8]) > 0.0:
        return zero
    m = h[:6] / h[8]
    thr2 = float(reproj_threshold) ** 2
    marked = [] if marked is None else marked
    marked.append(m.copy())
    mask = error2(m, a, b) <= thr2
    if mask.sum() < S + 1:
        return zero
    c0 = c1 = error2(m, a, b)[mask].sum()
    done = 0
    for r in range(rounds):
        if r > 0:
            marked.append(m.copy())
            new = error2(m, a, b) <= thr2
            changed = not np.array_equal(new, mask)
            mask = new
            if not changed:
                break
            if mask.sum() < S + 1:
                return zero
        f = fit(model, a, b, mask)
        if f is None:
            break
        before, after = error2(m, a, b)[mask].sum(), error2(f, a, b)[mask].sum()
        if not after <= before:
            c0 = c1 = before
            break
        c0, c1, m = before, after, f
        done += 1
    return as_matrix(m), mask, int(mask.sum()), np.array([c0, c1]), done
