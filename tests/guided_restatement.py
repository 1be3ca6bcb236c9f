"""float64 yardstick of mp_match_guided (mutual nearest neighbours inside a geometric gate) and the planted inputs its
tests run on.  numpy only.

Definition restated (include/multipoint_hip.h: mp_match_guided), for one pair with homography H (optical (x, y, 1) ->
thermal):
    wa_i       = H (x_i, y_i, 1) in double, divided by its third component, rounded once to fp32 (no candidates when that
                 component is 0 or the result is not finite)
    gate(i, j) = (wa_i.x - x_j)^2 + (wa_i.y - y_j)^2 <= radius^2 in fp32
    u          = 2 - 2 clip(A . B^T, -1, 1) in DOUBLE on the fp32 descriptors (the kernel: fp32 MFMA tiles)
    i ~ j  iff  j = argmin u(i, .) over the gated j  and  i = argmin u(., j) over the gated i  (stable: lowest index on ties)

Tolerance, as in tests/test_gpu_match_modes.py: tau = 2 (D + 2) 2^-24 bounds the error of an fp32 dot product of D terms of
unit rows carried into u.  A row (column) is AMBIGUOUS when the gap between its two best gated u lies in (0, 2 tau]: there
either order is a correct answer."""
import numpy as np

K = 160
FRAME = (240, 320)            # H, W
PAIRS = [(160, 130), (37, 160), (129, 33), (96, 1), (5, 2), (0, 7), (7, 0)]
# 129 rows cross the 128-row workgroup; 130 and 33 columns the 32-column tile and the column-share boundary; one- and
# two-row sides; two pairs with an empty side
WIDTHS = (64, 128, 256)
RADII = (6.0, 48.0)
MIN_RADIUS_MARGIN = 5e-4      # px: no |d - radius| below this (the fp32 error of d is < 1e-4 px at these coordinates)
MAX_AMBIGUOUS = 0.02


def tau(D):
    return 2.0 * (D + 2) * 2.0 ** -24


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def planted_homography(rng):
    """rotation +-0.08 rad, scale 0.95-1.05, shift +-4 px, perspective terms +-1e-4; about the frame centre"""
    Hf, Wf = FRAME
    a = rng.uniform(-0.08, 0.08); s = rng.uniform(0.95, 1.05)
    tx, ty = rng.uniform(-4, 4, 2)
    p1, p2 = rng.uniform(-1e-4, 1e-4, 2)
    cx, cy = Wf / 2.0, Hf / 2.0
    C = np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1.0]]); Ci = np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1.0]])
    R = np.array([[s * np.cos(a), -s * np.sin(a), tx], [s * np.sin(a), s * np.cos(a), ty], [p1, p2, 1.0]])
    H = Ci @ R @ C
    return H / H[2, 2]


def warp_f32(H, kp_yx):
    """wa [N, 2] fp32 (x, y); NaN rows have no candidates"""
    H = np.asarray(H, np.float64).reshape(3, 3)
    kp = np.asarray(kp_yx, np.float64).reshape(-1, 2)
    x, y = kp[:, 1], kp[:, 0]
    w = H[2, 0] * x + H[2, 1] * y + H[2, 2]
    with np.errstate(divide='ignore', invalid='ignore'):
        u = ((H[0, 0] * x + H[0, 1] * y + H[0, 2]) / w).astype(np.float32)
        v = ((H[1, 0] * x + H[1, 1] * y + H[1, 2]) / w).astype(np.float32)
    bad = (w == 0) | ~np.isfinite(u) | ~np.isfinite(v)
    out = np.stack([u, v], 1)
    out[bad] = np.nan
    return out


def gate_matrix(H, kpA_yx, kpB_yx, radius):
    """(gate [N, M] bool decided in fp32 as the kernel does, distance [N, M] float64 of the fp32 positions)"""
    wa = warp_f32(H, kpA_yx)
    b = np.asarray(kpB_yx).reshape(-1, 2)[:, ::-1].astype(np.float32)
    dx = wa[:, None, 0] - b[None, :, 0]; dy = wa[:, None, 1] - b[None, :, 1]
    with np.errstate(invalid='ignore'):
        d2 = dx * dx + dy * dy                                   # fp32
        gate = d2 <= np.float32(radius) * np.float32(radius)
        dist = np.sqrt(dx.astype(np.float64) ** 2 + dy.astype(np.float64) ** 2)
    return gate, dist


def u_matrix(A, B):
    return 2.0 - 2.0 * np.clip(A.astype(np.float64) @ B.astype(np.float64).T, -1.0, 1.0)


def _best_two(u, gate, axis):
    """per row (axis 1) / column (axis 0): (arg-min over the gated entries, -1 if none; whether a second gated entry with a
    larger u exists; the gap between the two best)"""
    g = np.where(gate, u, np.inf)
    if axis == 0:
        g = g.T
    n, m = g.shape
    if m == 0:
        return np.full(n, -1, np.int64), np.zeros(n, bool), np.full(n, np.inf)
    order = np.argsort(g, axis=1, kind='stable')[:, :2]              # stable: equal u -> lower index first
    us = np.take_along_axis(g, order, 1)
    best = np.where(np.isfinite(us[:, 0]), order[:, 0], -1)
    if m < 2:
        return best, np.zeros(n, bool), np.full(n, np.inf)
    with np.errstate(invalid='ignore'):
        gap = us[:, 1] - us[:, 0]
    return best, np.isfinite(us[:, 1]) & (gap > 0), gap


def guided_mutual(A, B, kpA_yx, kpB_yx, H, radius, D=None, threshold=-1.0):
    """The yardstick.  Returns (match [N] int64 (-1 = none), ambiguous [N] bool, u [N, M] float64).  A row is ambiguous when
    its own two best gated u, or those of the column it picks, are within (0, 2 tau]."""
    N, M = len(A), len(B)
    D = A.shape[1] if D is None else D
    u = u_matrix(A, B)
    if np.isinf(radius):
        gate = np.ones((N, M), bool)
    else:
        gate, _ = gate_matrix(H, kpA_yx, kpB_yx, radius)
    if N == 0 or M == 0:
        return np.full(N, -1, np.int64), np.zeros(N, bool), u
    rb = _best_two(u, gate, 1); cb = _best_two(u, gate, 0)
    row_best, col_best = rb[0], cb[0]
    t2 = 2 * tau(D)
    with np.errstate(invalid='ignore'):
        row_amb = rb[1] & (rb[2] <= t2)
        col_amb = cb[1] & (cb[2] <= t2)
    match = np.full(N, -1, np.int64)
    has = row_best >= 0
    j = row_best[has]
    mutual = col_best[j] == np.nonzero(has)[0]
    match[np.nonzero(has)[0][mutual]] = j[mutual]
    if threshold >= 0:
        rows = np.nonzero(match >= 0)[0]
        far = ~(np.sqrt(u[rows, match[rows]]) < threshold)
        match[rows[far]] = -1
    amb = row_amb.copy()
    amb[has] |= col_amb[j]
    return match, amb, u


def plain_mutual(A, B):
    """mutual nearest neighbours in float64 without a gate (stable arg-mins): match [N] (-1 = none)"""
    N, M = len(A), len(B)
    if N == 0 or M == 0:
        return np.full(N, -1, np.int64)
    u = u_matrix(A, B)
    j = np.argmin(u, axis=1); i = np.argmin(u, axis=0)             # (np.argmin: the first minimum)
    return np.where(i[j] == np.arange(N), j, -1)


def make_pair(D, case):
    """One planted pair (seed 1000 D + case) in a 240 x 320 frame: N distinct integer optical keypoints >= 10 px from the
    border, a planted H, M thermal rows of random unit descriptors at random positions, of which min(N, M) // 2 shuffled slots
    become TRUE partners (position round(H a_i) + jitter in {-1, 0, 1}^2 clipped to the frame, descriptor
    unit(a_i + 0.6 g / sqrt(D))); half of those get a DISTRACTOR row with a closer descriptor (unit(a_i + 0.2 g / sqrt(D)))
    half a frame width away.  Returns dict(A, B, kpA, kpB (int32 y, x), H, true [n_true, 2] (i, j))."""
    N, M = PAIRS[case]
    Hf, Wf = FRAME
    rng = np.random.default_rng(1000 * D + case)
    cells = rng.permutation((Hf - 20) * (Wf - 20))[:N]
    kpA = np.stack([cells // (Wf - 20) + 10, cells % (Wf - 20) + 10], 1).astype(np.int32).reshape(N, 2)
    H = planted_homography(rng)
    A = _unit(rng.standard_normal((N, D))) if N else np.zeros((0, D), np.float32)
    B = _unit(rng.standard_normal((M, D))) if M else np.zeros((0, D), np.float32)
    kpB = np.stack([rng.integers(0, Hf, M), rng.integers(0, Wf, M)], 1).astype(np.int32).reshape(M, 2)
    n_true = min(N, M) // 2
    slots = rng.permutation(M)
    src = rng.permutation(N)[:n_true]
    true = []
    for t in range(n_true):
        i, j = int(src[t]), int(slots[t])
        x, y = float(kpA[i, 1]), float(kpA[i, 0])
        w = H[2, 0] * x + H[2, 1] * y + H[2, 2]
        px = (H[0, 0] * x + H[0, 1] * y + H[0, 2]) / w; py = (H[1, 0] * x + H[1, 1] * y + H[1, 2]) / w
        jx, jy = rng.integers(-1, 2, 2)
        bx = int(np.clip(np.round(px) + jx, 0, Wf - 1)); by = int(np.clip(np.round(py) + jy, 0, Hf - 1))
        kpB[j] = (by, bx)
        B[j] = _unit((A[i].astype(np.float64) + 0.6 * rng.standard_normal(D) / np.sqrt(D))[None])[0]
        true.append((i, j))
    # distractors for the first half of the true partners, in slots the partners do not use
    n_dis = min(n_true // 2, M - n_true)
    for t in range(n_dis):
        i, j = true[t]
        k = int(slots[n_true + t])
        kpB[k] = (kpB[j, 0], (kpB[j, 1] + Wf // 2) % Wf)
        B[k] = _unit((A[i].astype(np.float64) + 0.2 * rng.standard_normal(D) / np.sqrt(D))[None])[0]
    return dict(A=A, B=B, kpA=kpA, kpB=kpB, H=H, true=np.array(true, np.int64).reshape(-1, 2))


def input_conditions(pair, D, radius):
    """What the tests assert on their INPUTS before touching the GPU: (smallest |d - radius| over all (i, j) in px,
    fraction of ambiguous rows)."""
    N, M = len(pair['A']), len(pair['B'])
    if N == 0 or M == 0:
        return np.inf, 0.0
    _, dist = gate_matrix(pair['H'], pair['kpA'], pair['kpB'], radius)
    margin = float(np.nanmin(np.abs(dist - radius)))
    _, amb, _ = guided_mutual(pair['A'], pair['B'], pair['kpA'], pair['kpB'], pair['H'], radius, D)
    return margin, float(amb.sum()) / N
