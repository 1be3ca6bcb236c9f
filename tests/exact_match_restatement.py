"""Exact-arithmetic inputs for the matchers and the descriptor sampler, and their integer truths.  numpy only.

Descriptor rows with entries in {0, +-1/s}, s a power of two, and s^2 non-zero entries have norm exactly 1, and every dot
product of two of them is an integer multiple of 1/s^2 of magnitude <= 1: every partial sum of every summation order is
exactly representable in fp32, so a kernel that adds the products in any order -- MFMA tiles, a scalar loop, fused or not --
returns the integer truth.  With

    u_int = 2 s^2 - 2 A . B^T      (int64; the squared distance u = 2 - 2 a.b in units of 1 / s^2, a multiple of 4)
    d     = float32(sqrt(float64(u_int) / s^2))    (one correctly rounded sqrtf of an exact u: float64 sqrt rounded to fp32
                                                    equals the correctly rounded fp32 sqrt, 53 >= 2 * 24 + 2)

nothing about a matcher's answer is ambiguous: neighbours are the stable arg-sort of an integer matrix (equal distances: the
lower index first), thresholds are strict comparisons of fp32 numbers, and every index, count and distance bit pattern is
determined.  Rows are drawn from a small codebook (12 base sign patterns, up to 3 sign flips per row), so the distances take
few values and most queries have TIED nearest neighbours, spread over half-waves, 32-column tiles and column shares.

The widths:  D = 64: 64 x +-1/8;  D = 128 and 192: 64 x +-1/8 on one fixed pattern per codebook, zeros elsewhere;
D = 256: 256 x +-1/16.

The gate of the guided matcher gets the same treatment: integer keypoints and homographies whose double arithmetic is exact
and whose warped positions are integers or half-integers (exact in fp32, as are the gate's differences and, wherever the sum
is anywhere near r^2, its squares and their sum), so gate(i, j) is decided in integers:
(X - bx W)^2 + (Y - by W)^2 <= r^2 W^2 for the homogeneous (X, Y, W) = Hn (x, y, 1) of an integer matrix Hn = q H."""
import numpy as np

N_BASE = 12
MAX_FLIPS = 3
MATCH_SHARES = 2             # mp_common.h


def scale_of(D):
    return 16 if D == 256 else 8


def make_book(rng, D):
    """A codebook: N_BASE sign patterns on the s^2 non-zero positions of the width (one fixed zero pattern, which every row
    drawn from the book shares)."""
    s = scale_of(D)
    nz = np.sort(rng.permutation(D)[:s * s])
    base = np.zeros((N_BASE, D), np.int32)
    base[:, nz] = rng.integers(0, 2, (N_BASE, s * s)) * 2 - 1
    return dict(D=D, s=s, nz=nz, base=base)


def flip(row, rng, k, nz):
    """`row` with the signs of exactly k of its non-zero positions changed: u_int = 4 k from the original"""
    out = row.copy()
    out[rng.permutation(nz)[:k]] *= -1
    return out


def fresh_row(rng, book):
    """A random sign pattern on the book's non-zero positions: far (u about 1) from every codebook row"""
    r = np.zeros(book['D'], np.int32)
    r[book['nz']] = rng.integers(0, 2, len(book['nz'])) * 2 - 1
    return r


def exact_rows(rng, n, D, book=None):
    """(rows [n, D] int32 with entries in {0, +-1}, s): rows / s are fp32 rows of norm exactly 1.  Every row is a codebook
    pattern with 0 .. MAX_FLIPS sign flips."""
    book = make_book(rng, D) if book is None else book
    rows = book['base'][rng.integers(0, N_BASE, n)].copy()
    for i in range(n):
        rows[i] = flip(rows[i], rng, int(rng.integers(0, MAX_FLIPS + 1)), book['nz'])
    return rows.reshape(n, D), book['s']


def as_f32(rows, s):
    return (rows.astype(np.float64) / s).astype(np.float32)


def flips_for(D, d):
    """the number of sign flips that puts two rows at distance exactly d (d^2 = 4 k / s^2)"""
    k = d * d * scale_of(D) ** 2 / 4
    assert k == int(k)
    return int(k)


def make_pair(D, N, M, seed):
    """One pair of exact rows with planted structure (as far as N and M have room for it):
      * exact duplicates: rows of B copied from rows of A (d = 0), one of them also into the last, partial tile, and rows of
        B copied to rows of B one half-wave, one tile and one column share away (tied winners at every distance);
      * fresh rows a (far from the codebook) whose only near row of B is a with k flips, k chosen for d = 0.5 and d = 1.0
        exactly: mutual matches that sit ON the thresholds 0.5 and 1.0; the d = 0.5 partner is duplicated in B;
      * an exactly opposite row (d = 2).
    Pairs with M <= 2: (N, 1) is N copies of a row against its opposite (the mutual match has d = 2 exactly), (N, 2) is a row
    against itself and its opposite (nearest d = 0, second d = 2).
    Returns dict(A, B int32 rows, s, book, planted = {name: (i, j)})."""
    rng = np.random.default_rng(seed)
    book = make_book(rng, D)
    A, s = exact_rows(rng, N, D, book)
    B, _ = exact_rows(rng, M, D, book)
    planted = {}
    if N and M == 1:
        A[:] = A[0]; B[0] = -A[0]
        planted['opposite'] = (0, 0)
    elif N and M == 2:
        B[0] = A[0]; B[1] = -A[0]
        planted['duplicate'] = (0, 0); planted['opposite'] = (0, 1)
    elif N >= 30 and M >= 30:
        ia = rng.permutation(N); jb = rng.permutation(M)
        # duplicates of A rows in B
        for t in range(4):
            B[jb[t]] = A[ia[t]]
        planted['duplicate'] = (int(ia[0]), int(jb[0]))
        # on-threshold partners of fresh rows
        for t, (name, d) in enumerate((('half', 0.5), ('one', 1.0))):
            i, j = int(ia[4 + t]), int(jb[4 + t])
            A[i] = fresh_row(rng, book)
            B[j] = flip(A[i], rng, flips_for(D, d), book['nz'])
            planted[name] = (i, j)
        # the d = 0.5 partner once more, elsewhere in B (the lower index must win, the threshold must refuse both)
        j2 = int(jb[6]); B[j2] = B[planted['half'][1]]
        planted['half'] = (planted['half'][0], min(planted['half'][1], j2))
        # an opposite row
        i, j = int(ia[6]), int(jb[7])
        B[j] = -A[i]
        planted['opposite'] = (i, j)
        # duplicates inside B at fixed offsets: the other half-wave, the next tile, the other column share
        taken = set(int(x) for x in jb[:8])
        # ... and one duplicate of an A row in the last, partial tile (a d = 0 tie that reaches it)
        if M % 32 and M - 1 not in taken:
            B[M - 1] = A[ia[1]]; taken.add(M - 1)
        for off in (4, 32, M // 2 + 1):
            for j in range(0, M - off, 7):
                if j not in taken and j + off not in taken:
                    B[j + off] = B[j]; taken.update((j, j + off))
                    break
    return dict(A=A, B=B, s=s, book=book, planted=planted)


# ---- the truths, in integers ----

def u_int(A, B, s):
    return 2 * s * s - 2 * (A.astype(np.int64) @ B.astype(np.int64).T)


def dist_f32(u, s):
    return np.sqrt(u.astype(np.float64) / float(s * s)).astype(np.float32)


def two_nearest(u):
    """(idx [N, 2] int64, -1 where B has no such row): stable arg-sort by (u_int, index)"""
    N, M = u.shape
    idx = np.full((N, 2), -1, np.int64)
    if M:
        order = np.argsort(u, axis=1, kind='stable')[:, :2]
        idx[:, :order.shape[1]] = order
    return idx


def _gated_argmin(u, gate):
    """per row: the first minimum over the gated entries, -1 if there is none"""
    N, M = u.shape
    if M == 0:
        return np.full(N, -1, np.int64)
    big = np.iinfo(np.int64).max
    g = u if gate is None else np.where(gate, u, big)
    j = np.argmin(g, axis=1)
    return np.where(g[np.arange(N), j] < big, j, -1)


def mutual(u, s, threshold=-1.0, gate=None):
    """(match [N] int64, -1 = none; dist [N] float32, 0 where none): mutual nearest neighbours over the gated entries, kept
    iff the fp32 distance is STRICTLY below the fp32 threshold (threshold < 0: no threshold)"""
    N, M = u.shape
    match = np.full(N, -1, np.int64); dist = np.zeros(N, np.float32)
    if N == 0 or M == 0:
        return match, dist
    rb = _gated_argmin(u, gate)
    cb = _gated_argmin(u.T, None if gate is None else gate.T)
    d = dist_f32(u, s)
    for i in range(N):
        j = rb[i]
        if j >= 0 and cb[j] == i and (threshold < 0 or d[i, j] < np.float32(threshold)):
            match[i] = j; dist[i] = d[i, j]
    return match, dist


def ratio_keep(d1, d2, has_second, ratio):
    """Lowe's test as nearest_kernel and get_matches define it: float64(d1) < ratio * float64(d2) on the fp32 distances"""
    return has_second & (d1.astype(np.float64) < float(ratio) * d2.astype(np.float64))


def threshold_list(u, s, threshold):
    """(ij [n, 2] int64 in row-major order, dist [n] float32): every pair with fp32 d < fp32 threshold"""
    d = dist_f32(u, s)
    ij = np.argwhere(d < np.float32(threshold))
    return ij, d[ij[:, 0], ij[:, 1]]


def share_boundary(M):
    """first column of the second column share (mp_match.h: column_share with MATCH_SHARES = 2)"""
    ntile = (M + 31) // 32
    return ((ntile + MATCH_SHARES - 1) // MATCH_SHARES) * 32


CATEGORIES = ('half_wave', 'tile', 'share', 'last_partial_tile')


def coverage(u, M):
    """Per query row, where its decisive columns lie.  {'tied': [N] bool, 'tie_<c>' / 'top2_<c>': [N] bool for c in
    CATEGORIES}: tie_<c> -- the row's TIED nearest columns (two or more at the minimum) fall into different half-waves
    (col & 4) / different 32-column tiles / different column shares / reach the last, partial tile; top2_<c> -- the same for
    the row's best and second-best column."""
    N = u.shape[0]
    out = {'tied': np.zeros(N, bool)}
    for c in CATEGORIES:
        out['tie_' + c] = np.zeros(N, bool); out['top2_' + c] = np.zeros(N, bool)
    if M < 2 or N == 0:
        return out
    sb = share_boundary(M)
    last = (M // 32) * 32 if M % 32 else M            # first column of the partial tile (M: there is none)

    def spread(cols):
        cols = np.asarray(cols)
        return {'half_wave': len(set((cols & 4).tolist())) > 1, 'tile': len(set((cols >> 5).tolist())) > 1,
                'share': len(set((cols >= sb).tolist())) > 1, 'last_partial_tile': bool((cols >= last).any())}
    top2 = two_nearest(u)
    for i in range(N):
        tied = np.nonzero(u[i] == u[i].min())[0]
        out['tied'][i] = len(tied) > 1
        if len(tied) > 1:
            for c, v in spread(tied).items():
                out['tie_' + c][i] = v
        for c, v in spread(top2[i]).items():
            out['top2_' + c][i] = v
    return out


def categories_of(cov, i):
    """the coverage categories row i belongs to, for failure messages"""
    return [k for k, v in cov.items() if v[i]] or ['none']


# ---- the gate ----

RADIUS = 5
ON_BOUNDARY = [(3, 4), (5, 0), (4, 3), (0, 5), (-3, 4), (-5, 0), (3, -4), (0, -5)]      # (dx, dy): dx^2 + dy^2 = 25
JUST_OUTSIDE = [(4, 4), (-4, 4), (4, -4)]                                               # 32 > 25
INSIDE = [(0, 0), (1, 1), (2, -1), (-3, 3), (0, 4)]
FAR = [(40, 17), (-33, 29)]

# name: (Hn integer matrix, q): H = Hn / q.  (X, Y, W) = Hn (x, y, 1); wa = (X / W, Y / W)
HOMOGRAPHIES = {
    'identity': ([[1, 0, 0], [0, 1, 0], [0, 0, 1]], 1),
    'shift': ([[1, 0, 7], [0, 1, -3], [0, 0, 1]], 1),
    'half': ([[1, 0, 0], [0, 1, 0], [0, 0, 2]], 2),                    # diag(0.5, 0.5, 1)
    'projective': ([[0, 64, 0], [0, 0, 128], [1, 0, 0]], 1),           # w = x, optical x in {1, 2, 4}: wa = (64 y / x, 128 / x)
    'zero': ([[0, 0, 0], [0, 0, 0], [0, 0, 0]], 1),                    # find_homography's "no estimate"
    'w_zero': ([[0, 64, 0], [0, 0, 128], [1, 0, 0]], 1),               # ... with optical x in {0, 1, 2, 4}: w = 0 where x = 0
}
GATE_CASES = [('identity', 160, 130), ('shift', 129, 33), ('half', 33, 129), ('projective', 37, 160), ('zero', 128, 64),
              ('w_zero', 160, 130), ('identity', 5, 2), ('identity', 0, 7), ('shift', 7, 0), ('half', 32, 32)]


def homography_f64(name):
    Hn, q = HOMOGRAPHIES[name]
    return np.asarray(Hn, np.float64) / q


def warp_int(name, kp_yx):
    """(X, Y, W) int64 [N] each"""
    Hn = np.asarray(HOMOGRAPHIES[name][0], np.int64)
    kp = np.asarray(kp_yx, np.int64).reshape(-1, 2)
    p = np.stack([kp[:, 1], kp[:, 0], np.ones(len(kp), np.int64)], 0)
    X, Y, W = Hn @ p
    return X, Y, W


def gate_int(name, kpA_yx, kpB_yx, radius=RADIUS):
    """gate [N, M] bool in integers: W != 0 and (X - bx W)^2 + (Y - by W)^2 <= r^2 W^2"""
    X, Y, W = warp_int(name, kpA_yx)
    b = np.asarray(kpB_yx, np.int64).reshape(-1, 2)
    ex = X[:, None] - b[None, :, 1] * W[:, None]; ey = Y[:, None] - b[None, :, 0] * W[:, None]
    r2 = int(radius) * int(radius)
    assert radius == int(radius)
    return (W[:, None] != 0) & (ex * ex + ey * ey <= r2 * (W * W)[:, None])


def make_gate_case(D, case, seed):
    """Descriptors as make_pair's, integer keypoints for GATE_CASES[case]: distinct optical keypoints (y, x); every thermal
    keypoint is the warped position of an optical one with an INTEGER image plus an offset drawn in turn from ON_BOUNDARY,
    JUST_OUTSIDE, INSIDE and FAR, so the gate's `<=` is decided exactly on, just outside and well inside the radius.  The first
    quarter of the optical rows is never used as a source (most of them end up without a candidate).  The partners make_pair
    planted at d = 0.5 and d = 1.0 are placed on the boundary and on the image of their rows where that image is an integer.
    Returns make_pair's dict plus name, kpA, kpB (int32 [., 2] (y, x)), H (float64 3x3), offsets [(j, i, (dx, dy))]."""
    name, N, M = GATE_CASES[case]
    pair = make_pair(D, N, M, seed)
    rng = np.random.default_rng(seed + 7)
    if name in ('projective', 'w_zero'):
        xs = np.array([1, 2, 4] if name == 'projective' else [0, 1, 2, 4])
        cells = rng.permutation(len(xs) * 64)[:N]
        kpA = np.stack([(cells // len(xs)) * 2, xs[cells % len(xs)]], 1)          # even y: 64 y / x is an integer
    else:
        cells = rng.permutation(100 * 140)[:N]
        kpA = np.stack([cells // 140 + 20, cells % 140 + 20], 1)                  # ('half' maps odd coordinates to half-integers)
    kpA = kpA.astype(np.int32).reshape(N, 2)
    kpB = np.stack([rng.integers(300, 400, M), rng.integers(400, 500, M)], 1).astype(np.int32).reshape(M, 2)     # far from every image
    offsets = []
    if N and M:
        X, Y, W = warp_int(name, kpA)
        src = [i for i in range(N // 4, N) if W[i] != 0 and X[i] % W[i] == 0 and Y[i] % W[i] == 0]
        menu = ON_BOUNDARY + JUST_OUTSIDE + INSIDE + FAR
        # the partners planted ON the thresholds 0.5 and 1.0 stay candidates of their rows (one of them on the gate's boundary)
        fixed = {}
        for key, off in (('half', (3, 4)), ('one', (0, 0))):
            if key in pair['planted'] and pair['planted'][key][0] in src:
                fixed[pair['planted'][key][1]] = (pair['planted'][key][0], off)
        for j in range(M):
            if not src:
                break
            i, (dx, dy) = fixed.get(j, (src[int(rng.integers(0, len(src)))], menu[j % len(menu)]))
            kpB[j] = (Y[i] // W[i] + dy, X[i] // W[i] + dx)
            offsets.append((j, i, (dx, dy)))
    pair.update(name=name, kpA=kpA, kpB=kpB, H=homography_f64(name), offsets=offsets)
    return pair


# ---- descriptor sampling ----

def sample_truth(rows_map, s, kp_yx, H, W):
    """float64 bilinear sampling (grid_sample, zeros padding, align_corners=True) of the map rows_map [Hc, Wc, D] / s at the
    integer keypoints (y, x), then L2 normalisation with F.normalize's 1e-12 floor: [n, D] float64"""
    m = rows_map.astype(np.float64) / s
    Hc, Wc, D = m.shape
    out = np.zeros((len(kp_yx), D))
    for n, (y, x) in enumerate(np.asarray(kp_yx, np.int64)):
        iy = (y / (H * 0.5) - 1.0 + 1.0) / 2.0 * (Hc - 1); ix = (x / (W * 0.5) - 1.0 + 1.0) / 2.0 * (Wc - 1)
        y0, x0 = int(np.floor(iy)), int(np.floor(ix))
        v = np.zeros(D)
        for yy, wy in ((y0, y0 + 1 - iy), (y0 + 1, iy - y0)):
            for xx, wx in ((x0, x0 + 1 - ix), (x0 + 1, ix - x0)):
                if 0 <= yy < Hc and 0 <= xx < Wc:
                    v += m[yy, xx] * (wy * wx)
        out[n] = v / max(np.sqrt((v * v).sum()), 1e-12)
    return out


# ---- the cases the tests run on (built once per process and left unchanged) ----

import functools

K = 160
PAIRS = [(160, 130), (129, 33), (33, 129), (37, 160), (5, 2), (3, 1), (0, 7), (7, 0), (32, 32), (128, 64)]
# 129 rows cross the 128-row workgroup; 130, 33 and 129 columns the 32-column tile and the column-share boundary; 32 and 64
# are whole tiles; two- and one-row sides; two pairs with an empty side
WIDTHS = (64, 128, 256)
K_CLAMP, CLAMP_COUNTS = 96, (130, 200)          # counts beyond the capacity: the kernels clamp to K_CLAMP rows
SINGLES = [(64, 300, 333), (64, 1000, 1000), (256, 65, 400)]      # (D, N, M): the per-pair routes
LARGE = 100                                     # pairs with N * M >= LARGE ** 2 must have mostly tied queries


@functools.lru_cache(maxsize=None)
def batch(D):
    """[make_pair dict + u (int64 [N, M]) + cov (coverage)] for PAIRS"""
    out = []
    for c, (N, M) in enumerate(PAIRS):
        p = make_pair(D, N, M, 5000 * D + c)
        p['u'] = u_int(p['A'], p['B'], p['s']); p['cov'] = coverage(p['u'], M)
        out.append(p)
    return out


@functools.lru_cache(maxsize=None)
def clamp_pair(D):
    """a K_CLAMP x K_CLAMP pair (its counts will claim CLAMP_COUNTS rows)"""
    p = make_pair(D, K_CLAMP, K_CLAMP, 5000 * D + 50)
    p['u'] = u_int(p['A'], p['B'], p['s']); p['cov'] = coverage(p['u'], K_CLAMP)
    return p


@functools.lru_cache(maxsize=None)
def gate_batch(D):
    """[make_gate_case dict + u + gate (bool [N, M]) + cov] for GATE_CASES"""
    out = []
    for c in range(len(GATE_CASES)):
        p = make_gate_case(D, c, 7000 * D + c)
        p['u'] = u_int(p['A'], p['B'], p['s']); p['cov'] = coverage(p['u'], len(p['B']))
        p['gate'] = gate_int(p['name'], p['kpA'], p['kpB'])
        out.append(p)
    return out


@functools.lru_cache(maxsize=None)
def single(k):
    D, N, M = SINGLES[k]
    p = make_pair(D, N, M, 9000 + k)
    p['u'] = u_int(p['A'], p['B'], p['s']); p['cov'] = coverage(p['u'], M)
    return p
