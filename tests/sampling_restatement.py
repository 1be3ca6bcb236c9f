"""TEST INFRASTRUCTURE: numpy float64 restatements of the hand-written grid_sample kernels of
multipoint_amd/csrc/homog_adapt.hip (warp_kernel, accumulate_kernel, begin_kernel, finalize_kernel, gaussian_filter_kernel,
valid_mask_kernel) and multipoint_amd/csrc/sample_desc.hip (sample_desc_kernel).  No torch, no GPU.

The comments of the two .hip files are the specification.  Every function restates the arithmetic they state -- coordinates
in float64 rounded once to float32, weights from the float32 coordinates, taps summed in float64 -- and returns the expected
array together with a per-element error bound whose derivation is in its docstring.  Nothing here is tuned on a kernel's
output.  U = 2^-24 is the unit round-off of float32 (half an ulp, relative).

Every restatement takes `mutant=None`.  MUTANTS maps the name of a deliberately wrong variant, one line different each, to
the restatement it lives in; tests/test_sampling_host.py demands that the committed cases tell every one of them from the
truth by more than the bound."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -126            # one flushed subnormal product
TIE_PX = 1e-4                 # |coordinate - half-integer| below which a nearest sample may go either way
VACUOUS_FRACTION = 0.01       # a bound above this fraction of max|src| says nothing


def has_exact_terms(m):
    """every entry a multiple of 1/8 below 2^12: with pixel indices below 2^8 the products and sums X, Y, Z are exact in float64,
    fused or not, so u and v are the correctly rounded quotients on the device as here and nothing can land on the other side of
    a rounding."""
    m = np.asarray(m, np.float64).reshape(3, 3)
    return bool(np.all(m * 8 == np.rint(m * 8)) and np.abs(m).max() < 2 ** 12)


def is_exact_matrix(m):
    """exact terms and the third row 0 0 1: the coordinates themselves are exact, in float64 and in float32 (below 2^21 with
    three fractional bits: 24 bits)."""
    m = np.asarray(m, np.float64).reshape(3, 3)
    return has_exact_terms(m) and bool(np.array_equal(m[2], [0.0, 0.0, 1.0]))


# ---------------------------------------------------------------------------------------------------------------------
# shared pieces: project(), reflect_coord(), sample_bilinear()
# ---------------------------------------------------------------------------------------------------------------------
def project(hom, Ho, Wo):
    """project(): X, Y, Z and the divisions in float64 (no contraction), u and v rounded to float32.  Returns
    (u64, v64, u32, v32, ok) with ok = both quotients finite."""
    m = np.asarray(hom, np.float64).reshape(9)
    y, x = np.mgrid[0:Ho, 0:Wo].astype(np.float64)
    X = (m[0] * x + m[1] * y) + m[2]
    Y = (m[3] * x + m[4] * y) + m[5]
    Z = (m[6] * x + m[7] * y) + m[8]
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        u, v = X / Z, Y / Z
        ok = np.isfinite(u) & np.isfinite(v)
        return u, v, u.astype(F32), v.astype(F32), ok


def reflect_coord(c, size, mutant=None):
    """reflect_coord(): float32 fabs, fmod, flip parity, clip; size <= 1 gives 0."""
    c = np.asarray(c, F32)
    if size <= 1:
        return np.zeros_like(c)
    span = F32(size if mutant == 'reflect_about_size' else size - 1)
    with np.errstate(invalid='ignore', over='ignore'):
        a = np.abs(c)
        extra = np.fmod(a, span).astype(F32)
        flips = np.floor((a / span).astype(F32))
        odd = np.fmod(flips, F32(2)) == 1
        r = np.where(odd, (span - extra).astype(F32), extra)
        return np.minimum(span, np.maximum(r, F32(0))).astype(F32)


def _next(c, up):
    return np.nextafter(np.asarray(c, F32), F32(np.inf if up else -np.inf)).astype(F32)


def _ulp(c):
    c = np.abs(np.asarray(c, F32))
    with np.errstate(invalid='ignore', over='ignore'):
        return (_next(c, True).astype(np.float64) - c.astype(np.float64))


def _taps(img, yy, xx):
    """zero-padded gather img[yy, xx] (int64 index arrays) as float64."""
    H, W = img.shape
    ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
    return np.where(ok, img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0.0).astype(np.float64)


def sample_bilinear(img, ix, iy, mutant=None):
    """sample_bilinear() of a float64 (H,W) image at float32 coordinates: the four weights are float32 products of float32
    differences (the kernel's own operations, none of which can be fused), the taps are summed in float64; taps outside the
    frame are 0; |ix| or |iy| >= 1e9 (or NaN) gives 0.  Returns (value, amax, spread): amax = the largest |tap| of the cell,
    spread = max - min over the taps that a coordinate one float32 step away could touch (the 2x2 cell, or the 4x4 patch
    around it when a coordinate sits within one ulp of an integer)."""
    ix, iy = np.asarray(ix, F32), np.asarray(iy, F32)
    with np.errstate(invalid='ignore', over='ignore'):
        far = ~(np.abs(ix) < F32(1e9)) | ~(np.abs(iy) < F32(1e9))
        sx, sy = np.where(far, F32(0), ix), np.where(far, F32(0), iy)
        x0f, y0f = np.floor(sx), np.floor(sy)
        x1f, y1f = x0f + F32(1), y0f + F32(1)
        ax, bx = (x1f - sx).astype(F32), (sx - x0f).astype(F32)
        ay, by = (y1f - sy).astype(F32), (sy - y0f).astype(F32)
        nw, ne, sw, se = (ax * ay).astype(F32), (bx * ay).astype(F32), (ax * by).astype(F32), (bx * by).astype(F32)
    if mutant == 'swap_ne_sw':
        ne, sw = sw, ne
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    t = [_taps(img, y0, x0), _taps(img, y0, x0 + 1), _taps(img, y0 + 1, x0), _taps(img, y0 + 1, x0 + 1)]
    val = t[0] * nw.astype(np.float64) + t[1] * ne.astype(np.float64) + t[2] * sw.astype(np.float64) + t[3] * se.astype(np.float64)
    amax = np.max(np.abs(t), axis=0)
    lo, hi = np.min(t, axis=0), np.max(t, axis=0)
    edge = (bx.astype(np.float64) <= _ulp(sx)) | (ax.astype(np.float64) <= _ulp(sx)) | \
           (by.astype(np.float64) <= _ulp(sy)) | (ay.astype(np.float64) <= _ulp(sy))
    if edge.any():
        for dy in range(-1, 3):
            for dx in range(-1, 3):
                w = _taps(img, y0 + dy, x0 + dx)
                lo, hi = np.where(edge, np.minimum(lo, w), lo), np.where(edge, np.maximum(hi, w), hi)
    val = np.where(far, 0.0, val)
    return val, np.where(far, 0.0, amax), np.where(far, 0.0, hi - lo)


C1 = 5


def bilinear_bound(amax, spread, u32, v32, exact_terms=False):
    """|device - restatement| for one bilinear sample.

    The weights are the same float32 numbers on both sides.  The device then rounds four products, each by at most
    U |tap_i w_i| with sum_i |tap_i w_i| <= amax sum_i w_i, and three sums (the first `out += ` adds to 0 and is exact), each
    by at most U amax sum_i w_i; a contracted multiply-add only drops roundings.  sum_i w_i <= 1 + 3U.  That is 1 + 3 roundings
    of size U amax, and one more for the second-order terms: c1 = 5.  4 TINY covers products flushed to zero.

    The device may fuse m0*x + m1*y + m2, which moves X, Y or Z by a few 2^-53 relative; where the float64 quotient lies that
    close to the midpoint of two float32 numbers, one coordinate comes out one float32 step away.  The bilinear surface moves
    by at most that step times the largest difference between the taps involved: ulp32(max(|u|,|v|)) * spread, with u, v taken
    before reflection (reflection is 1-Lipschitz); no such term under has_exact_terms.  Both coordinates stepping at once is
    not covered (probability ~1e-17 per pixel)."""
    with np.errstate(invalid='ignore', over='ignore'):
        step = _ulp(np.maximum(np.abs(u32), np.abs(v32)))
    step = np.where(np.isfinite(step), step, 0.0) * (0.0 if exact_terms else 1.0)
    return C1 * U * amax + 4 * TINY + step * spread


def _reflect_jump(c32, size):
    """True where a coordinate one float32 step away reflects to a place further off than that step (plus the roundings of
    `span - extra` and of the clip): floorf(c / span) rounds up just below a multiple of span.  The bound is void there."""
    c32 = np.asarray(c32, F32)
    mid = reflect_coord(c32, size).astype(np.float64)
    out = np.zeros(c32.shape, bool)
    for up in (False, True):
        other = reflect_coord(_next(c32, up), size).astype(np.float64)
        with np.errstate(invalid='ignore'):
            out |= np.abs(other - mid) > 2 * _ulp(c32) + _ulp(F32(max(size - 1, 1)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# warp_kernel<MODE, PAD>
# ---------------------------------------------------------------------------------------------------------------------
def warp(src, hom, dsize, mode, padding, mutant=None):
    """warp_kernel: src (n_src,H,W), hom (n_out,3,3) destination -> source, output map n samples source n % n_src.

    Returns a dict:
      want     (n_out,Ho,Wo) float64
      bound    (n_out,Ho,Wo) float64; bilinear: bilinear_bound (inf where _reflect_jump); nearest: 0
      vacuous  bilinear pixels whose bound exceeds VACUOUS_FRACTION * max|src|
      tie      nearest pixels where the float64 u or v (the reflected coordinate under reflection padding) lies within
               TIE_PX of a half-integer and the matrix has no exact terms (has_exact_terms): the kernel may return either neighbour
      alts     (4,n_out,Ho,Wo): the values at (floor|floor+1) x (floor|floor+1) of the sampled coordinate, the candidates on ties
    Nearest: nearbyint (half to even) of the float32 coordinate, zeros outside; the value is a copy, hence exact."""
    src = np.asarray(src, np.float64)
    n_src, H, W = src.shape
    hom = np.asarray(hom, np.float64).reshape(-1, 3, 3)
    n_out = len(hom)
    Ho, Wo = dsize
    want = np.zeros((n_out, Ho, Wo))
    bound = np.zeros_like(want)
    tie = np.zeros(want.shape, bool)
    alts = np.zeros((4,) + want.shape)
    for n in range(n_out):
        img = src[n % n_src]
        u64, v64, u, v, ok = project(hom[n], Ho, Wo)
        cu, cv = u, v
        jump = np.zeros(ok.shape, bool)
        if padding == 'reflection':
            cu, cv = reflect_coord(u, W, mutant), reflect_coord(v, H, mutant)
            if mutant == 'zeros_on_one_side':                 # no reflection left of / above the frame
                cu, cv = np.where(u < 0, u, cu), np.where(v < 0, v, cv)
            jump = _reflect_jump(u, W) | _reflect_jump(v, H)
        if mode == 'bilinear':
            val, amax, spread = sample_bilinear(img, cu, cv, mutant)
            want[n] = np.where(ok, val, 0.0)
            b = bilinear_bound(amax, spread, u, v, has_exact_terms(hom[n]))
            bound[n] = np.where(ok, np.where(jump & (not has_exact_terms(hom[n])), np.inf, b), 0.0)
        else:
            with np.errstate(invalid='ignore', over='ignore'):
                if mutant == 'round_half_up':
                    xr, yr = np.floor(cu.astype(np.float64) + 0.5), np.floor(cv.astype(np.float64) + 0.5)
                else:
                    xr, yr = np.rint(cu).astype(np.float64), np.rint(cv).astype(np.float64)
                inside = ok & (xr >= 0) & (xr < W) & (yr >= 0) & (yr < H)
                xi = np.where(inside, xr, 0).astype(np.int64)
                yi = np.where(inside, yr, 0).astype(np.int64)
                want[n] = np.where(inside, img[yi, xi], 0.0)
                fx = np.where(ok, np.floor(cu.astype(np.float64)), 0.0)
                fy = np.where(ok, np.floor(cv.astype(np.float64)), 0.0)
                fx, fy = np.clip(fx, -2.0 ** 40, 2.0 ** 40).astype(np.int64), np.clip(fy, -2.0 ** 40, 2.0 ** 40).astype(np.int64)
                for i, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                    alts[i, n] = np.where(ok, _taps(img, fy + dy, fx + dx), 0.0)
                if not has_exact_terms(hom[n]):
                    def near_half(c):
                        return np.abs(c - np.floor(c) - 0.5) < TIE_PX
                    t = near_half(u64) | near_half(v64) | near_half(cu.astype(np.float64)) | near_half(cv.astype(np.float64))
                    tie[n] = ok & (t | jump)
    vacuous = bound > VACUOUS_FRACTION * max(np.abs(src).max(), TINY) if mode == 'bilinear' else np.zeros(want.shape, bool)
    return {'want': want, 'bound': bound, 'vacuous': vacuous, 'tie': tie, 'alts': alts}


# ---------------------------------------------------------------------------------------------------------------------
# begin_kernel / accumulate_kernel<AGG> / finalize_kernel
# ---------------------------------------------------------------------------------------------------------------------
def _combine(a, b, agg):
    """a, a*b or a+b as ONE float32 operation (what begin_kernel and the accumulate gather compute per tap)."""
    a = np.asarray(a, F32)
    if agg == 0:
        return a
    b = np.asarray(b, F32)
    return (a * b).astype(F32) if agg == 1 else (a + b).astype(F32)


def begin(pa, pb, agg):
    """begin_kernel: count = 1, prob = a, a*b or a+b: a single IEEE float32 operation, so the expected value is exact
    (bound 0).  Returns (prob, count) as float32."""
    prob = _combine(pa, pb, agg)
    return prob.copy(), np.ones_like(prob)


def accumulate(pa, pb, mask, hom, B, agg, prob0, count0, mutant=None):
    """accumulate_kernel: pa, pb (G*B,H,W) float32 maps (map g*B + b = image b seen through homography g), mask (G,H,W) 0/1
    (one per homography, shared by the B images), hom (G,3,3) output pixel -> view pixel, prob0 / count0 (B,H,W) the state
    the launch adds to.  For g ascending: a view whose projection is not finite is skipped; cs = nearest sample of mask g
    (zeros outside), s = bilinear zero-padded sample of the combined map (each tap combined in float32 first: one rounding,
    restated exactly); c += cs; p += s * cs.

    Returns dict: prob, count (float64), bound (on prob), tie (pixels where some view's nearest sample is within TIE_PX of a
    half-integer under a non-exact matrix; there count lies in [count_lo, count_hi] and prob is not compared), count_lo/hi.

    count is a sum of at most G ones added to a small integer or quarter-integer: exact in float32, bound 0.
    prob: s * cs is exact (cs is 0 or 1), so each view adds its sample's bilinear_bound and one rounding of the running sum,
    U * max(|p| before, |p| after) at most:  bound = sum_g cs_g * bilinear_bound_g + U * sum_g cs_g * max|partial p|."""
    pa = np.asarray(pa, F32)
    GB, H, W = pa.shape
    hom = np.asarray(hom, np.float64).reshape(-1, 3, 3)
    G = len(hom)
    assert GB == G * B
    comb = _combine(pa, pb, agg).astype(np.float64)
    p = np.asarray(prob0, np.float64).copy()
    c = np.asarray(count0, np.float64).copy()
    c_lo, c_hi = c.copy(), c.copy()
    bound = np.zeros_like(p)
    tie = np.zeros(p.shape, bool)
    mask = np.asarray(mask, np.float64)
    for g in range(G):
        w = warp(mask[g:g + 1] if mutant != 'mask_per_image' else mask[:1], hom[g:g + 1], (H, W), 'nearest', 'zeros')
        u64, v64, u, v, ok = project(hom[g], H, W)
        # NOTE on this mutant: accumulate_kernel's `continue` is not observable as written -- without it nearbyintf(inf) fails the
        # range test (cs = 0) and sample_bilinear returns 0 for a coordinate that is NaN or >= 1e9, so the view adds nothing
        # either way.  The mutant therefore stands for the nearest fault that WOULD show: handling Z == 0 as valid_mask_kernel
        # (cv2) does, iz = 0, which sends the point at infinity to pixel (0, 0).  It guards a rewrite, not today's kernel.
        if mutant == 'infinity_not_skipped':
            u, v = np.where(ok, u, F32(0)), np.where(ok, v, F32(0))
        for b in range(B):
            if mutant == 'mask_per_image':
                mi = (g * B + b) % G
                w = warp(mask[mi:mi + 1], hom[g:g + 1], (H, W), 'nearest', 'zeros')
            cs = w['want'][0]
            if mutant == 'infinity_not_skipped':
                cs = np.where(ok, cs, mask[g, 0, 0])
            src = comb[(b * G + g) if mutant == 'map_b_major' else (g * B + b)]
            s, amax, spread = sample_bilinear(src, u, v)
            live = ok if mutant != 'infinity_not_skipped' else np.ones_like(ok)
            s = np.where(live, s, 0.0)
            before = np.abs(p[b])
            c[b] += np.where(live, cs, 0.0)
            p[b] += s * cs
            bound[b] += np.where(live, cs * (bilinear_bound(amax, spread, u, v, has_exact_terms(hom[g])) + U * np.maximum(before, np.abs(p[b]))), 0.0)
            a = w['alts'][:, 0]
            c_lo[b] += np.where(ok & w['tie'][0], a.min(axis=0), np.where(ok, cs, 0.0))
            c_hi[b] += np.where(ok & w['tie'][0], a.max(axis=0), np.where(ok, cs, 0.0))
            tie[b] |= w['tie'][0]
    return {'prob': p, 'count': c, 'bound': bound, 'tie': tie, 'count_lo': c_lo, 'count_hi': c_hi}


def finalize(prob, count, agg, min_count, mutant=None):
    """finalize_kernel: v = prob / count; sqrt (aggregation 1) or * 0.5 (aggregation 2); 0 where min_count > 0 and
    count < min_count.  Division and square root are correctly rounded float32 operations and * 0.5 is exact, so numpy's
    float32 gives the expected bits: bound 0.  count == 0 gives inf or NaN as IEEE does (compare with equal_nan)."""
    p, c = np.asarray(prob, F32), np.asarray(count, F32)
    with np.errstate(divide='ignore', invalid='ignore'):
        v = (p / c).astype(F32)
        first, second = (1, 2) if mutant != 'sqrt_half_exchanged' else (2, 1)
        if agg == first:
            v = np.sqrt(v).astype(F32)
        elif agg == second:
            v = (v * F32(0.5)).astype(F32)
    mc = F32(min_count)
    if mc > 0:
        v = np.where((c <= mc) if mutant == 'min_count_le' else (c < mc), F32(0), v)
    return v.astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# gaussian_filter_kernel
# ---------------------------------------------------------------------------------------------------------------------
def _reflect_index(i, n, mutant=None):
    i = np.asarray(i)
    hi = 2 * n - i - 1 if mutant == 'filter_reflect_edge' else 2 * (n - 1) - i
    return np.where(i < 0, -i, np.where(i >= n, hi, i))


def gaussian_filter(x, wgt, mutant=None):
    """gaussian_filter_kernel: x (B,H,W), wgt (k,k) any table, k odd, r = (k-1)/2 < H, W.
    out[y, x] = sum_dy sum_dx in[refl(y + dy - r), refl(x + dx - r)] * wgt[dy, dx], single reflection about 0 and H-1.
    Bound: k^2 products and k^2 sums, each rounding at most U times a partial sum of |in * w| (a fused multiply-add drops
    half of them): (k^2 + 1) * U * sum|in * w|."""
    x = np.asarray(x, np.float64)
    w = np.asarray(wgt, np.float64)
    k = w.shape[0]
    assert w.shape == (k, k) and k % 2 == 1
    if mutant == 'filter_weights_transposed':
        w = w.T
    r = (k - 1) // 2
    B, H, W = x.shape
    ys, xs = np.arange(H), np.arange(W)
    out = np.zeros_like(x)
    mag = np.zeros_like(x)
    for dy in range(k):
        yy = _reflect_index(ys + dy - r, H, mutant)
        for dx in range(k):
            xx = _reflect_index(xs + dx - r, W, mutant)
            t = x[:, np.clip(yy, 0, H - 1)[:, None], np.clip(xx, 0, W - 1)[None, :]] * w[dy, dx]
            out += t
            mag += np.abs(t)
    return out, (k * k + 1) * U * mag + k * k * TINY


# ---------------------------------------------------------------------------------------------------------------------
# valid_mask_kernel
# ---------------------------------------------------------------------------------------------------------------------
def valid_mask(hom_inv, H, W, r, mask_border):
    """valid_mask_kernel: hom_inv (G,3,3) destination -> source.  raw(x, y) = 1 iff the source coordinate
    ((m0 x + m1 y + m2) * iz, ...), iz = 1/Z (0 where Z == 0), every float64 operation rounded on its own, clamped to the int
    range and rounded half to even, lies inside the frame.  Outside the frame raw is 0 with mask_border (the zero ring) and
    ignored (1) without.  out = minimum of raw over the (2r+1)^2 window.  (G,H,W) uint8, exact."""
    hom_inv = np.asarray(hom_inv, np.float64).reshape(-1, 3, 3)
    out = np.zeros((len(hom_inv), H, W), np.uint8)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    for g, m in enumerate(hom_inv.reshape(-1, 9)):
        Z = (m[6] * x + m[7] * y) + m[8]
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            iz = np.where(Z != 0, 1.0 / Z, 0.0)
            fx = ((m[0] * x + m[1] * y) + m[2]) * iz
            fy = ((m[3] * x + m[4] * y) + m[5]) * iz
            rx = np.rint(np.maximum(-2147483648.0, np.minimum(2147483647.0, fx)))
            ry = np.rint(np.maximum(-2147483648.0, np.minimum(2147483647.0, fy)))
            raw = (rx >= 0) & (rx < W) & (ry >= 0) & (ry < H)
        pad = np.full((H + 2 * r, W + 2 * r), not mask_border, bool)
        pad[r:r + H, r:r + W] = raw
        m_out = np.ones((H, W), bool)
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                m_out &= pad[dy:dy + H, dx:dx + W]
        out[g] = m_out
    return out


# ---------------------------------------------------------------------------------------------------------------------
# sample_desc_kernel
# ---------------------------------------------------------------------------------------------------------------------
C2 = 8


def sample_descriptors(desc, H, W, kp_yx, kp_count, mutant=None):
    """sample_desc_kernel: desc (B,Hc,Wc,D) channels-last, kp_yx (B,K,2) int (y,x), kp_count (B,) -> (B,K,D).

    Coordinates in float32, one IEEE operation at a time (nothing to fuse): g = y / (H * 0.5) - 1, i = ((g + 1) / 2) * (Hc - 1).
    The four weights are float32 products of float32 differences; taps outside the map are 0; the taps are summed in float64,
    the norm is taken in float64 with the floor 1e-12.  Rows k >= min(kp_count[b], K) are exactly 0 and their keypoints are
    never read.

    Returns (want, bound, norm): want float64, bound per element, norm (B,K) = sqrt(ss) in float64 before the floor.
    Bound per element: (c2 + D) * U * max|row|, row = the normalised output row.  c2 = 8: four tap products, three sums and
    the divide, each at most U * sum_i|tap_i w_i| / norm; the D term covers the D squares, the adds of the 64-lane butterfly
    and of the D/64 per-lane partial sums, the square root, and -- D >= 64 -- the ratio between sum_i|tap_i w_i| / norm and
    max|row|, which tests/test_sampling_host.py asserts to stay below 4 on every row that is compared.  It says nothing for
    rows whose norm is decided by cancellation or by the floor (norm < 1e-6): the cases list those rows."""
    desc = np.asarray(desc, np.float64)
    B, Hc, Wc, D = desc.shape
    kp = np.asarray(kp_yx, np.int64)
    K = kp.shape[1]
    cnt = np.asarray(kp_count, np.int64)
    f = F32
    valid = np.zeros((B, K), bool)
    if mutant == 'count_not_clipped':                # an unclipped count spills into the rows of the next image
        flat = valid.reshape(-1)
        for b in range(B):
            flat[b * K:b * K + max(int(cnt[b]), 0)] = True
    else:
        for b in range(B):
            valid[b, :max(min(int(cnt[b]), K), 0)] = True
    y = np.where(valid, kp[..., 0], 0)
    x = np.where(valid, kp[..., 1], 0)
    if mutant == 'desc_xy_exchanged':
        y, x = x, y
    hh, ww = (H - 1, W - 1) if mutant == 'desc_w_minus_1' else (H, W)
    gy = (y.astype(f) / f(f(hh) * f(0.5))).astype(f) - f(1)
    gx = (x.astype(f) / f(f(ww) * f(0.5))).astype(f) - f(1)
    iy = (((gy + f(1)).astype(f) / f(2)).astype(f) * f(Hc - 1)).astype(f)
    ix = (((gx + f(1)).astype(f) / f(2)).astype(f) * f(Wc - 1)).astype(f)
    y0f, x0f = np.floor(iy), np.floor(ix)
    y1f, x1f = y0f + f(1), x0f + f(1)
    wts = [((x1f - ix).astype(f) * (y1f - iy).astype(f)).astype(f), ((ix - x0f).astype(f) * (y1f - iy).astype(f)).astype(f),
           ((x1f - ix).astype(f) * (iy - y0f).astype(f)).astype(f), ((ix - x0f).astype(f) * (iy - y0f).astype(f)).astype(f)]
    y0, x0 = y0f.astype(np.int64), x0f.astype(np.int64)
    v = np.zeros((B, K, D))
    mag = np.zeros((B, K, D))
    bi = np.arange(B)[:, None]
    for wt, (dy, dx) in zip(wts, ((0, 0), (0, 1), (1, 0), (1, 1))):
        yy, xx = y0 + dy, x0 + dx
        ok = (yy >= 0) & (yy < Hc) & (xx >= 0) & (xx < Wc)
        tap = np.where(ok[..., None], desc[bi, np.clip(yy, 0, Hc - 1), np.clip(xx, 0, Wc - 1)], 0.0)
        v += tap * wt.astype(np.float64)[..., None]
        mag += np.abs(tap) * wt.astype(np.float64)[..., None]
    norm = np.sqrt((v * v).sum(-1))
    want = v / np.maximum(norm, 1e-12)[..., None]
    want = np.where(valid[..., None], want, 1.0 if mutant == 'zero_rows_not_written' else 0.0)
    norm = np.where(valid, norm, 0.0)
    bound = np.broadcast_to(((C2 + D) * U * np.abs(want).max(-1))[..., None], want.shape).copy()
    bound[~valid] = 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(valid & (norm > 0), mag.max(-1) / norm / np.maximum(np.abs(want).max(-1), TINY), 0.0)
    return {'want': want, 'bound': bound, 'norm': norm, 'valid': valid, 'tap_ratio': ratio}


# ---------------------------------------------------------------------------------------------------------------------
# name -> kernel family of the restatement that takes it as `mutant=`
MUTANTS = {
    'swap_ne_sw': 'warp',                     # NE and SW weights swapped
    'reflect_about_size': 'warp',             # reflection about size instead of size - 1
    'round_half_up': 'warp',                  # round half up instead of half to even
    'zeros_on_one_side': 'warp',              # zeros instead of reflection on one side only
    'filter_weights_transposed': 'filter',    # wgt[dx*k + dy]
    'filter_reflect_edge': 'filter',          # reflection 2H - yy - 1
    'mask_per_image': 'accumulate',           # mask indexed (g*B + b) instead of g
    'map_b_major': 'accumulate',              # map indexed (b*G + g)
    'infinity_not_skipped': 'accumulate',     # views at infinity not skipped
    'sqrt_half_exchanged': 'finalize',        # sqrt and * 0.5 exchanged
    'min_count_le': 'finalize',               # min_count compared with <=
    'desc_w_minus_1': 'desc',                 # descriptor coordinates with W - 1 in place of W
    'desc_xy_exchanged': 'desc',              # descriptor x / y exchanged
    'zero_rows_not_written': 'desc',          # zero rows not written
    'count_not_clipped': 'desc',              # kp_count not clipped to K
}
