"""A float64 numpy restatement of the sub-pixel keypoint refinement (include/multipoint_hip.h: mp_refine_keypoints), written
from its specification and independent of the kernel: per axis the vertex of the parabola through the logarithms of the map
at the keypoint and its two neighbours.  Test infrastructure: the host tests pin it on planted Gaussian blobs and on every
"axis not refined" branch, the GPU tests hold the kernel to it."""
import numpy as np


def refine_axis(pm, p0, pp, inside=True):
    """One axis.  Returns (delta, refined, terms) with terms = (|l-|, |l0|, |l+|, |den|) where refined (else zeros): what the
    kernel's fp32 error bound is made of."""
    ok = bool(inside)
    for p in (pm, p0, pp):
        ok = ok and np.isfinite(p) and p > 0
    ok = ok and p0 >= pm and p0 >= pp
    if not ok:
        return 0.0, False, (0.0, 0.0, 0.0, 0.0)
    lm, l0, lp = np.log(np.float64(pm)), np.log(np.float64(p0)), np.log(np.float64(pp))
    den = lm - 2.0 * l0 + lp
    if not den < 0:
        return 0.0, False, (0.0, 0.0, 0.0, 0.0)
    return 0.5 * (lm - lp) / den, True, (abs(lm), abs(l0), abs(lp), abs(den))


def refine_keypoints(prob, kp_yx, kp_count):
    """prob [B,H,W], kp_yx [B,K,2] integer (y, x), kp_count [B].  Returns (sub [B,K,2] float64, refined [B,K,2] bool,
    bound [B,K,2] float64): rows k >= min(kp_count[b], K) are zero; bound is the per-axis fp32 error bound
    8 * 2^-23 * (|l-| + 2 |l0| + |l+|) / |den| + 1e-6 (<= 2 ulp for each logf, first-order sensitivity of the quotient; 1e-6
    where the axis is not refined)."""
    prob = np.asarray(prob)
    kp_yx = np.asarray(kp_yx)
    B, H, W = prob.shape
    K = kp_yx.shape[1]
    sub = np.zeros((B, K, 2), np.float64)
    refined = np.zeros((B, K, 2), bool)
    bound = np.zeros((B, K, 2), np.float64)
    for b in range(B):
        for k in range(min(int(kp_count[b]), K)):
            y, x = int(kp_yx[b, k, 0]), int(kp_yx[b, k, 1])
            p0 = prob[b, y, x]
            in_y, in_x = 1 <= y < H - 1, 1 <= x < W - 1
            axes = ((y, in_y, prob[b, y - 1, x] if in_y else 0.0, prob[b, y + 1, x] if in_y else 0.0),
                    (x, in_x, prob[b, y, x - 1] if in_x else 0.0, prob[b, y, x + 1] if in_x else 0.0))
            for a, (c, inside, pm, pp) in enumerate(axes):
                d, r, (am, a0, ap, aden) = refine_axis(pm, p0, pp, inside)
                sub[b, k, a] = c + d
                refined[b, k, a] = r
                bound[b, k, a] = (8.0 * 2.0 ** -23 * (am + 2.0 * a0 + ap) / aden if r else 0.0) + 1e-6
    return sub, refined, bound


def render_blobs(H, W, centres_yx, sigma, amplitude=0.5, dtype=np.float64):
    """amplitude * exp(-r^2 / (2 sigma^2)) around every centre, without background: a pixel holds the blob that is strongest
    there (the maximum, not the sum), so around a centre the map is ONE Gaussian exactly whatever its width -- a sum would add
    the tails of the neighbours 10 px away, exp(-12.5) = 4e-6 of a peak at sigma = 2, which is a background."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((H, W), np.float64)
    for cy, cx in np.asarray(centres_yx, np.float64):
        out = np.maximum(out, amplitude * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * sigma * sigma)))
    return out.astype(dtype)


def planted_centres(rng, H, W, n, spacing=10, border=6, max_fraction=0.45):
    """n centres on a jittered grid: integer parts >= `spacing` apart and >= `border` from the frame's edge, fractional parts
    in [-max_fraction, max_fraction].  Returns (centres [n,2] float64, their integer parts [n,2] int64)."""
    ys = np.arange(border, H - border, spacing)
    xs = np.arange(border, W - border, spacing)
    cells = np.array([(y, x) for y in ys for x in xs], np.int64)
    if len(cells) < n:
        raise ValueError('a %d x %d frame holds %d centres %d apart, not %d' % (H, W, len(cells), spacing, n))
    base = cells[np.sort(rng.choice(len(cells), n, replace=False))]
    return base + rng.uniform(-max_fraction, max_fraction, (n, 2)), base
