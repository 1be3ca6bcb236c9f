"""float64 numpy restatement of the Fourier-Mellin registration (multipoint_amd/csrc/register.hip): the four
stages and the driver, written from the specification.  The coordinates are the kernels' own fp32 fused multiply-adds (they
decide which pixels are zero and where a sample lies); everything after them is float64.  The tables are the fp32 ones the
host builds (multipoint_amd.utils.registration)."""
import math

import numpy as np

from multipoint_amd.utils.registration import fft_length_at_least, hann_table, logpolar_tables


def fmaf(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64, the sum is rounded there and once more to
    fp32 (a double rounding that differs from the true fmaf only when the float64 sum lands on an fp32 midpoint)."""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def tap_coordinates(H, W, c, s, dx, dy):
    """fp32 source coordinates (sx, sy), each [H,W], of the tap (x + dx, y + dy) of every output pixel through the similarity
    (c, s) about the frame centre."""
    cx, cy = np.float32((W - 1) * 0.5), np.float32((H - 1) * 0.5)
    px = (np.arange(W, dtype=np.float32) + np.float32(dx) - cx)[None, :].repeat(H, 0)
    py = (np.arange(H, dtype=np.float32) + np.float32(dy) - cy)[:, None].repeat(W, 1)
    c, s = np.float32(c), np.float32(s)
    sx = fmaf(c, px, fmaf(-s, py, cx))
    sy = fmaf(s, px, fmaf(c, py, cy))
    return sx, sy


def _bilinear(f, sx, sy):
    """(value float64, inside bool): bilinear sample of f [H,W] at fp32 coordinates; inside where all four samples are."""
    H, W = f.shape
    x0f, y0f = np.floor(sx), np.floor(sy)
    inside = (x0f >= 0) & (y0f >= 0) & (x0f <= W - 2) & (y0f <= H - 2)
    x0 = np.clip(x0f, 0, W - 2).astype(np.int64)
    y0 = np.clip(y0f, 0, H - 2).astype(np.int64)
    fx = (sx - x0f).astype(np.float64)       # exact in fp32
    fy = (sy - y0f).astype(np.float64)
    f = f.astype(np.float64)
    top = f[y0, x0] + fx * (f[y0, x0 + 1] - f[y0, x0])
    bot = f[y0 + 1, x0] + fx * (f[y0 + 1, x0 + 1] - f[y0 + 1, x0])
    return top + fy * (bot - top), inside


def prepare(frames, N, cs=None, border=None):
    """frames [n,H,W] -> float64 [n,N,N] (the real part; the imaginary part is 0).  border: a list that receives, per frame, the
    mask [N,N] of pixels with a tap coordinate within 1e-4 of the frame border (the pixels whose zero test may flip)."""
    frames = np.asarray(frames, np.float32)
    n, H, W = frames.shape
    wy, wx = hann_table(H).astype(np.float64), hann_table(W).astype(np.float64)
    oy, ox = (N - H) // 2, (N - W) // 2
    out = np.zeros((n, N, N))
    for i in range(n):
        c, s = (1.0, 0.0) if cs is None else cs[i]
        vals, ok, near = [], np.ones((H, W), bool), np.zeros((H, W), bool)
        for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            sx, sy = tap_coordinates(H, W, c, s, dx, dy)
            v, inside = _bilinear(frames[i], sx, sy)
            vals.append(v)
            ok &= inside
            for coord, size in ((sx, W), (sy, H)):
                near |= (np.abs(coord.astype(np.float64)) < 1e-4) | (np.abs(coord.astype(np.float64) - (size - 1)) < 1e-4)
        gx, gy = 0.5 * (vals[0] - vals[1]), 0.5 * (vals[2] - vals[3])
        mag = np.sqrt(gx * gx + gy * gy) * wy[:, None] * wx[None, :]
        out[i, oy:oy + H, ox:ox + W] = np.where(ok, mag, 0.0)
        if border is not None:
            m = np.zeros((N, N), bool)
            m[oy:oy + H, ox:ox + W] = near
            border.append(m)
    return out


def logpolar(spectrum, A, R, r_min=None):
    """spectrum complex [n,N,N] in FFT order -> float64 [n,A,R]."""
    spectrum = np.asarray(spectrum)
    n, N = spectrum.shape[0], spectrum.shape[1]
    ca, sa, rho, wr, _ = logpolar_tables(N, A, R, r_min)
    half = np.float32(N // 2)
    x = fmaf(rho[None, :], ca[:, None], half)
    y = fmaf(rho[None, :], sa[:, None], half)
    x0f, y0f = np.floor(x), np.floor(y)
    fx, fy = (x - x0f).astype(np.float64), (y - y0f).astype(np.float64)
    x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
    out = np.zeros((n, A, R))
    for i in range(n):
        mag = np.log1p(np.abs(spectrum[i].astype(np.complex128)))

        def at(yy, xx):          # the fftshifted plane: index i of it is index (i - N / 2) mod N of the spectrum
            return mag[(yy - N // 2) % N, (xx - N // 2) % N]
        top = at(y0, x0) + fx * (at(y0, x0 + 1) - at(y0, x0))
        bot = at(y0 + 1, x0) + fx * (at(y0 + 1, x0 + 1) - at(y0 + 1, x0))
        out[i] = (top + fy * (bot - top)) * wr.astype(np.float64)[None, :]
    return out


def cross_power(a, b, group_offsets):
    """a, b complex [P,h,w] -> complex128 [G,h,w]: per group the sum in pair order of a conj(b) / |a conj(b)| (0 where that is
    0); bin (0, 0) is 0."""
    a, b = np.asarray(a).astype(np.complex128), np.asarray(b).astype(np.complex128)
    go = np.asarray(group_offsets).astype(np.int64)
    out = np.zeros((len(go) - 1,) + a.shape[1:], np.complex128)
    for g in range(len(go) - 1):
        for p in range(go[g], go[g + 1]):
            x = a[p] * np.conj(b[p])
            m = np.abs(x)
            out[g] += np.where(m > 0, x / np.where(m > 0, m, 1.0), 0.0)
        out[g, 0, 0] = 0.0
    return out


def peak(plane):
    """plane [h,w] real -> dict(index (y, x), offset (oy, ox), signed (y, x), peak, second)."""
    plane = np.asarray(plane, np.float64)
    h, w = plane.shape
    flat = int(np.argmax(plane))             # the first maximum in row-major order
    y, x = divmod(flat, w)

    def parabola(l, c, r):
        d = l - 2.0 * c + r
        return 0.0 if d == 0.0 else 0.5 * (l - r) / d
    c = plane[y, x]
    oy = parabola(plane[(y - 1) % h, x], c, plane[(y + 1) % h, x])
    ox = parabola(plane[y, (x - 1) % w], c, plane[y, (x + 1) % w])
    dy = (np.arange(h) - y) % h
    dx = (np.arange(w) - x) % w
    block = ((dy <= 1) | (dy == h - 1))[:, None] & ((dx <= 1) | (dx == w - 1))[None, :]
    rest = plane[~block]
    second = float(rest.max()) if rest.size else -math.inf
    sy = y - h if y > h // 2 else y
    sx = x - w if x > w // 2 else x
    return dict(index=(y, x), offset=(oy, ox), signed=(sy + oy, sx + ox), peak=float(c), second=second)


def correlation_surface(a, b, group_offsets):
    """[G,h,w] real surfaces of planes a, b [P,h,w]: ifft2(cross_power(fft2 a, fft2 b)) (numpy's inverse divides by h w)."""
    x = cross_power(np.fft.fft2(a), np.fft.fft2(b), group_offsets)
    return np.fft.ifft2(x).real


def compose(cs, signed_yx, optical_hw, thermal_hw, N):
    """The optical -> thermal matrix: A = [[c, -s], [s, c]], tau = off_o - off_t - peak, d = Ct - A (Ct - tau)."""
    (Ho, Wo), (Ht, Wt) = optical_hw, thermal_hw
    c, s = float(cs[0]), float(cs[1])
    A = np.array([[c, -s], [s, c]])
    tau = (np.array([(N - Wo) // 2, (N - Ho) // 2], np.float64) - np.array([(N - Wt) // 2, (N - Ht) // 2], np.float64)
           - np.array([signed_yx[1], signed_yx[0]], np.float64))
    ct = np.array([(Wt - 1) / 2.0, (Ht - 1) / 2.0])
    T = np.eye(3)
    T[:2, :2] = A
    T[:2, 2] = ct - A @ (ct - tau)
    return T


def estimate(optical, thermal, group_offsets=None, angles=None, radii=None, r_min=None):
    """The driver: optical [P,Ho,Wo], thermal [P,Ht,Wt] -> dict(T [G,3,3], theta, scale, cs [G,2] fp32, pk1, pk2 (lists of peak
    dicts; pk2 of the chosen branch), branch [G], surface1 [G,A,R], surface2 [2][G,N,N])."""
    optical, thermal = np.asarray(optical, np.float32), np.asarray(thermal, np.float32)
    P = optical.shape[0]
    go = np.arange(P + 1) if group_offsets is None else np.asarray(group_offsets).astype(np.int64)
    G = len(go) - 1
    N = fft_length_at_least(max(optical.shape[1:] + thermal.shape[1:]))
    A = fft_length_at_least(N) if angles is None else angles
    R = fft_length_at_least(N) if radii is None else radii
    step = logpolar_tables(N, A, R, r_min)[4]
    po, pt = prepare(optical, N), prepare(thermal, N)
    fo = np.fft.fft2(po)
    lo, lt = logpolar(fo, A, R, r_min), logpolar(np.fft.fft2(pt), A, R, r_min)
    s1 = correlation_surface(lo, lt, go)
    pk1 = [peak(s1[g]) for g in range(G)]
    theta = np.array([-p['signed'][0] * (math.pi / A) for p in pk1])
    scale = np.array([math.exp(p['signed'][1] * step) for p in pk1])
    cs = np.stack([scale * np.cos(theta), scale * np.sin(theta)], 1).astype(np.float32)
    gid = np.repeat(np.arange(G), np.diff(go))
    s2 = []
    for sign in (1.0, -1.0):
        ptb = prepare(thermal, N, (np.float32(sign) * cs)[gid])
        s2.append(np.fft.ifft2(cross_power(fo, np.fft.fft2(ptb), go)).real)
    cand = [[peak(s2[b][g]) for g in range(G)] for b in range(2)]
    branch = np.array([1 if cand[1][g]['peak'] > cand[0][g]['peak'] else 0 for g in range(G)])
    pk2 = [cand[branch[g]][g] for g in range(G)]
    T = np.stack([compose((1.0, -1.0)[branch[g]] * cs[g].astype(np.float64), pk2[g]['signed'], optical.shape[1:],
                          thermal.shape[1:], N) for g in range(G)])
    return dict(T=T, theta=theta, scale=scale, cs=cs, pk1=pk1, pk2=pk2, branch=branch, surface1=s1, surface2=s2, N=N, A=A, R=R)
