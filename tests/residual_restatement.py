"""numpy restatement of the local residual field (include/multipoint_hip.h mp_residual_field), written from its
specification with plain loops over windows and displacements: the model csrc/residual.hip and multipoint_amd.utils.residual are
tested against.  Everything is float64; f32=True rounds the three per-pixel products to float32 before they are added, as the
kernel does, which measures how far fp32 products move a score (residual_cases.F32_DIFFERENCE).

  grid        the window origins of a frame
  scores      the (2r + 1)^2 scores and counts of one window
  window      the record of one window from its scores
  field       all windows of one pair of feature frames
  batch       field over a stack of pairs
"""
import numpy as np

F32 = np.float32
OK, FEW_VALID, FLAT, AT_EDGE = 0, 1, 2, 3
WINDOWS = (8, 16, 24, 32, 48, 64)


def grid(H, W, w, s, r):
    """(ys, xs): the window origins r + i s with origin + w + r <= size; ValueError for what the entry refuses."""
    if w not in WINDOWS or s < 1 or not 1 <= r <= 8 or not (8 <= H <= 4096 and 8 <= W <= 4096):
        raise ValueError('residual field: window %r, stride %r, radius %r, frame %dx%d' % (w, s, r, H, W))
    if H < w + 2 * r or W < w + 2 * r:
        raise ValueError('residual field: a %dx%d frame holds no window of %d + 2 x %d pixels' % (H, W, w, r))
    return np.arange(r, H - w - r + 1, s), np.arange(r, W - w - r + 1, s)


def scores(fo, ft, mask, y0, x0, w, r, min_valid, var_floor, f32):
    """(score [2r+1][2r+1] float64 with NaN = undefined, count [2r+1][2r+1]) of the window at (y0, x0)."""
    side = 2 * r + 1
    sc = np.full((side, side), np.nan)
    cnt = np.zeros((side, side), np.int64)
    t = ft[y0:y0 + w, x0:x0 + w].astype(np.float64)
    need = min_valid * float(w * w)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            o = fo[y0 + dy:y0 + dy + w, x0 + dx:x0 + dx + w].astype(np.float64)
            use = np.ones((w, w), bool) if mask is None else mask[y0 + dy:y0 + dy + w, x0 + dx:x0 + dx + w] != 0
            n = int(use.sum())
            cnt[dy + r, dx + r] = n
            if n == 0 or float(n) < need:
                continue
            tv, ov = t[use], o[use]
            tt, oo, to = tv * tv, ov * ov, tv * ov                     # exact: the factors are float32 values
            if f32:
                tt, oo, to = (v.astype(F32).astype(np.float64) for v in (tt, oo, to))
            st, so, stt, soo, sto = tv.sum(), ov.sum(), tt.sum(), oo.sum(), to.sum()
            mt, mo = st / n, so / n
            ctt, coo, cto = stt - mt * st, soo - mo * so, sto - mt * so
            if ctt > var_floor * n and coo > var_floor * n:
                sc[dy + r, dx + r] = cto / (np.sqrt(ctt) * np.sqrt(coo))
    return sc, cnt


def parabola(a, b, c):
    den = (a - 2.0 * b) + c
    if not den < 0.0:
        return 0.0
    return float(min(max(0.5 * (a - c) / den, -0.5), 0.5))


def window(sc, cnt, w, r, min_valid):
    """dict(d (2,), rho, rho0, second, n, status, gap) of one window; gap: the best score minus the runner-up over ALL other
    displacements (inf with one defined score, NaN with none) -- how well the integer peak is determined."""
    side = 2 * r + 1
    nan = float('nan')
    out = dict(d=(nan, nan), rho=nan, rho0=nan, second=nan, n=int(cnt[r, r]), status=FLAT, gap=nan)
    if float(cnt[r, r]) < min_valid * float(w * w):
        out['status'] = FEW_VALID
        return out
    best, at = None, None
    for iy in range(side):                                             # row-major from -r: the first of equal scores stays
        for ix in range(side):
            v = sc[iy, ix]
            if v == v and (best is None or v > best):
                best, at = v, (iy, ix)
    if best is None:
        return out
    by, bx = at
    second, runner = -np.inf, -np.inf
    for iy in range(side):
        for ix in range(side):
            v = sc[iy, ix]
            if not v == v or (iy, ix) == at:
                continue
            runner = max(runner, v)
            if abs(iy - by) > 1 or abs(ix - bx) > 1:
                second = max(second, v)
    fy = fx = 0.0
    edge_y, edge_x = by in (0, side - 1), bx in (0, side - 1)
    if not edge_y and sc[by - 1, bx] == sc[by - 1, bx] and sc[by + 1, bx] == sc[by + 1, bx]:
        fy = parabola(sc[by - 1, bx], best, sc[by + 1, bx])
    if not edge_x and sc[by, bx - 1] == sc[by, bx - 1] and sc[by, bx + 1] == sc[by, bx + 1]:
        fx = parabola(sc[by, bx - 1], best, sc[by, bx + 1])
    out.update(d=(by - r + fy, bx - r + fx), rho=float(best), rho0=float(sc[r, r]), second=float(second), n=int(cnt[by, bx]),
               status=AT_EDGE if (edge_y or edge_x) else OK, gap=float(best - runner))
    return out


def field(fo, ft, mask=None, w=32, s=16, r=8, min_valid=0.5, var_floor=1e-7, f32=False):
    """The residual field of one pair of float32 feature frames (H, W), mask (H, W) or None: a dict of arrays d (gy, gx, 2),
    rho, rho0, second, gap (gy, gx) float64, n, status (gy, gx) int64 and origin (gy, gx, 2)."""
    fo, ft = np.asarray(fo, F32), np.asarray(ft, F32)
    H, W = ft.shape
    assert fo.shape == ft.shape and (mask is None or mask.shape == ft.shape)
    if not 0.0 < min_valid <= 1.0 or not (var_floor >= 0.0 and np.isfinite(var_floor)):
        raise ValueError('residual field: min_valid %r, var_floor %r' % (min_valid, var_floor))
    ys, xs = grid(H, W, w, s, r)
    gy, gx = len(ys), len(xs)
    out = dict(d=np.full((gy, gx, 2), np.nan), rho=np.full((gy, gx), np.nan), rho0=np.full((gy, gx), np.nan),
               second=np.full((gy, gx), np.nan), gap=np.full((gy, gx), np.nan), n=np.zeros((gy, gx), np.int64),
               status=np.zeros((gy, gx), np.int64), origin=np.stack(np.meshgrid(ys, xs, indexing='ij'), -1))
    for i, y0 in enumerate(ys):
        for j, x0 in enumerate(xs):
            sc, cnt = scores(fo, ft, mask, int(y0), int(x0), w, r, min_valid, var_floor, f32)
            rec = window(sc, cnt, w, r, min_valid)
            for k in ('d', 'rho', 'rho0', 'second', 'gap', 'n', 'status'):
                out[k][i, j] = rec[k]
    return out


def batch(fo, ft, mask=None, **kw):
    """field() of every frame of (B, H, W) stacks; mask None, (H, W) shared or (B, H, W).  Arrays gain a leading B (origin not)."""
    recs = [field(fo[b], ft[b], None if mask is None else (mask if mask.ndim == 2 else mask[b]), **kw) for b in range(len(ft))]
    out = {k: np.stack([q[k] for q in recs]) for k in recs[0] if k != 'origin'}
    out['origin'] = recs[0]['origin']
    return out
