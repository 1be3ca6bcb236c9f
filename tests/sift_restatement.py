"""numpy restatement of the SIFT baseline as DESIGN.md 3.19 specifies it (Lowe 2004 with the constants of opencv-contrib 4.2's
sift.cpp) -- written from that text, not from the kernels.  Every stage is a function that can also start from given inputs: the
scale space from a uint8 image, candidates from a difference pyramid, refinement + orientation from pyramids plus a candidate,
the descriptor from a Gaussian layer plus a keypoint record.  `dtype=np.float64` is the model the HIP kernels are tested
against; `dtype=np.float32` runs the same formulas in single precision and gives the rounding noise floor the tolerances of the
GPU tests are derived from.  Pure numpy, no GPU."""
import numpy as np

SIGMA0 = 1.6
LAYERS = 3                     # nOctaveLayers: 6 Gaussian and 5 difference layers per octave
BORDER = 5
CONTRAST = 0.04
EDGE = 10.0
NFEATURES = 1000
ORI_BINS = 36
FLT_EPSILON = float(np.finfo(np.float32).eps)


# ---- scale space ----------------------------------------------------------------------------------------------------------------

def gaussian_taps(sigma):
    """float32 weights of width round(8 sigma + 1) | 1: exp(-x^2 / 2 sigma^2) in double, normalised by the double sum, rounded once"""
    n = int(np.rint(8.0 * sigma + 1.0)) | 1
    x = np.arange(n, dtype=np.float64) - n // 2
    w = np.exp(-x * x / (2.0 * sigma * sigma))
    return (w / w.sum()).astype(np.float32)


def chain_sigmas():
    """[sigma of the base blur, sigma of the blur from layer i-1 to layer i for i = 1 .. 5]"""
    k = 2.0 ** (1.0 / LAYERS)
    out = [np.sqrt(max(SIGMA0 ** 2 - 4 * 0.5 ** 2, 0.01))]
    for i in range(1, LAYERS + 3):
        prev = SIGMA0 * k ** (i - 1)
        out.append(np.sqrt((prev * k) ** 2 - prev ** 2))
    return out


def _pass(img, taps, axis, dtype):
    """one pass of the separable filter along `axis`, BORDER_REFLECT_101, taps added in ascending order"""
    r = len(taps) // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    p = np.pad(img.astype(dtype), pad, mode='reflect')
    n = img.shape[axis]
    acc = np.zeros(img.shape, dtype=dtype)
    for k, w in enumerate(taps):
        sl = [slice(None), slice(None)]
        sl[axis] = slice(k, k + n)
        acc = acc + dtype(w) * p[tuple(sl)]
    return acc


def blur(img, sigma, dtype=np.float64):
    """row pass, rounded to the stored format (float32), then column pass; the result is what the pyramid stores (float32 values)"""
    taps = gaussian_taps(sigma)
    rows = _pass(img, taps, 1, dtype)
    if dtype == np.float64:
        return _pass(rows, taps, 0, dtype)
    return _pass(rows.astype(np.float32), taps, 0, dtype)


def upscale2(u8):
    """cv2.resize(.., fx=2, fy=2, INTER_LINEAR) of the image as float: source coordinate (dst + 0.5) / 2 - 0.5, clamped"""
    src = u8.astype(np.float64)

    def axis_weights(n):
        f = (np.arange(2 * n) + 0.5) / 2.0 - 0.5
        i0 = np.floor(f).astype(int)
        w = f - i0
        w[i0 < 0] = 0.0
        i0[i0 < 0] = 0
        w[i0 >= n - 1] = 0.0
        i0[i0 >= n - 1] = n - 1
        return i0, np.minimum(i0 + 1, n - 1), w

    y0, y1, wy = axis_weights(src.shape[0])
    x0, x1, wx = axis_weights(src.shape[1])
    rows = src[:, x0] * (1 - wx) + src[:, x1] * wx
    return rows[y0] * (1 - wy)[:, None] + rows[y1] * wy[:, None]


def n_octaves(H, W):
    return int(np.rint(np.log2(min(2 * H, 2 * W)) - 2)) + 1


def scale_space(u8, dtype=np.float64, with_bound=False):
    """u8 [H,W] uint8 -> (gauss: list of [6,h,w], dog: list of [5,h,w]) per octave, in `dtype`.  In float64 the planes are the
    exact model (the row pass is not rounded); with_bound=True also returns per-plane bounds of a float32 implementation's error
    (see tests/test_gpu_sift.py for the derivation): (gauss, dog, gauss_bound, dog_bound)."""
    sig = chain_sigmas()
    u = 2.0 ** -24
    gauss, dog, gb, db = [], [], [], []

    def blur_bound(x, xb, s):
        # the input's error passes through the (non-negative, unit-sum) filter; each pass of n taps adds (n + 2) u sum |w x|
        taps = gaussian_taps(s)
        n = len(taps)
        rows = _pass(np.abs(x), taps, 1, np.float64)
        rb = _pass(xb, taps, 1, np.float64) + (n + 2) * u * rows
        out = _pass(rows, taps, 0, np.float64)
        return _pass(rb, taps, 0, np.float64) + (n + 2) * u * out

    base = upscale2(u8)
    bb = np.zeros_like(base)
    for o in range(n_octaves(*u8.shape)):
        g, b = [], []
        for i in range(LAYERS + 3):
            if i == 0 and o == 0:
                g.append(blur(base, sig[0], dtype))
                b.append(blur_bound(base, bb, sig[0]) if with_bound else None)
            elif i == 0:
                g.append(gauss[o - 1][LAYERS][::2, ::2][:gauss[o - 1].shape[1] // 2, :gauss[o - 1].shape[2] // 2].copy())
                b.append(gb[o - 1][LAYERS][::2, ::2][:g[0].shape[0], :g[0].shape[1]].copy() if with_bound else None)
            else:
                g.append(blur(g[i - 1], sig[i], dtype))
                b.append(blur_bound(g[i - 1], b[i - 1], sig[i]) if with_bound else None)
        g = np.stack(g).astype(dtype)
        gauss.append(g)
        dog.append((g[1:] - g[:-1]).astype(dtype))
        if with_bound:
            b = np.stack(b)
            gb.append(b)
            db.append(b[1:] + b[:-1] + u * np.abs(dog[-1]))
    return (gauss, dog, gb, db) if with_bound else (gauss, dog)


# ---- candidates -----------------------------------------------------------------------------------------------------------------

def candidates(dog):
    """dog: list of [5,h,w] -> [(octave, layer, row, column)] in list order: |v| > 1 and v >= (v > 0) or <= (v < 0) all 26 neighbours
    (non-strict), layers 1..3, pixels at least 5 from every border.  Comparisons only: exact on float32 values."""
    thr = np.floor(0.5 * CONTRAST / LAYERS * 255)
    out = []
    for o, d in enumerate(dog):
        _, h, w = d.shape
        if h <= 2 * BORDER or w <= 2 * BORDER:
            continue
        for layer in range(1, LAYERS + 1):
            c = d[layer, BORDER:h - BORDER, BORDER:w - BORDER]
            ge = np.ones(c.shape, bool)
            le = np.ones(c.shape, bool)
            for dl in (-1, 0, 1):
                for dr in (-1, 0, 1):
                    for dc in (-1, 0, 1):
                        n = d[layer + dl, BORDER + dr:h - BORDER + dr, BORDER + dc:w - BORDER + dc]
                        ge &= c >= n
                        le &= c <= n
            keep = (np.abs(c) > thr) & (((c > 0) & ge) | ((c < 0) & le))
            rr, cc = np.nonzero(keep)
            out += [(o, layer, int(r) + BORDER, int(x) + BORDER) for r, x in zip(rr, cc)]
    return out


# ---- refinement + orientation ---------------------------------------------------------------------------------------------------

def _solve3(A, g, dtype):
    """Gaussian elimination with partial pivoting (the first largest pivot) in `dtype`; None for a singular system"""
    A = A.astype(dtype).copy()
    g = g.astype(dtype).copy()
    for col in range(3):
        piv = col + int(np.argmax(np.abs(A[col:, col])))
        if A[piv, col] == 0:
            return None
        if piv != col:
            A[[col, piv]] = A[[piv, col]]
            g[[col, piv]] = g[[piv, col]]
        for r in range(col + 1, 3):
            f = A[r, col] / A[col, col]
            A[r, col + 1:] = A[r, col + 1:] - f * A[col, col + 1:]
            g[r] = g[r] - f * g[col]
    x = np.zeros(3, dtype)
    x[2] = g[2] / A[2, 2]
    x[1] = (g[1] - A[1, 2] * x[2]) / A[1, 1]
    x[0] = (g[0] - A[0, 1] * x[1] - A[0, 2] * x[2]) / A[0, 0]
    return x


def _derivatives(d, layer, r, c, dtype):
    f = dtype
    img, prv, nxt = d[layer].astype(f), d[layer - 1].astype(f), d[layer + 1].astype(f)
    s = f(1.0) / f(255.0)
    ds, ss, cs = s * f(0.5), s, s * f(0.25)
    g = np.array([(img[r, c + 1] - img[r, c - 1]) * ds, (img[r + 1, c] - img[r - 1, c]) * ds, (nxt[r, c] - prv[r, c]) * ds], f)
    v2 = img[r, c] * f(2)
    dxx = (img[r, c + 1] + img[r, c - 1] - v2) * ss
    dyy = (img[r + 1, c] + img[r - 1, c] - v2) * ss
    dss = (nxt[r, c] + prv[r, c] - v2) * ss
    dxy = (img[r + 1, c + 1] - img[r + 1, c - 1] - img[r - 1, c + 1] + img[r - 1, c - 1]) * cs
    dxs = (nxt[r, c + 1] - nxt[r, c - 1] - prv[r, c + 1] + prv[r, c - 1]) * cs
    dys = (nxt[r + 1, c] - nxt[r - 1, c] - prv[r + 1, c] + prv[r - 1, c]) * cs
    return g, np.array([[dxx, dxy, dxs], [dxy, dyy, dys], [dxs, dys, dss]], f)


def refine(dog, cand, dtype=np.float64):
    """One candidate -> dict(fate, ...).  fate 'kept' carries o, layer, r, c, offsets (xc, xr, xi), contr and the record fields x, y,
    size, response in doubled-base coordinates.  Every result carries `margins`: name -> distance of a decision from its
    threshold (offsets: of every offset of every step from the nearest half-integer; contrast, edge: relative)."""
    f = dtype
    o, layer, r, c = cand
    d = dog[o]
    _, h, w = d.shape
    m = {'offset': np.inf}
    x = None
    for step in range(5):
        g, A = _derivatives(d, layer, r, c, f)
        X = _solve3(A, g, f)
        if X is None:
            return {'fate': 'singular', 'margins': m}
        x = -X                                            # (xc, xr, xi)
        m['offset'] = min(m['offset'], float(np.min(np.abs(np.abs(x - np.floor(x)) - 0.5))))
        if np.all(np.abs(x) < 0.5):
            break
        if not np.all(np.abs(x) < 1e6):
            return {'fate': 'diverged', 'margins': m}
        c += int(np.rint(x[0]))
        r += int(np.rint(x[1]))
        layer += int(np.rint(x[2]))
        if layer < 1 or layer > LAYERS or c < BORDER or c >= w - BORDER or r < BORDER or r >= h - BORDER:
            return {'fate': 'left', 'margins': m}
    else:
        return {'fate': 'steps', 'margins': m}
    g, A = _derivatives(d, layer, r, c, f)
    contr = f(d[layer][r, c]) * (f(1.0) / f(255.0)) + (g[0] * x[0] + g[1] * x[1] + g[2] * x[2]) * f(0.5)
    m['contrast'] = float(abs(abs(contr) * LAYERS - CONTRAST) / CONTRAST)
    res = {'margins': m, 'o': o, 'layer': layer, 'r': r, 'c': c, 'offsets': x, 'contr': contr}
    if abs(contr) * f(LAYERS) < f(CONTRAST):
        return dict(res, fate='contrast')
    dxx, dyy, dxy = A[0, 0], A[1, 1], A[0, 1]
    tr, det = dxx + dyy, dxx * dyy - dxy * dxy
    m['edge'] = float(min(abs(det) / (abs(dxx * dyy) + dxy * dxy + 1e-300),
                          abs(tr * tr * EDGE - (EDGE + 1) ** 2 * det) / (tr * tr * EDGE + (EDGE + 1) ** 2 * abs(det) + 1e-300)))
    if det <= 0 or tr * tr * f(EDGE) >= f((EDGE + 1) ** 2) * det:
        return dict(res, fate='edge')
    scale = f(2 ** o)
    size = f(SIGMA0) * np.exp2((f(layer) + x[2]) / f(LAYERS)) * scale * f(2)
    return dict(res, fate='kept', x=(f(c) + x[0]) * scale, y=(f(r) + x[1]) * scale, size=size, response=abs(contr))


def _angles(dy, dx, dtype):
    a = np.arctan2(dy, dx) * dtype(180.0 / np.pi)
    a = np.where(a < 0, a + dtype(360), a)
    return np.where(a >= 360, dtype(0), a).astype(dtype)


def orientation_histogram(layer_img, r, c, scl, dtype=np.float64):
    """-> (smoothed 36-bin histogram, margin of the window radius's rounding, smallest distance (in bins) of a sample that
    matters from a bin boundary)"""
    f = dtype
    img = layer_img.astype(f)
    h, w = img.shape
    radius = int(np.rint(f(4.5) * scl))
    m_radius = float(abs(abs(float(f(4.5) * scl) - np.floor(float(f(4.5) * scl))) - 0.5))
    sigma = f(1.5) * scl
    scale = f(-1.0) / (f(2) * sigma * sigma)
    ii, jj = np.meshgrid(np.arange(-radius, radius + 1), np.arange(-radius, radius + 1), indexing='ij')
    y, x = r + ii, c + jj
    ok = (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
    y, x, ii, jj = y[ok], x[ok], ii[ok], jj[ok]
    dx = img[y, x + 1] - img[y, x - 1]
    dy = img[y - 1, x] - img[y + 1, x]
    wgt = np.exp((ii * ii + jj * jj).astype(f) * scale)
    pos = _angles(dy, dx, f) * f(ORI_BINS / 360.0)
    bins = np.rint(pos).astype(int) % ORI_BINS
    vote = wgt * np.sqrt(dx * dx + dy * dy)
    raw = np.zeros(ORI_BINS, f)
    np.add.at(raw, bins, vote)
    sm = ((np.roll(raw, 2) + np.roll(raw, -2)) * f(1 / 16) + (np.roll(raw, 1) + np.roll(raw, -1)) * f(4 / 16) + raw * f(6 / 16)).astype(f)
    matter = vote > 1e-4 * max(float(sm.max()), 1e-300)
    m_bin = float(np.min(np.abs(np.abs(pos[matter] - np.floor(pos[matter])) - 0.5))) if matter.any() else np.inf
    return sm, m_radius, m_bin


def orientations(hist, dtype=np.float64):
    """-> ([(bin, angle)], decisions: per bin (is a peak, relative margin of that decision))"""
    f = dtype
    mx = hist.max()
    out, dec = [], []
    for j in range(ORI_BINS):
        left, right = hist[(j - 1) % ORI_BINS], hist[(j + 1) % ORI_BINS]
        tests = [(hist[j] > left, abs(hist[j] - left)), (hist[j] > right, abs(hist[j] - right)), (hist[j] >= f(0.8) * mx, abs(hist[j] - f(0.8) * mx))]
        peak = all(t for t, _ in tests)
        # a peak needs all three tests to hold firmly; a non-peak one test to fail firmly
        margin = min(d for _, d in tests) if peak else max(d for t, d in tests if not t)
        dec.append((peak, float(margin) / max(float(mx), 1e-300)))
        if peak:
            b = f(j) + f(0.5) * (left - right) / (left - f(2) * hist[j] + right)
            b = f(ORI_BINS) + b if b < 0 else (b - f(ORI_BINS) if b >= ORI_BINS else b)
            angle = f(360) - f(360.0 / ORI_BINS) * b
            if abs(angle - f(360)) < FLT_EPSILON:
                angle = f(0)
            out.append((j, angle))
    return out, dec


def detect_candidate(gauss, dog, cand, dtype=np.float64):
    """refinement + orientation of one candidate -> the refine() dict plus, for kept ones, `records` [(x, y, size, angle, response,
    octave * 8 + layer)] in doubled-base coordinates, `bins`, and the orientation margins"""
    res = refine(dog, cand, dtype)
    if res['fate'] != 'kept':
        return res
    f = dtype
    scl = res['size'] * f(0.5) / f(2 ** res['o'])
    hist, m_radius, m_bin = orientation_histogram(gauss[res['o']][res['layer']], res['r'], res['c'], scl, f)
    peaks, dec = orientations(hist, f)
    res['margins'].update(radius=m_radius, sample=m_bin, histogram=min(mg for _, mg in dec))
    res['bins'] = [j for j, _ in peaks]
    res['hist'] = hist
    res['records'] = [(res['x'], res['y'], res['size'], a, res['response'], f(res['o'] * 8 + res['layer'])) for _, a in peaks]
    return res


def detect_records(gauss, dog, dtype=np.float64, capacity=None):
    """-> float [n,6] records in list order (octave, layer, row, column of the candidate, then orientation bin), doubled-base
    coordinates; with a capacity both lists are cut to it from the end, as the kernels do"""
    cands = candidates(dog)
    if capacity is not None:
        cands = cands[:capacity]
    recs = []
    for cd in cands:
        recs += detect_candidate(gauss, dog, cd, dtype).get('records', [])
    if capacity is not None:
        recs = recs[:capacity]
    return np.array(recs, dtype=np.float64).reshape(-1, 6)


# ---- selection ------------------------------------------------------------------------------------------------------------------

def select(records, nfeatures=NFEATURES):
    """records [n,6] (doubled-base coordinates) -> [m,6] in frame coordinates: an entry whose (x, y, size, angle) equals an earlier
    one's is dropped; the nfeatures largest responses are kept, a tie at the cut going to the earlier entry; list order is kept;
    x, y, size are halved.  (OpenCV's retainBest keeps every entry tied with the cut: a stated deviation.)"""
    records = np.asarray(records, dtype=np.float64).reshape(-1, 6)
    seen, keep = set(), []
    for i, rec in enumerate(records):
        key = tuple(rec[:4])
        if key not in seen:
            seen.add(key)
            keep.append(i)
    keep = np.array(keep, dtype=int)
    if len(keep) > nfeatures:
        order = np.lexsort((keep, -records[keep, 4]))           # response descending, then position ascending
        keep = np.sort(keep[order[:nfeatures]])
    out = records[keep].copy()
    out[:, :3] *= 0.5
    return out


# ---- descriptor -----------------------------------------------------------------------------------------------------------------

def describe(gauss, kp, dtype=np.float64, quantise=True):
    """kp = (x, y, size, angle, response, octave * 8 + layer) in FRAME coordinates -> the 128 values [row][column][orientation]
    (quantise=False: the scaled values before rounding and saturation)"""
    f = dtype
    code = int(kp[5])
    o, layer = code >> 3, code & 7
    img = gauss[o][layer].astype(f)
    h, w = img.shape
    inv = f(2.0) / f(2 ** o)
    px, py = int(np.rint(f(kp[0]) * inv)), int(np.rint(f(kp[1]) * inv))
    scl = f(kp[2]) * inv * f(0.5)
    ori = f(360) - f(kp[3])
    if abs(ori - f(360)) < FLT_EPSILON:
        ori = f(0)
    hist_width = f(3) * scl
    radius = int(np.rint(hist_width * f(1.4142135623730951) * f(5) * f(0.5)))
    radius = min(radius, int(np.sqrt(float(h) * h + float(w) * w)))
    cos_t = np.cos(ori * f(np.pi / 180)) / hist_width
    sin_t = np.sin(ori * f(np.pi / 180)) / hist_width
    ii, jj = np.meshgrid(np.arange(-radius, radius + 1), np.arange(-radius, radius + 1), indexing='ij')
    ii, jj = ii.ravel(), jj.ravel()
    c_rot = jj.astype(f) * cos_t - ii.astype(f) * sin_t
    r_rot = jj.astype(f) * sin_t + ii.astype(f) * cos_t
    rbin, cbin = r_rot + f(1.5), c_rot + f(1.5)
    y, x = py + ii, px + jj
    ok = (rbin > -1) & (rbin < 4) & (cbin > -1) & (cbin < 4) & (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
    y, x, rbin, cbin, c_rot, r_rot = y[ok], x[ok], rbin[ok], cbin[ok], c_rot[ok], r_rot[ok]
    dx = img[y, x + 1] - img[y, x - 1]
    dy = img[y - 1, x] - img[y + 1, x]
    obin = (_angles(dy, dx, f) - ori) * f(8 / 360.0)
    mag = np.sqrt(dx * dx + dy * dy) * np.exp((c_rot * c_rot + r_rot * r_rot) * f(-1.0 / 8.0))
    r0, c0, o0 = np.floor(rbin), np.floor(cbin), np.floor(obin)
    fr, fc, fo = (rbin - r0).astype(f), (cbin - c0).astype(f), (obin - o0).astype(f)
    r0, c0, o0 = r0.astype(int), c0.astype(int), o0.astype(int) % 8
    hist = np.zeros((4, 4, 8), f)
    for dr in (0, 1):
        vr = mag * fr if dr else mag - mag * fr
        for dc in (0, 1):
            vrc = vr * fc if dc else vr - vr * fc
            for do in (0, 1):
                v = vrc * fo if do else vrc - vrc * fo
                rr, cc = r0 + dr, c0 + dc
                inside = (rr >= 0) & (rr < 4) & (cc >= 0) & (cc < 4)
                np.add.at(hist, (rr[inside], cc[inside], (o0[inside] + do) % 8), v[inside].astype(f))
    vals = hist.ravel()
    thr = np.sqrt((vals * vals).sum(dtype=f)) * f(0.2)
    vals = np.minimum(vals, thr)
    vals = vals * (f(512) / max(np.sqrt((vals * vals).sum(dtype=f)), f(FLT_EPSILON)))
    if not quantise:
        return vals
    return np.clip(np.rint(vals), 0, 255).astype(np.float64)


# ---- adapter --------------------------------------------------------------------------------------------------------------------

def scatter(keypoints, H, W):
    """-> (prob [H,W]: 1.0 at (round(y), round(x)) of every keypoint; owner [H,W]: the last list index rounding there, -1 elsewhere)"""
    prob = np.zeros((H, W), np.float32)
    owner = np.full((H, W), -1, np.int32)
    for k, kp in enumerate(keypoints):
        x, y = int(np.rint(np.float32(kp[0]))), int(np.rint(np.float32(kp[1])))
        if 0 <= x < W and 0 <= y < H:
            prob[y, x] = 1.0
            owner[y, x] = k
    return prob, owner


def detect_and_describe(u8, nfeatures=NFEATURES, dtype=np.float64):
    """the whole chain on one frame -> (keypoints [n,6] in frame coordinates, descriptors [n,128])"""
    gauss, dog = scale_space(u8, dtype)
    if dtype == np.float64:          # the pyramid is stored in float32: the later stages read the stored values
        gauss = [g.astype(np.float32) for g in gauss]
        dog = [(g[1:] - g[:-1]) for g in gauss]
    kps = select(detect_records(gauss, dog, dtype), nfeatures)
    desc = np.array([describe(gauss, kp, dtype) for kp in kps]).reshape(-1, 128)
    return kps, desc


def mutual_matches(da, db):
    """mutual nearest neighbours of unit rows -> [(i, j)]"""
    if len(da) == 0 or len(db) == 0:
        return np.zeros((0, 2), int)
    d = da @ db.T
    ab, ba = d.argmax(1), d.argmax(0)
    i = np.arange(len(da))
    keep = ba[ab] == i
    return np.stack((i[keep], ab[keep]), 1)
