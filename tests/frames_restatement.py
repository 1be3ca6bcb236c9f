"""numpy restatement of the frame preparation (reference create_dataset/extract_images.py:167-242): the model
csrc/frames.hip and multipoint_amd/utils/frames.py are held to, bit for bit.  numpy only: no torch, no GPU, no cv2.

  optimal_new_camera_matrix   cv2.getOptimalNewCameraMatrix(K, D, (w, h), alpha)[0], five fixed-point iterations
  undistort                   cv2.undistort(src, K, D, None, K_new) for uint8 (H, W, 3) and uint16 (H, W), optionally rotated
  resize_bgr8                 cv2.resize(src, (ow, oh)), INTER_LINEAR, the 11-bit fixed-point path of 8-bit images
  percentile_bounds           np.percentile(x, 1), np.percentile(x, 99) from the four order statistics they interpolate between
  thermal_rescale             the 1 % / 99 % clip as numpy assigns it, cv2.normalize(NORM_MINMAX, CV_32F), the saved 16-bit form
  prepare_frames              preprocess_images' sequence on one pair

**Not verified against OpenCV**: no `cv2` exists where this was developed; DESIGN.md 3.13 is the specification.  Every float64
and float32 step is one rounded operation (numpy never contracts a multiply and an add), in the order written here."""
import numpy as np

INT32_MIN, INT32_MAX = -2147483648, 2147483647
DBL_EPSILON = 2.220446049250313e-16


# ---------------------------------------------------------------------------------------------------------------- camera model
def camera(K, D):
    """(fx, fy, cx, cy), (k1, k2, p1, p2, k3) as Python floats; four or five coefficients, anything else is ValueError."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    D = np.asarray(D, np.float64).reshape(-1)
    if D.size not in (4, 5):
        raise ValueError('4 or 5 distortion coefficients (k1, k2, p1, p2[, k3]), got %d' % D.size)
    d = [float(v) for v in D] + [0.0] * (5 - D.size)
    return (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])), tuple(d)


def distort_normalised(x, y, d):
    """the radial-tangential model on normalised coordinates (float64 arrays), + - * only, in this order"""
    k1, k2, p1, p2, k3 = d
    r2 = x * x + y * y
    kr = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
    xy2 = (2.0 * x) * y
    xd = (x * kr + p1 * xy2) + p2 * (r2 + (2.0 * x) * x)
    yd = (y * kr + p1 * (r2 + (2.0 * y) * y)) + p2 * xy2
    return xd, yd


def source_position(K, D, K_new, H, W):
    """(us, vs): the float64 source position of every destination pixel, (H, W) each"""
    (fx, fy, cx, cy), d = camera(K, D)
    (fxn, fyn, cxn, cyn), _ = camera(K_new, D)
    u = np.arange(W, dtype=np.float64)[None, :] + np.zeros((H, 1))
    v = np.arange(H, dtype=np.float64)[:, None] + np.zeros((1, W))
    x = (u - cxn) / fxn
    y = (v - cyn) / fyn
    xd, yd = distort_normalised(x, y, d)
    return fx * xd + cx, fy * yd + cy


def round_fixed(t):
    """rint(t) (half to even) saturated to int32; NaN gives INT32_MIN"""
    with np.errstate(invalid='ignore'):
        r = np.rint(t)
        r = np.where(r >= float(INT32_MIN), np.minimum(r, float(INT32_MAX)), float(INT32_MIN))
    return r.astype(np.int64)


def undistort_taps(K, D, K_new, H, W):
    """sx, sy (first tap), ax, ay (1/32-pixel fractions), int64 (H, W) each"""
    with np.errstate(all='ignore'):
        us, vs = source_position(K, D, K_new, H, W)
        iu, iv = round_fixed(us * 32.0), round_fixed(vs * 32.0)
    return iu >> 5, iv >> 5, iu & 31, iv & 31


def _tap(src, sy, sx):
    H, W = src.shape[:2]
    ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    v = src[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)]
    return np.where(ok[..., None] if src.ndim == 3 else ok, v, 0)


def undistort(src, K, D, K_new, rotate180=False):
    """src uint8 (H, W, 3) or uint16 (H, W).  Border constant 0."""
    src = np.asarray(src)
    H, W = src.shape[:2]
    sx, sy, ax, ay = undistort_taps(K, D, K_new, H, W)
    w = [(32 - ax) * (32 - ay), ax * (32 - ay), (32 - ax) * ay, ax * ay]          # over 1024
    taps = [_tap(src, sy, sx), _tap(src, sy, sx + 1), _tap(src, sy + 1, sx), _tap(src, sy + 1, sx + 1)]
    if src.dtype == np.uint8 and src.ndim == 3:
        acc = np.zeros(src.shape, np.int64)
        for wi, t in zip(w, taps):
            acc += (wi * 32)[..., None] * t.astype(np.int64)
        out = ((acc + 16384) >> 15).astype(np.uint8)
    elif src.dtype == np.uint16 and src.ndim == 2:
        wf = [wi.astype(np.float32) / np.float32(1024) for wi in w]
        tf = [t.astype(np.float32) for t in taps]
        s = wf[0] * tf[0]
        for k in (1, 2, 3):
            s = s + wf[k] * tf[k]
        out = np.clip(np.rint(s), 0, 65535).astype(np.uint16)
    else:
        raise ValueError('undistort: uint8 (H, W, 3) or uint16 (H, W)')
    return np.ascontiguousarray(out[::-1, ::-1]) if rotate180 else out


def undistort_points_normalised(u, v, K, D, iterations=5):
    """pixel -> undistorted normalised coordinates by `iterations` fixed-point steps (float64)"""
    (fx, fy, cx, cy), (k1, k2, p1, p2, k3) = camera(K, D)
    x0, y0 = (np.asarray(u, np.float64) - cx) / fx, (np.asarray(v, np.float64) - cy) / fy
    x, y = x0, y0
    for _ in range(iterations):
        r2 = x * x + y * y
        icd = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (x0 - dx) * icd, (y0 - dy) * icd
    return x, y


def optimal_new_camera_matrix(K, D, size, alpha):
    """size = (w, h).  The 3x3 float64 matrix."""
    w, h = int(size[0]), int(size[1])
    j = np.arange(9, dtype=np.float32)
    gu = (j * np.float32(w) / np.float32(8))[None, :] + np.zeros((9, 1), np.float32)         # point (j w / 8, i h / 8), float32
    gv = (j * np.float32(h) / np.float32(8))[:, None] + np.zeros((1, 9), np.float32)
    x, y = undistort_points_normalised(gu, gv, K, D)
    ox, oy, ow, oh = x.min(), y.min(), x.max() - x.min(), y.max() - y.min()
    ix, iy = x[:, 0].max(), y[0, :].max()
    iw, ih = x[:, 8].min() - ix, y[8, :].min() - iy
    alpha = float(alpha)

    def entries(rx, ry, rw, rh):
        fx, fy = (w - 1) / rw, (h - 1) / rh
        return fx, fy, -fx * rx, -fy * ry
    v0, v1 = entries(ix, iy, iw, ih), entries(ox, oy, ow, oh)
    fx, fy, cx, cy = [a * (1.0 - alpha) + b * alpha for a, b in zip(v0, v1)]
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], np.float64)


# ---------------------------------------------------------------------------------------------------------------------- resize
def _sat16(v):
    return np.clip(v, -32768, 32767).astype(np.int64)


def resize_axis(n_in, n_out):
    """(i, a0, a1) per destination index: first source index and the two 11-bit weights"""
    s = np.float64(n_in) / np.float64(n_out)
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * s - 0.5).astype(np.float32)
    i = np.floor(f).astype(np.int64)
    f = f - i.astype(np.float32)
    lo = i < 0
    i, f = np.where(lo, 0, i), np.where(lo, np.float32(0), f)
    hi = i >= n_in - 1
    i, f = np.where(hi, n_in - 1, i), np.where(hi, np.float32(0), f).astype(np.float32)
    a1 = _sat16(np.rint(f * np.float32(2048)))
    a0 = _sat16(np.rint((np.float32(1) - f) * np.float32(2048)))
    return i, a0, a1


def resize_bgr8(src, size):
    """src uint8 (H, W, 3), size = (oh, ow)"""
    src = np.asarray(src)
    H, W = src.shape[:2]
    oh, ow = int(size[0]), int(size[1])
    xi, xa0, xa1 = resize_axis(W, ow)
    yi, yb0, yb1 = resize_axis(H, oh)
    v = src.astype(np.int64)
    S = v[:, xi] * xa0[None, :, None] + v[:, np.minimum(xi + 1, W - 1)] * xa1[None, :, None]          # (H, ow, 3)
    S0, S1 = S[yi], S[np.minimum(yi + 1, H - 1)]
    r = ((yb0[:, None, None] * (S0 >> 4)) >> 16) + ((yb1[:, None, None] * (S1 >> 4)) >> 16)
    return np.clip((r + 2) >> 2, 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------- thermal rescale
def percentile_ranks(n, q):
    """np.percentile's linear method on n values: (previous rank, next rank, gamma) of quantile q in [0, 1]"""
    vi = (n - 1) * q
    prev = int(np.floor(vi))
    nxt = prev + 1
    if vi >= n - 1:
        prev = nxt = n - 1
    if vi < 0:
        prev = nxt = 0
    return prev, nxt, vi - np.floor(vi)


def lerp(a, b, t):
    """numpy's _lerp on two order statistics (a <= b)"""
    a, b, t = float(a), float(b), float(t)
    diff = b - a
    return b - diff * (1.0 - t) if t >= 0.5 else a + diff * t


def percentile_bounds(x):
    """(np.percentile(x, 1), np.percentile(x, 99)) as float64, from the sorted values"""
    flat = np.sort(np.asarray(x).reshape(-1))
    out = []
    for q in (1 / 100, 99 / 100):
        prev, nxt, g = percentile_ranks(flat.size, q)
        out.append(lerp(flat[prev], flat[nxt], g))
    return out[0], out[1]


def saved_u16(rescaled):
    """(rescaled * 65535).astype('uint16'): truncation toward zero; a value below zero wraps as the x86 conversion does"""
    return ((rescaled * np.float32(65535)).astype(np.int64) & 0xFFFF).astype(np.uint16)


def thermal_rescale(x, outlier_rejection=True):
    """x uint16 (H, W) -> (clipped uint16, rescaled float32, saved uint16).  Without outlier rejection nothing is clipped."""
    x = np.array(x, np.uint16)
    if outlier_rejection:
        lower, upper = percentile_bounds(x)
        x[x < lower] = np.uint16(int(lower))          # the float64 bound assigned into a uint16 array truncates
        x[x > upper] = np.uint16(int(upper))
    smin, smax = float(x.min()), float(x.max())
    scale = 1.0 / (smax - smin) if smax - smin > DBL_EPSILON else 0.0
    shift = -smin * scale
    a, b = np.float32(scale), np.float32(shift)
    rescaled = x.astype(np.float32) * a + b
    return x, rescaled, saved_u16(rescaled)


# -------------------------------------------------------------------------------------------------------------- whole sequence
def prepare_frames(optical, thermal, params, calibration=None):
    """preprocess_images on one pair: optical uint8 (H, W, 3), thermal uint16 (h, w).  Returns (optical, thermal_raw,
    thermal_rescaled); with outlier rejection thermal_raw is the clipped frame (the reference clips through an alias)."""
    optical, thermal = np.asarray(optical), np.asarray(thermal)
    if params['undistort_images']:
        for cam in calibration['cameras']:
            c = cam['camera']
            i = c['intrinsics']['data']
            K = np.array([[i[0], 0, i[2]], [0, i[1], i[3]], [0, 0, 1]], np.float64)
            D = np.array(c['distortion']['parameters']['data'], np.float64)
            if c['label'] == 'optical':
                h, w = optical.shape[:2]
                optical = undistort(optical, K, D, optimal_new_camera_matrix(K, D, (w, h), params['image/undistort_alpha']))
            elif c['label'] == 'thermal':
                h, w = thermal.shape[:2]
                thermal = undistort(thermal, K, D, optimal_new_camera_matrix(K, D, (w, h), params['image/undistort_alpha']))
            else:
                raise ValueError('ERROR unknown camera label: ' + c['label'])
    if params['image/thermal/rotate']:
        thermal = np.ascontiguousarray(thermal[::-1, ::-1])
    if params['image/optical/downscale']:
        ratio = float(thermal.shape[0]) / optical.shape[0]
        optical = resize_bgr8(optical, (int(thermal.shape[0]), int(optical.shape[1] * ratio)))
    raw, rescaled, _ = thermal_rescale(thermal, bool(params['image/thermal/rescale_outlier_rejection']))
    return optical, raw, rescaled


# ---------------------------------------------------------------------------------------------------------------- image makers
def smooth_bgr8(seed, H, W):
    """a smooth analytic colour pattern, uint8 (H, W, 3)"""
    rng = np.random.RandomState(seed)
    ph = rng.uniform(0, 2 * np.pi, (3, 2))
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    ch = [127.5 + 100.0 * np.sin(0.23 * x + ph[c, 0]) * np.cos(0.17 * y + ph[c, 1]) + 20.0 * np.sin(0.05 * (x + y)) for c in range(3)]
    return np.clip(np.rint(np.stack(ch, -1)), 0, 255).astype(np.uint8)


def noise_bgr8(seed, H, W):
    return np.random.RandomState(seed).randint(0, 256, (H, W, 3)).astype(np.uint8)


def noise_u16(seed, H, W):
    return np.random.RandomState(seed).randint(0, 65536, (H, W)).astype(np.uint16)


def thermal_u16(seed, H, W, base=29000, span=1800, outliers=0.02):
    """a smooth 16-bit thermal frame with sensor noise and hot / cold outlier pixels"""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    f = base + span * (0.5 + 0.5 * np.sin(0.19 * x + rng.uniform(0, 6)) * np.cos(0.13 * y + rng.uniform(0, 6)))
    f = f + rng.normal(0, 12, (H, W))
    n = max(int(outliers * H * W), 2)
    idx = rng.choice(H * W, n, replace=False)
    f.reshape(-1)[idx[: n // 2]] = rng.uniform(55000, 65535, n // 2)
    f.reshape(-1)[idx[n // 2:]] = rng.uniform(0, 900, n - n // 2)
    return np.clip(np.rint(f), 0, 65535).astype(np.uint16)


def test_camera(H, W):
    """a plausible K for an H x W frame (square pixels, principal point off the centre)"""
    f = 0.9 * max(W, H)
    return np.array([[f, 0, (W - 1) / 2 + 0.3], [0, f, (H - 1) / 2 - 0.2], [0, 0, 1]], np.float64)


test_camera.__test__ = False                  # (not a pytest test)


def calibration_of(cameras, optical_size, thermal_size):
    """the reference's calibration layout for cameras = [(label, D)], each with test_camera of its frame size (H, W)"""
    out = []
    for label, D in cameras:
        H, W = optical_size if label == 'optical' else thermal_size
        K = test_camera(H, W)
        out.append({'camera': {'label': label, 'intrinsics': {'data': [float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])]},
                               'distortion': {'parameters': {'data': [float(d) for d in D]}}}})
    return {'cameras': out}


DISTORTIONS = [(0.0, 0.0, 0.0, 0.0), (-0.32, 0.11, 1e-3, -5e-4), (0.25, -0.08, -2e-3, 1e-3, 0.02)]


def rescale_cases():
    """{name: uint16 frame}: the frames the thermal rescale is tested on, on the host and on the GPU"""
    ramp = (np.arange(201, dtype=np.uint16) * 7 + 1000)
    np.random.RandomState(4).shuffle(ramp)
    return {
        'fractional_bounds': thermal_u16(5, 24, 32),            # 768 pixels: both bounds lie between two order statistics
        'constant': np.full((7, 9), 1234, np.uint16),           # max = min: scale 0, the output is all 0
        'rank_on_element': ramp.reshape(3, 67),                 # 201 distinct values: 0.01 * 200 and 0.99 * 200 are whole ranks
        'noise_33x47': noise_u16(6, 33, 47),
        'all_65535': np.full((8, 16), 65535, np.uint16),
    }


def golden_case(z, name):
    """one pair of tests/golden/frames.npz: (optical_in, thermal_in, params, calibration, (optical, thermal_raw, thermal_rescaled)).
    The inputs are regenerated from the stored seeds and must equal the stored ones."""
    so, Ho, Wo, st, Ht, Wt = (int(v) for v in z['case_%s_setup' % name])
    optical, thermal = smooth_bgr8(so, Ho, Wo), thermal_u16(st, Ht, Wt)
    assert np.array_equal(optical, z['case_%s_optical_in' % name]) and np.array_equal(thermal, z['case_%s_thermal_in' % name])
    params = {str(k): float(v) for k, v in zip(z['case_%s_param_keys' % name], z['case_%s_params' % name])}
    params = {k: (v if k == 'image/undistort_alpha' else bool(v)) for k, v in params.items()}
    cameras = [(str(label), tuple(z['case_%s_D%d' % (name, k)])) for k, label in enumerate(z['case_%s_labels' % name])]
    want = tuple(z['case_%s_%s' % (name, key)] for key in ('optical', 'thermal_raw', 'thermal_rescaled'))
    return optical, thermal, params, calibration_of(cameras, (Ho, Wo), (Ht, Wt)), want
