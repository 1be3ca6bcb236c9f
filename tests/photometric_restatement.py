"""CPU restatement of the OpenCV 4.2 calls behind the reference's photometric augmentation
(multipoint/datasets/augmentation/photometric_augmentation.py), written from OpenCV's published algorithm:

    cv2.ellipse(mask, (x, y), (ax, ay), angle, 0, 360, 1.0, -1)   EllipseEx -> ellipse2Poly -> FillConvexPoly (LINE_8)
    cv2.GaussianBlur(mask, (k, k), 0)                              getGaussianKernel + sepFilter2D, BORDER_REFLECT_101
    cv2.filter2D(image, -1, kernel)                                the non-zero taps in row-major order, BORDER_REFLECT_101

and numpy's float32 pairwise sum (what `image.mean()` computes).  OpenCV is not installed here, so parity of these
restatements with a real OpenCV build is not pinned; the HIP kernels are pinned against them.
Pixel sums are float32 with every operation rounded separately (no fused multiply-add)."""
import math

import numpy as np

XY_SHIFT = 16
XY_ONE = 1 << XY_SHIFT
F32 = np.float32
MEAN_CHUNK = 8192          # numpy's default iterator buffer size (np.getbufsize())


def sin_table(d):
    """OpenCV's SinTable[d] (drawing.cpp): sin of d degrees with 7 decimals, as float32, for 0 <= d <= 450."""
    return F32(np.rint(math.sin(d * (math.pi / 180.0)) * 1e7) / 1e7)


def cv_round(v):
    """cvRound: nearest integer, ties to even."""
    return int(round(v))


def _cdiv(a, b):
    """C integer division (truncates toward zero)."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def ellipse_vertices(x, y, ax, ay, angle):
    """EllipseEx + ellipse2Poly for a full filled ellipse: the 16.16 fixed-point polygon.  `angle` is the double the
    caller passes (rounded to integer degrees here, as cv::ellipse does)."""
    angle = cv_round(angle)
    cx, cy = float(x << XY_SHIFT), float(y << XY_SHIFT)
    aw, ah = abs(ax) << XY_SHIFT, abs(ay) << XY_SHIFT
    delta = (max(aw, ah) + (XY_ONE >> 1)) >> XY_SHIFT
    delta = 90 if delta < 3 else 30 if delta < 10 else 18 if delta < 15 else 5
    while angle < 0:
        angle += 360
    while angle > 360:
        angle -= 360
    alpha, beta = float(sin_table(450 - angle)), float(sin_table(angle))     # cos, sin
    pts = []
    for i in range(0, 360 + delta, delta):
        a = min(i, 360)
        px = float(aw) * float(sin_table(450 - a))
        py = float(ah) * float(sin_table(a))
        pts.append((cx + px * alpha - py * beta, cy + px * beta + py * alpha))
    if len(pts) == 1:
        pts = [(cx, cy), (cx, cy)]
    v = []
    for fx, fy in pts:
        qx, qy = cv_round(fx / XY_ONE) << XY_SHIFT, cv_round(fy / XY_ONE) << XY_SHIFT
        qx += cv_round(fx - qx)
        qy += cv_round(fy - qy)
        if not v or v[-1] != (qx, qy):
            v.append((qx, qy))
    if len(v) == 1:
        v = [(x << XY_SHIFT, y << XY_SHIFT)] * 2
    return v


def _clip_line(W, H, p1, p2):
    right, bottom = (W << XY_SHIFT) - 1, (H << XY_SHIFT) - 1
    x1, y1 = p1
    x2, y2 = p2
    c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8
    c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * (x2 - x1) / (y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * (x2 - x1) / (y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * (y2 - y1) / (x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * (y2 - y1) / (x2 - x1))
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, (x1, y1), (x2, y2)


def _line2(img, p1, p2):
    """Line2: the LINE_8 segment between two 16.16 points."""
    H, W = img.shape
    ok, (x1, y1), (x2, y2) = _clip_line(W, H, p1, p2)
    if not ok:
        return
    dx, dy = x2 - x1, y2 - y1
    j = -1 if dx < 0 else 0
    ax = (dx ^ j) - j
    i = -1 if dy < 0 else 0
    ay = (dy ^ i) - i
    if ax > ay:
        if j:
            x1, x2, y1, y2 = x2, x1, y2, y1
        y_step = _cdiv(((dy ^ j) - j) * XY_ONE, ax | 1)
        ecount = (x2 - x1) >> XY_SHIFT
    else:
        if i:
            x1, x2, y1, y2 = x2, x1, y2, y1
        x_step = _cdiv(((dx ^ i) - i) * XY_ONE, ay | 1)
        ecount = (y2 - y1) >> XY_SHIFT
    x1 += XY_ONE >> 1
    y1 += XY_ONE >> 1

    def put(px, py):
        if 0 <= px < W and 0 <= py < H:
            img[py, px] = 1.0
    put((x2 + (XY_ONE >> 1)) >> XY_SHIFT, (y2 + (XY_ONE >> 1)) >> XY_SHIFT)
    if ax > ay:
        x1 >>= XY_SHIFT
        while ecount >= 0:
            put(x1, y1 >> XY_SHIFT)
            x1 += 1
            y1 += y_step
            ecount -= 1
    else:
        y1 >>= XY_SHIFT
        while ecount >= 0:
            put(x1 >> XY_SHIFT, y1)
            x1 += x_step
            y1 += 1
            ecount -= 1


def fill_convex_poly(img, v):
    """FillConvexPoly(img, v, npts, color, LINE_8, XY_SHIFT): the outline, then the scanline spans."""
    H, W = img.shape
    npts = len(v)
    delta = XY_ONE >> 1
    xmin = xmax = v[0][0]
    ymin = ymax = v[0][1]
    imin = 0
    p0 = v[-1]
    for i, p in enumerate(v):
        if p[1] < ymin:
            ymin, imin = p[1], i
        ymax, xmax, xmin = max(ymax, p[1]), max(xmax, p[0]), min(xmin, p[0])
        _line2(img, p0, p)
        p0 = p
    xmin, xmax = (xmin + delta) >> XY_SHIFT, (xmax + delta) >> XY_SHIFT
    ymin, ymax = (ymin + delta) >> XY_SHIFT, (ymax + delta) >> XY_SHIFT
    if npts < 3 or xmax < 0 or ymax < 0 or xmin >= W or ymin >= H:
        return img
    ymax = min(ymax, H - 1)
    edge = [dict(idx=imin, di=1, x=-XY_ONE, dx=0, ye=ymin), dict(idx=imin, di=npts - 1, x=-XY_ONE, dx=0, ye=ymin)]
    y = ymin
    edges = npts
    while True:
        for e in edge:
            if y >= e['ye']:
                idx0, di = e['idx'], e['di']
                idx = idx0 + di
                if idx >= npts:
                    idx -= npts
                while edges > 0:
                    edges -= 1
                    ty = (v[idx][1] + delta) >> XY_SHIFT
                    if ty > y:
                        xs, xe = v[idx0][0], v[idx][0]
                        e['ye'] = ty
                        e['dx'] = _cdiv((xe - xs) * 2 + (ty - y), 2 * (ty - y))
                        e['x'] = xs
                        e['idx'] = idx
                        break
                    idx0 = idx
                    idx += di
                    if idx >= npts:
                        idx -= npts
                else:
                    edges -= 1          # the C loop `for (; edges-- > 0; )` decrements once more when it ends
        if edges < 0:
            break
        if y >= 0:
            left, right = (1, 0) if edge[0]['x'] > edge[1]['x'] else (0, 1)
            xx1 = (edge[left]['x'] + delta) >> XY_SHIFT
            xx2 = (edge[right]['x'] + delta) >> XY_SHIFT
            if xx2 >= 0 and xx1 < W:
                img[y, max(xx1, 0):min(xx2, W - 1) + 1] = 1.0
        edge[0]['x'] += edge[0]['dx']
        edge[1]['x'] += edge[1]['dx']
        y += 1
        if y > ymax:
            break
    return img


def cv_ellipse_fill(mask, center, axes, angle):
    """cv2.ellipse(mask, center, axes, angle, 0, 360, 1.0, -1) on a float32 mask, in place."""
    return fill_convex_poly(mask, ellipse_vertices(int(center[0]), int(center[1]), int(axes[0]), int(axes[1]), angle))


def border_interpolate(p, n):
    """borderInterpolate(p, n, BORDER_REFLECT_101), repeating the reflection while p stays outside."""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def gaussian_kernel(k):
    """getGaussianKernel(k, 0, CV_32F): computed in double, stored as float."""
    sigma = ((k - 1) * 0.5 - 1) * 0.3 + 0.8
    scale2x = -0.5 / (sigma * sigma)
    cf = np.empty(k, np.float32)
    s = 0.0
    for i in range(k):
        x = i - (k - 1) * 0.5
        cf[i] = F32(math.exp(scale2x * x * x))
        s += float(cf[i])
    s = 1.0 / s
    for i in range(k):
        cf[i] = F32(float(cf[i]) * s)
    return cf


def _reflect_index(n, r):
    return np.array([border_interpolate(p, n) for p in range(-r, n + r)], np.int64)


def gaussian_blur(mask, k):
    """cv2.GaussianBlur(mask, (k, k), 0) for a float32 (H,W) mask: the row filter (taps summed left to right), then the
    symmetric column filter (centre tap, then ky[r+j] * (S[+j] + S[-j]) for j = 1..r), float32."""
    mask = np.asarray(mask, np.float32)
    H, W = mask.shape
    w = gaussian_kernel(k)
    r = k // 2
    cols = _reflect_index(W, r)
    rows = _reflect_index(H, r)
    t = w[0] * mask[:, cols[0:W]]
    for j in range(1, k):
        t = t + w[j] * mask[:, cols[j:j + W]]
    t = t.astype(np.float32)
    out = w[r] * t[rows[r:r + H], :]
    for j in range(1, r + 1):
        out = out + w[r + j] * (t[rows[r + j:r + j + H], :] + t[rows[r - j:r - j + H], :])
    return out.astype(np.float32)


def motion_taps(mode, ksize):
    """The reference's motion_blur kernel (photometric_augmentation.py:61-77) as float32 non-zero taps in row-major order:
    a list of (dy, dx, weight) relative to the anchor (centre)."""
    center = int((ksize - 1) / 2)
    kernel = np.zeros((ksize, ksize))
    if mode == 'h':
        kernel[center, :] = 1.
    elif mode == 'v':
        kernel[:, center] = 1.
    elif mode == 'diag_down':
        kernel = np.eye(ksize)
    elif mode == 'diag_up':
        kernel = np.flip(np.eye(ksize), 0)
    var = ksize * ksize / 16.0
    grid = np.repeat(np.arange(ksize)[:, np.newaxis], ksize, axis=-1)
    gaussian = np.exp(-(np.square(grid - center) + np.square(grid.T - center)) / (2.0 * var))
    kernel *= gaussian
    kernel /= np.sum(kernel)
    k32 = kernel.astype(np.float32)
    return [(i - center, j - center, k32[i, j]) for i in range(ksize) for j in range(ksize) if k32[i, j] != 0]


def filter2d(image, taps):
    """cv2.filter2D(image, -1, kernel) for float32: s = 0; s += w * src over the non-zero taps, BORDER_REFLECT_101."""
    image = np.asarray(image, np.float32)
    H, W = image.shape
    r = max([max(abs(dy), abs(dx)) for dy, dx, _ in taps] + [0])
    rows, cols = _reflect_index(H, r), _reflect_index(W, r)
    s = np.zeros((H, W), np.float32)
    for dy, dx, w in taps:
        s = (s + F32(w) * image[rows[r + dy:r + dy + H]][:, cols[r + dx:r + dx + W]]).astype(np.float32)
    return s


def pairwise_sum(a):
    """numpy's float32 pairwise_sum of a 1-D array: 8 accumulators in leaves of at most 128 elements, splits at
    n/2 - (n/2) % 8."""
    a = np.asarray(a, np.float32)
    n = a.shape[0]
    if n < 8:
        res = F32(0.0)
        for v in a:
            res = F32(res + v)
        return res
    if n <= 128:
        r = a[:8].copy()
        i = 8
        while i < n - n % 8:
            r = (r + a[i:i + 8]).astype(np.float32)
            i += 8
        res = F32(F32(F32(r[0] + r[1]) + F32(r[2] + r[3])) + F32(F32(r[4] + r[5]) + F32(r[6] + r[7])))
        while i < n:
            res = F32(res + a[i])
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return F32(pairwise_sum(a[:n2]) + pairwise_sum(a[n2:]))


def image_mean(image):
    """image.mean() of a float32 image as numpy computes it: its reduction runs through the iterator's buffer of 8192
    elements, so the pixels in C order are summed in chunks of 8192, each chunk a pairwise sum accumulated onto the running
    float32 total; divided by the pixel count in float32.  A strided crop is copied into the same buffer, so a view and a
    contiguous copy of the same pixels give the same bits."""
    a = np.ascontiguousarray(image, np.float32).reshape(-1)
    s = F32(0.0)
    for i in range(0, a.size, MEAN_CHUNK):
        s = F32(s + pairwise_sum(a[i:i + MEAN_CHUNK]))
    return F32(s / F32(a.size))


def apply_plan(image, plan):
    """The chain of a multipoint_amd PhotometricPlan ('host' noise) on the CPU, in the kernels' float32 operation order:
    what mp_photometric_augment computes for one image."""
    x = np.array(image, np.float32)
    H, W = x.shape
    for op in plan.ops:
        name = op['name']
        if name in ('additive_gaussian_noise', 'gaussian_add'):
            x = (x.astype(np.float64) + op['normal']).astype(np.float32)
            if name == 'additive_gaussian_noise':
                x = np.clip(x, 0.0, 1.0)
        elif name == 'additive_speckle_noise':
            x[op['uniform'] < op['value']] = 0.0
            x[op['uniform'] > 1.0 - op['value']] = 1.0
        elif name == 'random_brightness':
            x = np.clip(x + F32(op['value']), 0.0, 1.0)
        elif name == 'random_contrast':
            m = image_mean(x)
            x = np.clip((x - m) * F32(op['value']) + m, 0.0, 1.0)
        elif name == 'additive_shade':
            mask = np.zeros((H, W), np.float32)
            for ex, ey, ax, ay, angle in op['ellipses']:
                cv_ellipse_fill(mask, (ex, ey), (ax, ay), angle)
            mask = gaussian_blur(mask, op['ksize'])
            x = np.clip(x * (F32(1) - F32(op['value']) * mask), 0.0, 1.0)
        elif name == 'motion_blur':
            c = (op['ksize'] - 1) // 2
            offs = [(0, t - c) if op['mode'] == 0 else (t - c, 0) if op['mode'] == 1 else
                    (t - c, t - c) if op['mode'] == 2 else (t - c, c - t) for t in range(op['ksize'])]
            x = filter2d(x, [(dy, dx, F32(w)) for (dy, dx), w in zip(offs, op['taps'])])
        x = x.astype(np.float32)
    return x
