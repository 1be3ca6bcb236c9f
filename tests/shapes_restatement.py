"""CPU restatement of the OpenCV 4.2 calls behind the reference's synthetic shapes (multipoint/utils/draw_primitives.py,
multipoint/datasets/SyntheticShapes.py), written from OpenCV's published algorithm:

    cv2.circle(img, c, r, col, -1)            Circle(): the midpoint walk, one or two row spans per step
    cv2.line(img, p1, p2, col, t)             ThickLine(): t <= 1 the 8-connected LineIterator, otherwise the 4-vertex
                                              16.16 rectangle through FillConvexPoly plus the two filled end circles
    cv2.fillPoly(img, [pts], col)             CollectPolyEdges (outline with Line) + FillEdgeCollection (even-odd)
    cv2.fillConvexPoly(img, pts, col)         FillConvexPoly at shift 0
    cv2.ellipse(..., col, -1)                 ellipse2Poly + FillConvexPoly (photometric_restatement.py)
    cv2.blur(img, (k, k))                     normalised box filter, anchor k // 2, BORDER_REFLECT_101
    cv2.threshold(img, t, 1.0, THRESH_BINARY) src > t ? 1 : 0
    cv2.randu(img, 0, 1)                      any seeded uniform field
    cv2.getAffineTransform(src, dst)          the 6 x 6 system solved in double
    cv2.resize(img, (w, h), INTER_LINEAR)     sx = (dx + 0.5) * scale - 0.5, float weight pair, indices clamped
    cv2.GaussianBlur(img, (k, k), 0)          on float64: double weights, sepFilter2D, BORDER_REFLECT_101

OpenCV is not installed here, so parity of these restatements with a real OpenCV build is not pinned;
the HIP kernels of shapes.hip are pinned against them.  Images are float64 (H, W) arrays drawn in place, as the reference
holds them."""
import math

import numpy as np

import photometric_restatement as P

XY_SHIFT, XY_ONE = P.XY_SHIFT, P.XY_ONE


def _paint(img, mask, color):
    img[mask != 0] = color


def circle_halfwidths(radius):
    """Circle(): for each row offset k in [0, radius] the half width of the widest span the midpoint walk draws on rows
    cy - k and cy + k (-1: the walk never touches that row, which does not happen for k <= radius)."""
    half = [-1] * (radius + 1)
    err, dx, dy, plus, minus = 0, radius, 0, 1, (radius << 1) - 1
    while dx >= dy:
        half[dy] = max(half[dy], dx)
        half[dx] = max(half[dx], dy)
        dy += 1
        err += plus
        plus += 2
        mask = -1 if err > 0 else 0
        err -= minus & mask
        dx += mask
        minus -= mask & 2
    return half


def circle(img, center, radius, color):
    """cv2.circle(img, center, radius, color, -1): rows clipped to the frame, spans clipped to [0, W - 1]."""
    H, W = img.shape
    cx, cy = int(center[0]), int(center[1])
    half = circle_halfwidths(int(radius))
    for k, hw in enumerate(half):
        if hw < 0:
            continue
        x1, x2 = max(cx - hw, 0), min(cx + hw, W - 1)
        if x1 > x2:
            continue
        for y in (cy - k, cy + k):
            if 0 <= y < H:
                img[y, x1:x2 + 1] = color
    return img


def _clip_line_int(W, H, p1, p2):
    """clipLine(Size(W, H), pt1, pt2) in pixel coordinates: the algorithm of the 16.16 one with right = W - 1."""
    right, bottom = W - 1, H - 1
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


def line_pixels(W, H, p1, p2):
    """Line(): the pixels of LineIterator(img, p1, p2, 8) in order (empty when the segment misses the frame)."""
    x1, y1 = int(p1[0]), int(p1[1])
    x2, y2 = int(p2[0]), int(p2[1])
    if not (0 <= x1 < W and 0 <= x2 < W and 0 <= y1 < H and 0 <= y2 < H):
        ok, (x1, y1), (x2, y2) = _clip_line_int(W, H, (x1, y1), (x2, y2))
        if not ok:
            return []
    if x2 < x1:                                    # Line() iterates left to right
        x1, y1, x2, y2 = x2, y2, x1, y1
    dx, dy = x2 - x1, y2 - y1
    sx = 1
    sy = -1 if dy < 0 else 1
    dx, dy = abs(dx), abs(dy)
    steep = dy > dx
    if steep:
        dx, dy = dy, dx
    err, plus_delta, minus_delta = dx - (dy + dy), dx + dx, -(dy + dy)
    out = []
    x, y = x1, y1
    for _ in range(dx + 1):
        out.append((x, y))
        minor = err < 0
        err += minus_delta + (plus_delta if minor else 0)
        if steep:
            y += sy
            x += sx if minor else 0
        else:
            x += sx
            y += sy if minor else 0
    return out


def _thin_line(img, p1, p2, color):
    H, W = img.shape
    for x, y in line_pixels(W, H, p1, p2):
        img[y, x] = color


def fill_convex(img, verts_fixed, color):
    """FillConvexPoly on 16.16 vertices with a colour (photometric_restatement.fill_convex_poly paints a mask)."""
    mask = np.zeros(img.shape, np.float32)
    P.fill_convex_poly(mask, [(int(x), int(y)) for x, y in verts_fixed])
    _paint(img, mask, color)
    return img


def thick_line_rect(p1, p2, thickness):
    """ThickLine's rectangle for thickness > 1: the four 16.16 vertices (None for a zero-length segment) and the radius of
    the end circles."""
    x0, y0 = int(p1[0]) << XY_SHIFT, int(p1[1]) << XY_SHIFT
    x1, y1 = int(p2[0]) << XY_SHIFT, int(p2[1]) << XY_SHIFT
    inv = 1.0 / XY_ONE
    dx, dy = (x0 - x1) * inv, (y1 - y0) * inv
    r = dx * dx + dy * dy
    odd = thickness & 1
    t = thickness << (XY_SHIFT - 1)
    rect = None
    if abs(r) > 2.220446049250313e-16:
        r = (t + odd * XY_ONE * 0.5) / math.sqrt(r)
        dpx, dpy = P.cv_round(dy * r), P.cv_round(dx * r)
        rect = [(x0 + dpx, y0 + dpy), (x0 - dpx, y0 - dpy), (x1 - dpx, y1 - dpy), (x1 + dpx, y1 + dpy)]
    return rect, (t + (XY_ONE >> 1)) >> XY_SHIFT


def line(img, p1, p2, color, thickness=1):
    """cv2.line(img, p1, p2, color, thickness), LINE_8, shift 0."""
    thickness = int(thickness)
    if thickness <= 1:
        _thin_line(img, p1, p2, color)
        return img
    rect, rad = thick_line_rect(p1, p2, thickness)
    if rect is not None:
        fill_convex(img, rect, color)
    circle(img, p1, rad, color)
    circle(img, p2, rad, color)
    return img


def fill_convex_poly(img, pts, color):
    """cv2.fillConvexPoly(img, pts, color) for integer points: at shift 0 FillConvexPoly draws its outline with Line() (the
    LineIterator), not Line2, and then walks the same spans."""
    pts = np.asarray(pts).reshape(-1, 2)
    for j in range(len(pts)):
        _thin_line(img, pts[j - 1], pts[j], color)
    mask = np.zeros(img.shape, np.float32)
    line2, P._line2 = P._line2, lambda *a: None               # the spans alone
    try:
        P.fill_convex_poly(mask, [(int(x) << XY_SHIFT, int(y) << XY_SHIFT) for x, y in pts])
    finally:
        P._line2 = line2
    _paint(img, mask, color)
    return img


def poly_edges(pts):
    """CollectPolyEdges at shift 0 without the outline: (y0, y1, x, dx) per non-horizontal edge, x and dx in 16.16."""
    pts = [(int(x), int(y)) for x, y in np.asarray(pts).reshape(-1, 2)]
    edges = []
    p0 = pts[-1]
    for p1 in pts:
        (x0, y0), (x1, y1) = p0, p1
        p0 = p1
        if y0 == y1:
            continue
        fx0, fx1 = x0 << XY_SHIFT, x1 << XY_SHIFT
        dx = P._cdiv(fx1 - fx0, y1 - y0)
        edges.append([y0, y1, fx0, dx] if y0 < y1 else [y1, y0, fx1, dx])
    return edges


def fill_edge_collection(img, edges, color):
    """FillEdgeCollection: the active edge list kept sorted by x, spans between the pairs (even-odd), from the ceiling of
    the left x to the floor of the right x."""
    H, W = img.shape
    total = len(edges)
    if total < 2:
        return img
    ends = [e[2] + (e[1] - e[0]) * e[3] for e in edges]
    y_min, y_max = min(e[0] for e in edges), max(e[1] for e in edges)
    x_min = min(min(e[2] for e in edges), min(ends))
    x_max = max(max(e[2] for e in edges), max(ends))
    if y_max < 0 or y_min >= H or x_max < 0 or x_min >= (W << XY_SHIFT):
        return img
    pending = sorted(([e[0], e[1], e[2], e[3]] for e in edges), key=lambda e: (e[0], e[2], e[3]))
    i = 0
    active = []
    y_max = min(y_max, H)
    for y in range(pending[0][0], y_max):
        row = []
        k = 0
        active = [e for e in active if e[1] != y]
        while k < len(active) or (i < total and pending[i][0] == y):
            new = i < total and pending[i][0] == y
            if k < len(active) and (not new or active[k][2] < pending[i][2]):
                row.append(active[k])
                k += 1
            else:
                row.append(pending[i])
                i += 1
            if len(row) % 2 == 0:
                a, b = row[-2], row[-1]
                if y >= 0:
                    if a[2] > b[2]:
                        x1, x2 = (b[2] + XY_ONE - 1) >> XY_SHIFT, a[2] >> XY_SHIFT
                    else:
                        x1, x2 = (a[2] + XY_ONE - 1) >> XY_SHIFT, b[2] >> XY_SHIFT
                    if x1 < W and x2 >= 0:
                        x1, x2 = max(x1, 0), min(x2, W - 1)
                        if x1 <= x2:
                            img[y, x1:x2 + 1] = color
                a[2] += a[3]
                b[2] += b[3]
        active = sorted(row, key=lambda e: e[2])             # the bubble sort is a stable sort by x
    return img


def fill_poly(img, pts, color):
    """cv2.fillPoly(img, [pts], color) for one contour of integer points."""
    pts = np.asarray(pts).reshape(-1, 2)
    n = len(pts)
    for j in range(n):
        _thin_line(img, pts[j - 1], pts[j], color)
    return fill_edge_collection(img, poly_edges(pts), color)


def ellipse(img, center, axes, angle, color):
    """cv2.ellipse(img, center, axes, angle, 0, 360, color, -1)."""
    v = P.ellipse_vertices(int(center[0]), int(center[1]), int(axes[0]), int(axes[1]), angle)
    return fill_convex(img, v, color)


def _reflect_index(n, before, after):
    return np.array([P.border_interpolate(p, n) for p in range(-before, n + after)], np.int64)


def blur(img, k):
    """cv2.blur(img, (k, k)) on float64: the k x k mean around the anchor k // 2, BORDER_REFLECT_101 (repeated while the
    index stays outside), sums in double."""
    img = np.asarray(img, np.float64)
    H, W = img.shape
    a = k // 2
    cols = _reflect_index(W, a, k - 1 - a)
    rows = _reflect_index(H, a, k - 1 - a)
    c = np.concatenate([np.zeros((H, 1)), np.cumsum(img[:, cols], axis=1)], axis=1)
    t = c[:, k:k + W] - c[:, 0:W]
    c = np.concatenate([np.zeros((1, W)), np.cumsum(t[rows, :], axis=0)], axis=0)
    return (c[k:k + H, :] - c[0:H, :]) * (1.0 / (k * k))


def threshold(img, t):
    """cv2.threshold(img, t, 1.0, THRESH_BINARY)."""
    return np.where(np.asarray(img) > t, 1.0, 0.0)


def randu(shape, seed):
    """cv2.randu(img, 0, 1): OpenCV's own generator is never seeded by the reference; any uniform field is faithful."""
    return np.random.default_rng(seed).random(shape)


def get_affine_transform(src, dst):
    """cv2.getAffineTransform: the 6 x 6 linear system in double."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    a = np.zeros((6, 6))
    b = np.zeros(6)
    for i in range(3):
        a[i, 0:3] = [src[i, 0], src[i, 1], 1.0]
        a[i + 3, 3:6] = [src[i, 0], src[i, 1], 1.0]
        b[i], b[i + 3] = dst[i, 0], dst[i, 1]
    return np.linalg.solve(a, b).reshape(2, 3)


def resize_coeffs(dst, src):
    """The INTER_LINEAR tap of each destination index: (left index clamped, right index clamped, float32 weight pair)."""
    scale = 1.0 / (dst / src)                      # resize.cpp: scale = 1 / inv_scale
    i0 = np.empty(dst, np.int64)
    i1 = np.empty(dst, np.int64)
    w = np.empty(dst, np.float32)
    for d in range(dst):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(math.floor(f))
        f = np.float32(f - np.float32(s))
        if s < 0:
            s, f = 0, np.float32(0)
        if s >= src - 1:
            s, f = src - 1, np.float32(0)
        i0[d], i1[d], w[d] = s, min(s + 1, src - 1), f
    return i0, i1, w


def resize(img, dsize):
    """cv2.resize(img, (w, h), interpolation=INTER_LINEAR) on a float image: float weights, horizontal then vertical."""
    img = np.asarray(img)
    H, W = img.shape
    w_out, h_out = int(dsize[0]), int(dsize[1])
    x0, x1, fx = resize_coeffs(w_out, W)
    y0, y1, fy = resize_coeffs(h_out, H)
    fx, fy = fx.astype(img.dtype), fy.astype(img.dtype)
    rows = img[:, x0] * (1 - fx) + img[:, x1] * fx
    return rows[y0, :] * (1 - fy)[:, None] + rows[y1, :] * fy[:, None]


def gaussian_kernel64(k):
    """getGaussianKernel(k, 0, CV_64F)."""
    sigma = ((k - 1) * 0.5 - 1) * 0.3 + 0.8
    x = np.arange(k) - (k - 1) * 0.5
    w = np.exp(-0.5 / (sigma * sigma) * x * x)
    return w / w.sum()


def gaussian_blur64(img, k):
    """cv2.GaussianBlur(img, (k, k), 0) on a float64 image."""
    img = np.asarray(img, np.float64)
    H, W = img.shape
    w = gaussian_kernel64(k)
    r = k // 2
    cols, rows = _reflect_index(W, r, r), _reflect_index(H, r, r)
    t = sum(w[j] * img[:, cols[j:j + W]] for j in range(k))
    return sum(w[j] * t[rows[j:j + H], :] for j in range(k))
