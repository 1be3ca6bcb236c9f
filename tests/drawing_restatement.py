"""CPU restatement of the result views (include/multipoint_hip.h mp_draw_*), numpy only: the four rules the
kernels of csrc/draw.hip are held to bit for bit.  The circle's half widths and the LINE_8 pixel walk are the ones the
synthetic shapes are pinned to (shapes_restatement.py).  Canvases are uint8 (B, Hc, Wc, 3) arrays drawn in place."""
import functools

import numpy as np

from shapes_restatement import circle_halfwidths, line_pixels

KINDS = ('ring', 'disc', 'cross')
MODES = ('blend', 'checker', 'anaglyph', 'difference')
MAX_RADIUS = 64


def to_u8(g):
    """NaN -> 0, clamp to [0, 1], one fp32 product with 255, truncated"""
    g = np.asarray(g, np.float32)
    c = np.where(np.isnan(g), np.float32(0), g)
    c = np.minimum(np.maximum(c, np.float32(0)), np.float32(1)).astype(np.float32)
    return (c * np.float32(255.0)).astype(np.uint8)


def gray_values(images, mask=None, gain=1.0):
    """the 8-bit values of fp32 frames: v = x or fl32(x m), g = fl32(v gain)"""
    v = np.asarray(images, np.float32)
    if mask is not None:
        v = (v * np.asarray(mask, np.float32)).astype(np.float32)
    return to_u8((v * np.float32(gain)).astype(np.float32))


def paste(canvas, values, offset=(0, 0)):
    """values (B, H, W) or (B, H, W, 3) into canvas[:, y0:y0 + H, x0:x0 + W], clipped; nothing else is written"""
    B, Hc, Wc = canvas.shape[:3]
    H, W = values.shape[1:3]
    y0, x0 = int(offset[0]), int(offset[1])
    ys, xs = max(0, -y0), max(0, -x0)
    ye, xe = min(H, Hc - y0), min(W, Wc - x0)
    if ys >= ye or xs >= xe:
        return canvas
    part = values[:, ys:ye, xs:xe]
    canvas[:, y0 + ys:y0 + ye, x0 + xs:x0 + xe] = part if part.ndim == 4 else part[..., None]
    return canvas


def gray_to_rgb(canvas, images, mask=None, gain=1.0, offset=(0, 0)):
    return paste(canvas, gray_values(images, mask, gain), offset)


@functools.lru_cache(maxsize=None)
def _disc_offsets(r):
    half = circle_halfwidths(r)
    return frozenset((dx, s * k) for k in range(r + 1) for s in (-1, 1) for dx in range(-half[k], half[k] + 1))


def disc(center, r):
    """{(x, y)}: |y - cy| <= r and |x - cx| <= half_r[|y - cy|]; empty for a negative radius"""
    if r < 0:
        return set()
    cx, cy = int(center[0]), int(center[1])
    return {(cx + dx, cy + dy) for dx, dy in _disc_offsets(int(r))}


def ring(center, r, t):
    return disc(center, r + t // 2) - disc(center, r - (t + 1) // 2)


def cross(center, r):
    cx, cy = int(center[0]), int(center[1])
    return {(cx + d, cy) for d in range(-r, r + 1)} | {(cx, cy + d) for d in range(-r, r + 1)}


def mark(center, r, t, kind):
    return ring(center, r, t) if kind == 'ring' else disc(center, r) if kind == 'disc' else cross(center, r)


def _paint(image, pixels, color):
    Hc, Wc = image.shape[:2]
    for x, y in pixels:
        if 0 <= x < Wc and 0 <= y < Hc:
            image[y, x] = color


def draw_marks(canvas, kp_yx, counts, r, t, kind, palette, offset=(0, 0)):
    """Marks in ascending index, so the highest index covering a pixel stays"""
    palette = np.asarray(palette, np.uint8).reshape(-1, 3)
    kp_yx = np.asarray(kp_yx).astype(np.int64)
    B, K = kp_yx.shape[:2]
    for b in range(B):
        for i in range(min(max(int(counts[b]), 0), K)):
            c = (int(kp_yx[b, i, 1]) + int(offset[1]), int(kp_yx[b, i, 0]) + int(offset[0]))
            _paint(canvas[b], mark(c, r, t, kind), palette[i % len(palette)])
    return canvas


def match_primitives(kp_a, kp_b, count_a, count_b, match_idx, mask=None):
    """the q that exist for one pair, with their train index"""
    K = len(match_idx)
    na, nb = min(max(int(count_a), 0), K), min(max(int(count_b), 0), K)
    return [(q, int(match_idx[q])) for q in range(na)
            if 0 <= int(match_idx[q]) < nb and (mask is None or mask[q] != 0)]


def draw_matches(canvas, kp_a, kp_b, count_a, count_b, match_idx, mask, offset_a, offset_b, r, t, palette):
    palette = np.asarray(palette, np.uint8).reshape(-1, 3)
    kp_a, kp_b = np.asarray(kp_a).astype(np.int64), np.asarray(kp_b).astype(np.int64)
    P, Hc, Wc = canvas.shape[:3]
    for p in range(P):
        for q, m in match_primitives(kp_a[p], kp_b[p], count_a[p], count_b[p], match_idx[p], None if mask is None else mask[p]):
            A = (int(kp_a[p, q, 1]) + int(offset_a[1]), int(kp_a[p, q, 0]) + int(offset_a[0]))
            B = (int(kp_b[p, m, 1]) + int(offset_b[1]), int(kp_b[p, m, 0]) + int(offset_b[0]))
            pixels = ring(A, r, t) | ring(B, r, t) | set(line_pixels(Wc, Hc, A, B))
            _paint(canvas[p], pixels, palette[q % len(palette)])
    return canvas


def match_picture(optical, thermal, kp_a, kp_b, count_a, count_b, match_idx, mask, r, t, palette):
    """utils.drawing.draw_matches: optical | thermal, the thermal side offset by W"""
    P, H, W = optical.shape
    canvas = np.zeros((P, H, 2 * W, 3), np.uint8)
    gray_to_rgb(canvas, optical)
    gray_to_rgb(canvas, thermal, offset=(0, W))
    return draw_matches(canvas, kp_a, kp_b, count_a, count_b, match_idx, mask, (0, 0), (0, W), r, t, palette)


def compose(a, t, mode, alpha=128, cell=32):
    """(B, H, W, 3) uint8 from the warped optical frames a (a < 0: outside) and the thermal frames t"""
    a, t = np.asarray(a, np.float32), np.asarray(t, np.float32)
    outside = a < 0
    A = np.where(outside, 0, to_u8(a)).astype(np.int64)
    T = to_u8(t).astype(np.int64)
    if mode == 'anaglyph':
        return np.stack([A, T, T], -1).astype(np.uint8)
    if mode == 'blend':
        v = (A * alpha + T * (256 - alpha) + 128) >> 8
    elif mode == 'checker':
        y, x = np.mgrid[0:a.shape[1], 0:a.shape[2]]
        v = np.where((x // cell + y // cell) % 2 == 0, A, T)
    elif mode == 'difference':
        v = np.abs(A - T)
    else:
        raise ValueError(mode)
    v = np.where(outside, T, v)
    return np.repeat(v[..., None], 3, -1).astype(np.uint8)
