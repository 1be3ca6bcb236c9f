"""Results as pictures: what the reference shows in cv2 / matplotlib windows (show_keypoints.py, show_image_pair_sample.py, the
-p halves of predict_keypoints.py and predict_align_image_pair.py, create_dataset/check_alignment.py) drawn on the GPU, where
the images, keypoint lists and matches already are, into uint8 RGB canvases that are written as PNG / GIF files (the GPU
machines have no display).  The drawing rules are DESIGN.md 3.14 and include/multipoint_hip.h (csrc/draw.hip):

    gray_to_rgb(images, valid_mask=None, gain=1.0, out=None, offset=(0, 0))      fp32 frames -> (B, H, W, 3) uint8
    draw_keypoints(canvas, kp_yx, kp_count=None, radius=4, color=(0, 255, 0), thickness=1, kind='ring', ...)    in place
    draw_matches(optical, thermal, kp_optical, kp_thermal, match_idx, ...)       -> (P, H, 2 W, 3), optical | thermal
    draw_pair_results(res, images, mask=None, ...)                                the same from a PairResults, all on the device
    compose(a, t, mode, alpha=128, cell=32) / alignment_views(optical, thermal, transform, modes, ...)
    draw_segments(canvas, segments, ...) / draw_residual_field(canvas, field, frame, scale=4, ...)   needle maps
    match_palette(n=64), save_png(path, rgb), save_gif(path, frames, dt_ms)

Marks are 8-connected (OpenCV's Circle() and LineIterator), one colour per mark, the highest index on top; the reference's
drawKeypoints / drawMatches are anti-aliased with random colours, so pictures agree in positions, radii and layer order, not
pixel by pixel.  There is no CPU path: without a GPU every entry raises."""
import colorsys

import numpy as np
import torch

from .. import _lib
from . import alignment

__all__ = ['gray_to_rgb', 'draw_keypoints', 'draw_matches', 'draw_pair_results', 'match_palette', 'alignment_views', 'compose',
           'save_png', 'save_gif', 'draw_segments', 'draw_residual_field']

_palettes = {}


def match_palette(n=64):
    """(n, 3) uint8: entry i is round(255 * colorsys.hsv_to_rgb((i * 0.618033988749895) % 1.0, 1.0, 1.0)) -- hues a golden-ratio
    step apart, so neighbouring indices differ clearly."""
    return np.array([[int(round(255 * c)) for c in colorsys.hsv_to_rgb((i * 0.618033988749895) % 1.0, 1.0, 1.0)]
                     for i in range(int(n))], np.uint8).reshape(-1, 3)


def _palette(palette, device):
    """uint8 (n, 3) on the device; uploaded once per palette and device"""
    p = np.ascontiguousarray(np.asarray(palette.cpu() if isinstance(palette, torch.Tensor) else palette)).reshape(-1, 3)
    if p.size and (p.min() < 0 or p.max() > 255):
        raise ValueError('palette entries must lie in [0, 255]')
    p = p.astype(np.uint8)
    key = (device, p.tobytes())
    if key not in _palettes:
        if len(_palettes) > 64:
            _palettes.clear()
        _palettes[key] = torch.from_numpy(p).to(device)
    return _palettes[key]


def _canvas(canvas, name='canvas'):
    """the caller's canvas as (B, Hc, Wc, 3): it is drawn in place, so it must be a contiguous uint8 CUDA tensor"""
    if not isinstance(canvas, torch.Tensor) or not canvas.is_cuda:
        raise RuntimeError('%s must be a CUDA tensor (multipoint_amd computes on the GPU only)' % name)
    if canvas.dtype != torch.uint8 or canvas.dim() not in (3, 4) or canvas.shape[-1] != 3 or not canvas.is_contiguous():
        raise ValueError('%s must be a contiguous uint8 (B, H, W, 3) or (H, W, 3) tensor, got %s %s'
                         % (name, str(canvas.dtype).replace('torch.', ''), tuple(canvas.shape)))
    return canvas if canvas.dim() == 4 else canvas[None]


def _int32(x, device):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=torch.int32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.int32)).to(device)


def _lists(kp, B, device, name):
    """keypoints as int32 (B, K, 2) on the device: (B, K, 2), or one (N, 2) list for a single canvas"""
    kp = _int32(kp, device)
    if kp.dim() == 2 and kp.shape[1] == 2 and B == 1:
        kp = kp[None]
    if kp.dim() != 3 or kp.shape[0] != B or kp.shape[2] != 2:
        raise ValueError('%s must be (B, K, 2) for the %d images, or one (N, 2) list for a single image, got %s'
                         % (name, B, tuple(kp.shape)))
    return kp


def _counts(count, B, K, device, name):
    if count is None:
        return torch.full((B,), K, dtype=torch.int32, device=device)
    count = _int32(count, device).reshape(-1)
    if count.numel() != B:
        raise ValueError('%s must hold one count per image (%d), got %d' % (name, B, count.numel()))
    return count


def _pad_lists(x, K, value):
    if x.shape[1] == K:
        return x
    out = torch.full((x.shape[0], K) + tuple(x.shape[2:]), value, dtype=x.dtype, device=x.device)
    out[:, :x.shape[1]] = x
    return out


def gray_to_rgb(images, valid_mask=None, gain=1.0, out=None, offset=(0, 0)):
    """fp32 frames (B, 1, H, W), (B, H, W) or (H, W) as grey RGB pixels, uint8 (B, H, W, 3): (np.clip(v * gain, 0, 1) *
    255.0).astype(np.uint8) with v = image, or image * valid_mask (a mask of the images' shape, any dtype), NaN as 0.  With
    `out` (a uint8 canvas (B, Hc, Wc, 3), or (Hc, Wc, 3) for one frame) the pixels go to out[:, y0:y0 + H, x0:x0 + W] for
    offset = (y0, x0), clipped to the canvas, nothing else of it is written, and `out` is returned."""
    x = alignment._frames(images, 'images')
    B, H, W = x.shape
    m = None
    if valid_mask is not None:
        m = alignment._frames(valid_mask.to(torch.float32) if isinstance(valid_mask, torch.Tensor) else valid_mask, 'valid_mask')
        if m.shape != x.shape:
            raise ValueError('valid_mask must have the shape of the images, got %s for %s' % (tuple(m.shape), tuple(x.shape)))
    if out is None:
        canvas = result = torch.empty((B, H, W, 3), dtype=torch.uint8, device=x.device)
    else:
        canvas, result = _canvas(out, 'out'), out
        if canvas.shape[0] != B or canvas.device != x.device:
            raise ValueError('out must hold one canvas per frame on the frames\' device')
    h = _lib.get_handle(x.device)
    h.check(h.lib.mp_draw_gray_to_rgb(h.ptr, _lib.ptr(x), _lib.ptr(m), B, H, W, float(gain), _lib.ptr(canvas), canvas.shape[1],
                                      canvas.shape[2], int(offset[0]), int(offset[1]), _lib.stream_ptr(x.device)))
    return result


def draw_keypoints(canvas, kp_yx, kp_count=None, radius=4, color=(0, 255, 0), thickness=1, kind='ring', offset=(0, 0),
                   palette=None):
    """Marks on the keypoints, in place; returns `canvas` (uint8 CUDA (B, H, W, 3) or (H, W, 3)).  kp_yx: (B, K, 2) rows of
    (y, x) with kp_count (B,) entries in use (None: all K), or one (N, 2) list for a single canvas -- a numpy array or a
    torch.nonzero result; what is not on the device is uploaded.  kind 'ring' (thickness t: the discs of radius r + t // 2
    without the one of radius r - (t + 1) // 2), 'disc' or 'cross' (the mark of show_synthetic_images.py).  Mark i is drawn
    in palette[i % n] (default: `color` for all) with the highest index on top; `offset` = (y0, x0) is added to every
    centre, marks are clipped to the canvas.  ValueError: a negative radius, thickness < 1, an outer radius above 64, an
    empty palette, an unknown kind."""
    c = _canvas(canvas)
    if kind not in _lib.MP_DRAW_KINDS:
        raise ValueError('unknown kind of mark: %r (ring, disc or cross)' % (kind,))
    kp = _lists(kp_yx, c.shape[0], c.device, 'kp_yx')
    B, K = kp.shape[:2]
    pal = _palette([color] if palette is None else palette, c.device)
    if K == 0 and pal.shape[0]:
        return canvas
    cnt = _counts(kp_count, B, K, c.device, 'kp_count')
    h = _lib.get_handle(c.device)
    h.check(h.lib.mp_draw_marks(h.ptr, _lib.ptr(kp), _lib.ptr(cnt), B, K, _lib.MP_DRAW_KINDS[kind], int(radius), int(thickness),
                                _lib.ptr(pal) if pal.shape[0] else None, pal.shape[0], _lib.ptr(c), c.shape[1], c.shape[2],
                                int(offset[0]), int(offset[1]), _lib.stream_ptr(c.device)))
    return canvas


def _matches_on(canvas, kp_a, kp_b, count_a, count_b, match_idx, mask, offset_a, offset_b, radius, thickness, palette):
    P = canvas.shape[0]
    dev = canvas.device
    kp_a, kp_b = _lists(kp_a, P, dev, 'kp_optical'), _lists(kp_b, P, dev, 'kp_thermal')
    count_a = _counts(count_a, P, kp_a.shape[1], dev, 'count_optical')
    count_b = _counts(count_b, P, kp_b.shape[1], dev, 'count_thermal')
    idx = _int32(match_idx, dev)
    idx = idx[None] if idx.dim() == 1 and P == 1 else idx
    if idx.dim() != 2 or idx.shape[0] != P or idx.shape[1] > kp_a.shape[1]:
        raise ValueError('match_idx must be (P, K): one entry per optical keypoint, got %s' % (tuple(idx.shape),))
    pal = _palette(match_palette() if palette is None else palette, dev)
    K = max(kp_a.shape[1], kp_b.shape[1])
    if K == 0 and pal.shape[0]:
        return
    kp_a, kp_b, idx = _pad_lists(kp_a, K, 0), _pad_lists(kp_b, K, 0), _pad_lists(idx, K, -1)
    m = None
    if mask is not None:
        m = mask.to(device=dev) if isinstance(mask, torch.Tensor) else torch.from_numpy(np.asarray(mask)).to(dev)
        m = (m != 0).to(torch.uint8)
        m = m[None] if m.dim() == 1 and P == 1 else m
        if m.dim() != 2 or m.shape[0] != P or m.shape[1] > K:
            raise ValueError('mask must be (P, K): one entry per optical keypoint, got %s' % (tuple(m.shape),))
        m = _pad_lists(m, K, 0).contiguous()
    h = _lib.get_handle(dev)
    h.check(h.lib.mp_draw_matches(h.ptr, _lib.ptr(kp_a), _lib.ptr(kp_b), _lib.ptr(count_a), _lib.ptr(count_b), _lib.ptr(idx),
                                  _lib.ptr(m), P, K, int(offset_a[0]), int(offset_a[1]), int(offset_b[0]), int(offset_b[1]),
                                  int(radius), int(thickness), _lib.ptr(pal) if pal.shape[0] else None, pal.shape[0],
                                  _lib.ptr(canvas), canvas.shape[1], canvas.shape[2], _lib.stream_ptr(dev)))


def draw_matches(optical, thermal, kp_optical, kp_thermal, match_idx, count_optical=None, count_thermal=None, mask=None,
                 radius=3, thickness=1, palette=None):
    """The match picture (reference predict_align_image_pair.py:197-206, cv2.drawMatches with flags=2): uint8 (P, H, 2 W, 3)
    with the optical frame on the left, the thermal one at column W, and for every optical keypoint q < count_optical with
    0 <= match_idx[q] < count_thermal (and mask[q] != 0 where a mask is given, e.g. RANSAC's inlier mask) a ring on both
    keypoints and the 8-connected segment between them, in palette[q % n] (default match_palette(64)), the highest q on
    top.  Unmatched keypoints are not drawn.  Frames (P, 1, H, W), (P, H, W) or (H, W); keypoint lists (P, K, 2) rows of
    (y, x), match_idx (P, K) (for one pair the leading axis may be left out); lists of different lengths are padded."""
    o, t = alignment._frames(optical, 'optical'), alignment._frames(thermal, 'thermal')
    if o.shape != t.shape or o.device != t.device:
        raise ValueError('optical and thermal must have the same shape and device, got %s and %s' % (tuple(o.shape), tuple(t.shape)))
    P, H, W = o.shape
    canvas = torch.empty((P, H, 2 * W, 3), dtype=torch.uint8, device=o.device)
    gray_to_rgb(o, out=canvas)
    gray_to_rgb(t, out=canvas, offset=(0, W))
    _matches_on(canvas, kp_optical, kp_thermal, count_optical, count_thermal, match_idx, mask, (0, 0), (0, W), radius, thickness,
                palette)
    return canvas


def draw_pair_results(res, images, mask=None, radius=3, thickness=1, palette=None):
    """draw_matches from a PairResults and the interleaved batch (2 P, 1, H, W) PairPipeline.run_interleaved took (image 2 p
    optical, 2 p + 1 thermal): the keypoint lists, counts and matches are read where they are, nothing goes through the host.
    mask: (P, K) as in draw_matches."""
    res.wait()
    x = alignment._frames(images, 'images')
    P, K = res.match_idx.shape
    if x.shape[0] != 2 * P:
        raise ValueError('images must be the interleaved batch of the %d pairs, got %d frames' % (P, x.shape[0]))
    kp = res.kp_yx.reshape(P, 2, K, 2)
    return draw_matches(x[0::2], x[1::2], kp[:, 0], kp[:, 1], res.match_idx, res.kp_count[0::2], res.kp_count[1::2], mask,
                        radius, thickness, palette)


def compose(a, t, mode, alpha=128, cell=32, out=None, offset=(0, 0)):
    """One alignment view of a warped optical frame `a` and a thermal frame `t` (fp32 (B, 1, H, W), (B, H, W) or (H, W); a < 0
    marks the pixels outside the optical frame, the -1 border of alignment.warp_image), uint8 (B, H, W, 3).  With A and T the
    8-bit values of gray_to_rgb (A = 0 outside): 'blend' (A alpha + T (256 - alpha) + 128) >> 8 with alpha in [0, 256],
    'checker' A where x // cell + y // cell is even and T elsewhere, 'anaglyph' (R, G, B) = (A, T, T), 'difference' |A - T|;
    outside pixels show T in all but the anaglyph.  `out` / `offset` as in gray_to_rgb."""
    if mode not in _lib.MP_DRAW_MODES:
        raise ValueError('unknown mode %r (blend, checker, anaglyph or difference)' % (mode,))
    a, t = alignment._frames(a, 'a'), alignment._frames(t, 't')
    if a.shape != t.shape or a.device != t.device:
        raise ValueError('a and t must have the same shape and device, got %s and %s' % (tuple(a.shape), tuple(t.shape)))
    B, H, W = a.shape
    if out is None:
        canvas = result = torch.empty((B, H, W, 3), dtype=torch.uint8, device=a.device)
    else:
        canvas, result = _canvas(out, 'out'), out
        if canvas.shape[0] != B or canvas.device != a.device:
            raise ValueError('out must hold one canvas per frame on the frames\' device')
    h = _lib.get_handle(a.device)
    h.check(h.lib.mp_draw_compose(h.ptr, _lib.ptr(a), _lib.ptr(t), B, H, W, _lib.MP_DRAW_MODES[mode], int(alpha), int(cell),
                                  _lib.ptr(canvas), canvas.shape[1], canvas.shape[2], int(offset[0]), int(offset[1]),
                                  _lib.stream_ptr(a.device)))
    return result


def alignment_views(optical, thermal, transform, modes=('checker', 'anaglyph'), alpha=128, cell=32):
    """{mode: uint8 (B, H, W, 3)} of the optical frames warped onto the thermal ones by alignment.warp_image(optical,
    transform, H, W) -- `transform` maps thermal pixels to optical ones, as everywhere in utils.alignment; one for all
    frames or one per frame."""
    t = alignment._frames(thermal, 'thermal')
    o = alignment._frames(optical, 'optical')
    warped = alignment.warp_image(o[:, None], transform, t.shape[1], t.shape[2])[:, 0]
    return {mode: compose(warped, t, mode, alpha, cell) for mode in modes}


def draw_segments(canvas, segments, seg_count=None, thickness=1, palette=((0, 255, 0),)):
    """Line segments, in place; returns `canvas` (uint8 CUDA (B, H, W, 3) or (H, W, 3)).  segments: (B, N, 5) rows of
    (y0, x0, y1, x1, colour) with seg_count (B,) rows in use (None: all N), or one (N, 5) list for a single canvas.  Segment i
    is the 8-connected walk of draw_matches' lines (clipped to the canvas; a zero-length segment is one pixel), every pixel
    widened to a thickness x thickness box, in palette[colour % n] with the highest i on top.  ValueError: thickness outside
    [1, 15], an empty palette."""
    c = _canvas(canvas)
    seg = _int32(segments, c.device)
    if seg.dim() == 2 and seg.shape[1] == 5 and c.shape[0] == 1:
        seg = seg[None]
    if seg.dim() != 3 or seg.shape[0] != c.shape[0] or seg.shape[2] != 5:
        raise ValueError('segments must be (B, N, 5) for the %d canvases, or one (N, 5) list for a single canvas, got %s'
                         % (c.shape[0], tuple(seg.shape)))
    B, N = seg.shape[:2]
    pal = _palette(palette, c.device)
    if N == 0 and pal.shape[0]:
        return canvas
    cnt = _counts(seg_count, B, N, c.device, 'seg_count')
    h = _lib.get_handle(c.device)
    h.check(h.lib.mp_segments_draw(h.ptr, _lib.ptr(seg), _lib.ptr(cnt), B, N, int(thickness), _lib.ptr(pal) if pal.shape[0] else None,
                                   pal.shape[0], _lib.ptr(c), c.shape[1], c.shape[2], _lib.stream_ptr(c.device)))
    return canvas


def draw_residual_field(canvas, field, frame=0, scale=4, min_rho=None, min_margin=None, tol_px=None, thickness=1, offset=(0, 0)):
    """The needle map of frame `frame` of a residual field (utils.residual.residual_field) on one canvas (uint8 CUDA (H, W, 3)),
    in place: every confident window (utils.residual.confident_windows) gets a segment from its centre c = origin + window // 2
    to c + rint(scale * d), green when |d| <= tol_px and red otherwise; every other window a grey ring of radius 2 at c.  The
    thresholds default to utils.residual.RESIDUAL_THRESHOLDS; `offset` = (y0, x0) is added to every centre."""
    from . import residual
    t = residual.RESIDUAL_THRESHOLDS
    min_rho, min_margin, tol_px = (t[k] if v is None else v for k, v in (('min_rho', min_rho), ('min_margin', min_margin),
                                                                           ('tol_px', tol_px)))
    c = _canvas(canvas)
    if c.shape[0] != 1:
        raise ValueError('draw_residual_field draws one frame on one canvas (H, W, 3)')
    conf = residual.confident_windows(field, min_rho, min_margin)[frame].reshape(-1)
    centre = (np.asarray(field['origin']).reshape(-1, 2) + int(field['window']) // 2 + np.asarray(offset, np.int64)).astype(np.int64)
    d = np.asarray(field['d'], np.float64)[frame].reshape(-1, 2)
    if (~conf).any():
        draw_keypoints(c, centre[~conf][None], radius=2, color=(128, 128, 128), kind='ring')
    if conf.any():
        dc = d[conf]
        tip = centre[conf] + np.rint(float(scale) * dc).astype(np.int64)
        colour = (np.hypot(dc[:, 0], dc[:, 1]) > float(tol_px)).astype(np.int64)
        seg = np.concatenate([centre[conf], tip, colour[:, None]], 1)
        draw_segments(c, seg[None], thickness=thickness, palette=((0, 255, 0), (255, 0, 0)))
    return canvas


def _host_image(rgb):
    a = rgb.detach().cpu().numpy() if isinstance(rgb, torch.Tensor) else np.asarray(rgb)
    if a.ndim == 4 and a.shape[0] == 1:
        a = a[0]
    if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)):
        raise ValueError('a picture is uint8 (H, W, 3) or (H, W), got %s %s' % (a.dtype, a.shape))
    return np.ascontiguousarray(a)


def save_png(path, rgb):
    """Write one uint8 picture (H, W, 3), (1, H, W, 3) or (H, W), tensor or array, as a PNG."""
    from PIL import Image
    Image.fromarray(_host_image(rgb)).save(str(path), format='PNG')


def save_gif(path, frames, dt_ms):
    """Write uint8 pictures of one size as an animated GIF that shows each for dt_ms milliseconds and loops for ever."""
    from PIL import Image
    pics = [Image.fromarray(_host_image(f)) for f in frames]
    if not pics:
        raise ValueError('save_gif: no frames')
    pics[0].save(str(path), format='GIF', save_all=True, append_images=pics[1:], duration=int(dt_ms), loop=0)
