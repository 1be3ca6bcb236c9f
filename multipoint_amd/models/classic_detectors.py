"""ClassicDetectors (reference multipoint/models/ClassicDetectors.py) for `method: LGHD`: FAST-9/16 keypoints and log-Gabor
histogram descriptors, every stage a HIP kernel (csrc/lghd.hip, csrc/fft.hip), and -- opt-in through
`implementation: restated` -- for `method: SIFT`: Lowe's detector and descriptor restated from the published algorithm
(csrc/sift.hip).  `method: RIFT` (an extension; csrc/rift.hip, csrc/fft.hip) is Li, Hu and
Ai's phase-congruency keypoints and maximum-index-map histograms, restated from the paper and not verified against the authors'
code.  PyTorch only holds the memory.

The reference runs one image at a time on the host and returns a dense [1,384,H,W] descriptor map with the raw counts
scattered at the keypoints.  Here `forward` takes any batch and returns, besides `prob`, the `orientation` maps the
descriptors are counted from; `describe` turns keypoint lists into unit descriptor rows directly.  The dense map is still
produced for B == 1, for callers written against the reference."""
import ctypes

import numpy as np
import torch

from .. import _lib
from ..utils import utils as U
from ..utils.homographies import gaussian_filter

DESCRIPTOR_SIZE = 384
SIFT_DESCRIPTOR_SIZE = 128
RIFT_DESCRIPTOR_SIZE = 256      # 216 counts (6 x 6 cells x 6 bins), zero-padded to a width the sampler and the matchers take
RIFT_MAX_PATCH = 156            # 36 (patch / 6)^4 stays below 2^24: the sum of squares of a row is exact in fp32
SIFT_NFEATURES = 1000           # the reference's cv2.xfeatures2d.SIFT_create(1000)


def fft_length_ok(n):
    """True for the line lengths the FFT takes: 2^a 3^b 5^c in [8, 4096]."""
    if n < 8 or n > 4096:
        return False
    for r in (2, 3, 5):
        while n % r == 0:
            n //= r
    return n == 1


def log_gabor_bank(H, W, n_scales=4, n_angles=6, min_wavelength=3, multiplier=1.6, sigma_onf=0.75):
    """LGHD.create_filter_bank with LGHD.lowpassfilter(H, W, 0.45, 15) (ClassicDetectors.py:152-203) in float64:
    [n_scales * n_angles][H][W], scale-major, in FFT order (the DC term at [0][0])."""
    x, y = np.meshgrid(np.linspace(-0.5, 0.5, W), np.linspace(-0.5, 0.5, H))
    radius = np.fft.ifftshift(np.sqrt(x ** 2 + y ** 2))
    theta = np.fft.ifftshift(np.arctan2(-y, x))
    sintheta, costheta = np.sin(theta), np.cos(theta)
    lowpass = 1.0 / (1.0 + (radius / 0.45) ** (2 * 15))
    bank = np.zeros((n_scales * n_angles, H, W))
    with np.errstate(divide='ignore'):           # log(0) at the DC term: exp(-inf) = 0, as in the reference
        for sc in range(n_scales):
            wavelength = min_wavelength * multiplier ** sc
            log_gabor = np.exp((-(np.log(radius * wavelength)) ** 2) / (2 * np.log(sigma_onf) ** 2)) * lowpass
            for o in range(n_angles):
                angle = o * np.pi / n_angles
                ds = sintheta * np.cos(angle) - costheta * np.sin(angle)
                dc = costheta * np.cos(angle) + sintheta * np.sin(angle)
                dtheta = np.minimum(np.abs(np.arctan2(ds, dc)) * n_angles * 0.5, np.pi)
                bank[sc * n_angles + o] = log_gabor * ((np.cos(dtheta) + 1) / 2)
    return bank


def fft2d(x, inverse=False, axes=3):
    """Unnormalised DFT of complex64 frames [..., H, W] on the GPU (mp_fft2d): axes 1 = along the rows, 2 = along the columns,
    3 = both.  The inverse conjugates the kernel and does not divide by the length."""
    if x.dtype != torch.complex64 or x.dim() < 2:
        raise ValueError('fft2d takes complex64 tensors of at least two dimensions')
    dev = _lib.require_cuda(x.device)
    H, W = x.shape[-2:]
    xr = torch.view_as_real(x.contiguous())
    out = torch.empty_like(xr)
    planes = x.numel() // (H * W)
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_fft2d(h.ptr, _lib.ptr(xr), _lib.ptr(out), planes, H, W, int(bool(inverse)), int(axes),
                               _lib.stream_ptr(dev)))
    return torch.view_as_complex(out)


def quantize(image):
    """(image * 255.0).astype(np.uint8) of a float32 tensor, on the GPU."""
    dev = _lib.require_cuda(image.device)
    img = image.to(torch.float32).contiguous()
    out = torch.empty(img.shape, dtype=torch.uint8, device=dev)
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_lghd_quantize(h.ptr, _lib.ptr(img), _lib.ptr(out), img.numel(), _lib.stream_ptr(dev)))
    return out


def fast_detect(u8, want_prob=True):
    """u8 [B,H,W] uint8 -> (score uint8 [B,H,W], corners uint8 [B,H,W], prob float32 [B,1,H,W] or None): FAST-9/16 with
    threshold 10 and strict 3 x 3 non-maximum suppression; prob marks the corners whose 40 x 40 patch lies inside the frame."""
    dev = _lib.require_cuda(u8.device)
    B, H, W = u8.shape
    u8 = u8.contiguous()
    score, corners = torch.empty_like(u8), torch.empty_like(u8)
    prob = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev) if want_prob else None
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_lghd_detect(h.ptr, _lib.ptr(u8), B, H, W, _lib.ptr(score), _lib.ptr(corners), _lib.ptr(prob),
                                     _lib.stream_ptr(dev)))
    return score, corners, prob


def orientation_maps(u8, bank):
    """u8 [B,H,W] uint8, bank float32 [24,H,W] -> uint8 [B,4,H,W]: per scale the first of the 6 orientations with the largest
    log-Gabor response magnitude."""
    dev = _lib.require_cuda(u8.device)
    B, H, W = u8.shape
    if not (fft_length_ok(H) and fft_length_ok(W)):
        raise ValueError('LGHD: frame of %d x %d: both sizes must be 2^a 3^b 5^c in [8, 4096]' % (H, W))
    nbytes = ctypes.c_longlong(0)
    h = _lib.get_handle(dev)
    h.check(h.lib.mp_lghd_workspace_bytes(B, H, W, ctypes.byref(nbytes)))
    ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=dev)
    out = torch.empty((B, 4, H, W), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_lghd_orientation(h.ptr, _lib.ptr(u8.contiguous()), _lib.ptr(bank), B, H, W, _lib.ptr(out), _lib.ptr(ws),
                                          nbytes.value, _lib.stream_ptr(dev)))
    return out


def describe(orientation, kp_yx, kp_count, raw=False):
    """orientation uint8 [B,4,H,W], kp_yx int32 [B,K,2], kp_count int32 [B] -> float32 [B,K,384]: the L2-normalised patch
    histograms (raw=True: the counts).  Rows beyond kp_count[b] are zero."""
    dev = _lib.require_cuda(orientation.device)
    B, _, H, W = orientation.shape
    K = kp_yx.shape[1]
    out = torch.empty((B, K, DESCRIPTOR_SIZE), dtype=torch.float32, device=dev)
    if K == 0:
        return out
    h = _lib.get_handle(dev)
    # (named, so that a converted copy lives until the launch is queued: a temporary's block is free for the next one to take)
    orientation, kp_yx, kp_count = orientation.contiguous(), kp_yx.to(dev, torch.int32).contiguous(), kp_count.to(dev, torch.int32).contiguous()
    with torch.cuda.device(dev):
        h.check(h.lib.mp_lghd_describe(h.ptr, _lib.ptr(orientation), B, H, W, _lib.ptr(kp_yx), _lib.ptr(kp_count), K,
                                       _lib.ptr(out) if raw else None, None if raw else _lib.ptr(out), _lib.stream_ptr(dev)))
    return out


def phase_congruency(u8, bank, k=1.0, g=3.0, cutoff=0.5, want_amplitudes=False):
    """u8 [B,H,W] uint8, bank float32 [24,H,W] -> (M float32 [B,H,W], m float32 [B,H,W], mim uint8 [B,H,W], T float32 [B,6]):
    the maximum and minimum moments of phase congruency over the 6 orientations, the maximum index map (the first orientation
    with the largest summed amplitude) and the noise thresholds (mp_phase_congruency).  want_amplitudes: a fifth
    result, float32 [B,6,H,W], the scale-0 amplitude planes the thresholds' medians were taken from."""
    dev = _lib.require_cuda(u8.device)
    B, H, W = u8.shape
    if not (fft_length_ok(H) and fft_length_ok(W)):
        raise ValueError('RIFT: frame of %d x %d: both sizes must be 2^a 3^b 5^c in [8, 4096]' % (H, W))
    nbytes = ctypes.c_longlong(0)
    h = _lib.get_handle(dev)
    h.check(h.lib.mp_rift_workspace_bytes(B, H, W, ctypes.byref(nbytes)))
    ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=dev)
    M = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    m = torch.empty_like(M)
    mim = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    T = torch.empty((B, 6), dtype=torch.float32, device=dev)
    amp = torch.empty((B, 6, H, W), dtype=torch.float32, device=dev) if want_amplitudes else None
    with torch.cuda.device(dev):
        u8, bank = u8.contiguous(), bank.contiguous()
        h.check(h.lib.mp_phase_congruency(h.ptr, _lib.ptr(u8), _lib.ptr(bank), B, H, W, float(k), float(g), float(cutoff),
                                          _lib.ptr(M), _lib.ptr(m), _lib.ptr(mim), _lib.ptr(T), _lib.ptr(amp), _lib.ptr(ws),
                                          nbytes.value, _lib.stream_ptr(dev)))
    return (M, m, mim, T, amp) if want_amplitudes else (M, m, mim, T)


def rift_detect(M, fast_threshold=13, patch_size=96, want_prob=True):
    """M float32 [B,H,W] -> (u8m uint8 [B,H,W], score uint8, corners uint8, prob float32 [B,1,H,W] or None): M stretched to
    0..255 per image, FAST-9/16 with `fast_threshold` and strict 3 x 3 non-maximum suppression on it; prob = score / 255 at the
    corners whose patch lies inside the frame."""
    dev = _lib.require_cuda(M.device)
    B, H, W = M.shape
    M = M.to(torch.float32).contiguous()
    u8m = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    score, corners = torch.empty_like(u8m), torch.empty_like(u8m)
    rng = torch.empty((B, 2), dtype=torch.float32, device=dev)
    prob = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev) if want_prob else None
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_rift_detect(h.ptr, _lib.ptr(M), B, H, W, int(fast_threshold), int(patch_size), _lib.ptr(u8m), _lib.ptr(rng),
                                     _lib.ptr(score), _lib.ptr(corners), _lib.ptr(prob), _lib.stream_ptr(dev)))
    return u8m, score, corners, prob


def rift_describe(mim, kp_yx, kp_count, patch_size=96, raw=False):
    """mim uint8 [B,H,W], kp_yx int32 [B,K,2], kp_count int32 [B] -> float32 [B,K,256]: the L2-normalised histograms of the
    patch's 6 x 6 cells (raw=True: the counts) in columns 0..215, zeros behind them.  Rows beyond kp_count[b] are zero."""
    dev = _lib.require_cuda(mim.device)
    B, H, W = mim.shape
    K = kp_yx.shape[1]
    out = torch.empty((B, K, RIFT_DESCRIPTOR_SIZE), dtype=torch.float32, device=dev)
    if K == 0:
        return out
    h = _lib.get_handle(dev)
    # (named, so that a converted copy lives until the launch is queued: a temporary's block is free for the next one to take)
    mim, kp_yx, kp_count = mim.contiguous(), kp_yx.to(dev, torch.int32).contiguous(), kp_count.to(dev, torch.int32).contiguous()
    with torch.cuda.device(dev):
        h.check(h.lib.mp_rift_describe(h.ptr, _lib.ptr(mim), B, H, W, int(patch_size), _lib.ptr(kp_yx), _lib.ptr(kp_count), K,
                                       _lib.ptr(out) if raw else None, None if raw else _lib.ptr(out), _lib.stream_ptr(dev)))
    return out


def sift_capacity(H, W):
    """list slots per image the model asks for: one per 8 pixels, at least 4096 (flags report an overflow)"""
    return max(4096, (H * W) // 8)


class SiftWorkspace:
    """The one buffer every SIFT stage of a batch works in (mp_sift_workspace_bytes), and views of the stages' results in it."""

    def __init__(self, B, H, W, capacity, device):
        self.dev = _lib.require_cuda(device)
        self.B, self.H, self.W, self.capacity = B, H, W, int(capacity)
        self.h = _lib.get_handle(self.dev)
        nbytes = ctypes.c_longlong(0)
        if self.h.lib.mp_sift_workspace_bytes(B, H, W, self.capacity, ctypes.byref(nbytes)) != _lib.MP_OK:
            raise ValueError('SIFT: need 1 <= B <= 65535, frames of 16 x 16 to 4096 x 4096 and 1 <= capacity <= 2^24 (got B = %d, '
                             '%d x %d, capacity %d)' % (B, H, W, self.capacity))
        self.nbytes = nbytes.value
        self.buf = torch.empty((self.nbytes,), dtype=torch.uint8, device=self.dev)
        lay = (ctypes.c_longlong * (8 + 4 * 16))()
        _lib.check(self.h.lib.mp_sift_layout(B, H, W, self.capacity, lay))
        self.layout = list(lay)
        self.octaves = self.layout[0]

    def _view(self, offset, dtype, shape):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        return self.buf[offset:offset + n].view(dtype).reshape(shape)

    def pyramids(self):
        """([gauss [B,6,h,w] per octave], [dog [B,5,h,w] per octave]) as views of the workspace"""
        g, d = [], []
        for o in range(self.octaves):
            h, w, go, do = self.layout[8 + 4 * o:12 + 4 * o]
            g.append(self._view(go, torch.float32, (self.B, 6, h, w)))
            d.append(self._view(do, torch.float32, (self.B, 5, h, w)))
        return g, d

    def candidates(self):
        """(int32 [B,capacity,4] octave, layer, row, column; int32 [B] counts, which may exceed the capacity)"""
        return (self._view(self.layout[1], torch.int32, (self.B, self.capacity, 4)), self._view(self.layout[2], torch.int32, (self.B,)))

    def refined(self):
        """per candidate slot: (float32 [B,capacity,5] x, y, size, response, octave * 8 + layer in doubled-base coordinates; int32
        [B,capacity] emitted orientations; int32 [B,capacity,4] final row, final column, peak bins 0..17 / 18..35 as bit masks)"""
        shape = (self.B, self.capacity)
        return (self._view(self.layout[5], torch.float32, shape + (5,)), self._view(self.layout[6], torch.int32, shape),
                self._view(self.layout[7], torch.int32, shape + (4,)))

    def oriented(self):
        """(float32 [B,capacity,6] records in doubled-base coordinates; int32 [B] counts, which may exceed the capacity)"""
        return (self._view(self.layout[3], torch.float32, (self.B, self.capacity, 6)), self._view(self.layout[4], torch.int32, (self.B,)))


def sift_scale_space(u8, capacity=None, workspace=None):
    """u8 [B,H,W] uint8 -> SiftWorkspace holding the Gaussian and difference-of-Gaussian pyramids (`.pyramids()`)."""
    dev = _lib.require_cuda(u8.device)
    B, H, W = u8.shape
    ws = workspace or SiftWorkspace(B, H, W, capacity or sift_capacity(H, W), dev)
    with torch.cuda.device(dev):
        ws.h.check(ws.h.lib.mp_sift_scale_space(ws.h.ptr, _lib.ptr(u8.contiguous()), B, H, W, ws.capacity, _lib.ptr(ws.buf), ws.nbytes,
                                                _lib.stream_ptr(dev)))
    return ws


def sift_detect(u8, nfeatures=SIFT_NFEATURES, capacity=None, workspace=None, N=None):
    """u8 [B,H,W] uint8 (None: the pyramids `workspace` already holds) -> (keypoints float32 [B,N,6] = x, y, size, angle,
    response, octave * 8 + layer; count int32 [B]; flags int32 [B]; the SiftWorkspace)."""
    if u8 is None:
        ws = workspace
        B, H, W, dev = ws.B, ws.H, ws.W, ws.dev
    else:
        dev = _lib.require_cuda(u8.device)
        B, H, W = u8.shape
        ws = workspace or SiftWorkspace(B, H, W, capacity or sift_capacity(H, W), dev)
        u8 = u8.contiguous()
    N = int(N or nfeatures)
    kp = torch.empty((B, N, 6), dtype=torch.float32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    flags = torch.empty((B,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws.h.check(ws.h.lib.mp_sift_detect(ws.h.ptr, _lib.ptr(u8), B, H, W, ws.capacity, int(nfeatures), _lib.ptr(ws.buf), ws.nbytes,
                                           _lib.ptr(kp), _lib.ptr(count), _lib.ptr(flags), N, _lib.stream_ptr(dev)))
    return kp, count, flags, ws


def sift_select(records, rec_count, nfeatures=SIFT_NFEATURES, N=None):
    """records float32 [B,M,6] in doubled-base coordinates, rec_count int32 [B] -> (keypoints [B,N,6], count [B]): exact
    duplicates (x, y, size, angle) dropped, the nfeatures largest responses kept in list order, x / y / size halved."""
    dev = _lib.require_cuda(records.device)
    B, M, _ = records.shape
    N = int(N or nfeatures)
    kp = torch.empty((B, N, 6), dtype=torch.float32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    scratch = torch.empty((B * M,), dtype=torch.uint8, device=dev)
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_sift_select(h.ptr, _lib.ptr(records.to(torch.float32).contiguous()), _lib.ptr(rec_count.to(dev, torch.int32).contiguous()),
                                     B, M, int(nfeatures), _lib.ptr(kp), _lib.ptr(count), N, _lib.ptr(scratch), B * M, _lib.stream_ptr(dev)))
    return kp, count


def sift_describe(workspace, keypoints, count):
    """keypoints float32 [B,N,6] (as sift_detect returns them), count int32 [B] -> float32 [B,N,128]: the descriptors (values
    0 .. 255) from the Gaussian pyramid `workspace` holds; rows beyond count[b] are zero."""
    ws = workspace
    B, N, _ = keypoints.shape
    out = torch.empty((B, N, SIFT_DESCRIPTOR_SIZE), dtype=torch.float32, device=ws.dev)
    with torch.cuda.device(ws.dev):
        ws.h.check(ws.h.lib.mp_sift_describe(ws.h.ptr, ws.B, ws.H, ws.W, ws.capacity, _lib.ptr(ws.buf), ws.nbytes,
                                             _lib.ptr(keypoints.to(torch.float32).contiguous()), _lib.ptr(count.to(ws.dev, torch.int32).contiguous()),
                                             N, _lib.ptr(out), _lib.stream_ptr(ws.dev)))
    return out


def sift_scatter(keypoints, count, H, W):
    """-> (prob float32 [B,1,H,W]: 1.0 at (round(y), round(x)) of every keypoint; owner int32 [B,H,W]: the last list index that
    rounds to the pixel, -1 elsewhere)"""
    dev = _lib.require_cuda(keypoints.device)
    B, N, _ = keypoints.shape
    prob = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
    owner = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_sift_scatter(h.ptr, _lib.ptr(keypoints.to(torch.float32).contiguous()), _lib.ptr(count.to(dev, torch.int32).contiguous()),
                                      B, N, H, W, _lib.ptr(prob), _lib.ptr(owner), _lib.stream_ptr(dev)))
    return prob, owner


def sift_dense_map(sift_desc, owner):
    """B == 1: the reference's dense map [1,128,H,W] with the raw row of every pixel's owner, [1,1,H,W] zeros without any keypoint"""
    _, H, W = owner.shape
    yx = torch.nonzero(owner[0] >= 0)
    if not yx.shape[0]:
        return torch.zeros((1, 1, H, W), dtype=torch.float32, device=owner.device)
    dense = torch.zeros((1, SIFT_DESCRIPTOR_SIZE, H, W), dtype=torch.float32, device=owner.device)
    dense[0, :, yx[:, 0], yx[:, 1]] = sift_desc[0, owner[0, yx[:, 0], yx[:, 1]].long()].t()
    return dense


def sift_owner_rows(sift_desc, owner, kp_yx, kp_count):
    """The owner's descriptor row, L2-normalised, for every listed pixel: sift_desc [B,N,128], owner int32 [B,H,W], kp_yx int32
    [B,K,2], kp_count [B] -> float32 [B,K,128]; rows beyond the count and pixels without an owner are zero."""
    B, K = kp_yx.shape[:2]
    dev = sift_desc.device
    if K == 0:
        return torch.zeros((B, 0, SIFT_DESCRIPTOR_SIZE), dtype=torch.float32, device=dev)
    H, W = owner.shape[1:]
    yx = kp_yx.to(dev).long()
    y, x = yx[..., 0].clamp(0, H - 1), yx[..., 1].clamp(0, W - 1)
    idx = owner[torch.arange(B, device=dev)[:, None], y, x].long()                                  # [B,K]
    live = (idx >= 0) & (torch.arange(K, device=dev)[None, :] < kp_count.to(dev)[:, None])
    rows = torch.gather(sift_desc, 1, idx.clamp(min=0)[..., None].expand(B, K, SIFT_DESCRIPTOR_SIZE))
    rows = rows / rows.norm(dim=2, keepdim=True).clamp(min=1e-12)
    return torch.where(live[..., None], rows, torch.zeros_like(rows))


class ClassicDetectors:
    default_config = {
        'method': 'SURF',
        'prob_smoothing': False,
        'smoothing_kernel_size': 5,
        'min_keypoints': 100,
        'image_H': 512,
        'image_W': 640,
    }

    describes_keypoints = True      # pipeline.py: descriptors come from `describe(out, kp, cnt)`, not from sampling a dense map

    def __init__(self, config=None):
        given = dict(config or {})
        # `implementation` (an extension, read from the given configuration only): dict_update would copy a key the defaults lack
        # into self.config, so it is taken out first -- the configuration keeps the reference's six keys
        implementation = given.pop('implementation', None)
        if implementation not in (None, 'restated'):
            raise ValueError("ClassicDetectors: implementation must be 'restated' or absent, got %r" % (implementation,))
        # `patch_size`, `fast_threshold` (extensions of `method: RIFT`): taken out the same way
        rift_keys = {key: given.pop(key) for key in ('patch_size', 'fast_threshold') if key in given}
        self.config = U.dict_update(dict(self.default_config), given)
        method = self.config['method']
        if rift_keys and method != 'RIFT':
            raise ValueError('ClassicDetectors: %s belong(s) to method RIFT, not %s' % (sorted(rift_keys), method))
        self.patch_size, self.fast_threshold = rift_keys.get('patch_size', 96), rift_keys.get('fast_threshold', 13)
        for name, v in (('patch_size', self.patch_size), ('fast_threshold', self.fast_threshold)):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError('ClassicDetectors: %s must be an integer, got %r' % (name, v))
        if self.patch_size <= 0 or self.patch_size % 12 or self.patch_size > RIFT_MAX_PATCH:
            raise ValueError('ClassicDetectors: patch_size must be a positive multiple of 12, at most %d, got %d'
                             % (RIFT_MAX_PATCH, self.patch_size))
        if not 1 <= self.fast_threshold <= 255:
            raise ValueError('ClassicDetectors: fast_threshold must lie in [1, 255], got %d' % self.fast_threshold)
        if method == 'SURF' or (method == 'SIFT' and implementation is None):
            raise NotImplementedError('ClassicDetectors: %s lives inside opencv-contrib and is not rebuilt here; LGHD is, and SIFT as '
                                      'a restatement of the published algorithm behind `implementation: restated`' % method)
        if method not in ('LGHD', 'SIFT', 'RIFT'):
            raise ValueError('Unknown alignment method: ' + str(method))
        self.method = method
        if self.config['prob_smoothing'] and self.config['smoothing_kernel_size'] % 2 == 0:
            raise ValueError('smoothing_kernel_size needs to be uneven')
        # the reference sizes its filter bank by image_H / image_W; here the bank follows the frame, and the two keys only
        # check the frame when the yaml names them
        self._frame = (given.get('image_H'), given.get('image_W'))
        self._banks = {}
        self.device = None
        self.training = False

    # -- nn.Module-like plumbing: there are no weights ----------------------------------------------
    def load_state_dict(self, state_dict, strict=True):
        if state_dict:
            raise ValueError('ClassicDetectors has no weights (got %d tensors)' % len(state_dict))
        return self

    def state_dict(self):
        return {}

    def init_random_weights(self, seed=0):
        return self

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError('ClassicDetectors has nothing to train')
        return self.eval()

    def to(self, device):
        self.device = _lib.require_cuda(device)
        return self

    def cuda(self, device=None):
        return self.to(torch.device('cuda', torch.cuda.current_device() if device is None else device))

    def direct_twin(self):
        return None                 # no convolution algorithm to switch: nothing for the tie-robust redo to re-run

    def filter_bank(self, H, W, device):
        """float32 [24,H,W] on `device`, built once per frame size in float64 and rounded once"""
        key = (H, W, str(device))
        bank = self._banks.get(key)
        if bank is None:
            bank = torch.from_numpy(log_gabor_bank(H, W).astype(np.float32)).to(device)
            self._banks[key] = bank
        return bank

    def forward(self, data):
        image = data['image']
        if image.dim() != 4 or image.shape[1] != 1:
            raise ValueError('image must have shape (B,1,H,W), got %s' % (tuple(image.shape),))
        if self.device is None:
            self.to(image.device)
        if image.device != self.device:
            raise RuntimeError('input image is on %s but the model is on %s' % (image.device, self.device))
        B, _, H, W = image.shape
        if self.method in ('LGHD', 'RIFT') and not (fft_length_ok(H) and fft_length_ok(W)):
            raise ValueError('%s: frame of %d x %d: both sizes must be 2^a 3^b 5^c in [8, 4096]' % (self.method, H, W))
        if self.method == 'RIFT' and self.patch_size > min(H, W):
            raise ValueError('RIFT: a frame of %d x %d holds no patch of %d' % (H, W, self.patch_size))
        for name, want, got in (('image_H', self._frame[0], H), ('image_W', self._frame[1], W)):
            if want is not None and int(want) != got:
                raise ValueError('ClassicDetectors: the configuration says %s = %d, the frame has %d' % (name, int(want), got))
        u8 = quantize(image).reshape(B, H, W)
        if self.method == 'SIFT':
            return self._smooth(self._forward_sift(u8))
        if self.method == 'RIFT':
            return self._smooth(self._forward_rift(u8))
        _, _, prob = fast_detect(u8)
        orientation = orientation_maps(u8, self.filter_bank(H, W, self.device))
        out = {'prob': prob, 'orientation': orientation}
        if B == 1:
            # the reference's dense map (ClassicDetectors.py:62-73): raw counts at the keypoints, [1,1,H,W] zeros without any
            kp = torch.nonzero(prob[0, 0] > 0).to(torch.int32)
            n = kp.shape[0]
            if n:
                raw = describe(orientation, kp.reshape(1, n, 2), torch.tensor([n], dtype=torch.int32, device=self.device), raw=True)
                desc = torch.zeros((1, DESCRIPTOR_SIZE, H, W), dtype=torch.float32, device=self.device)
                desc[0, :, kp[:, 0].long(), kp[:, 1].long()] = raw[0].t()
            else:
                desc = torch.zeros((1, 1, H, W), dtype=torch.float32, device=self.device)
            out['desc'] = desc
        return self._smooth(out)

    def _forward_sift(self, u8):
        """detect + describe + scatter.  The reference's second detector, SIFT_create(1500) when fewer than
        min_keypoints are found, only raises a cap that fewer than 100 keypoints never reach: there is no second pass."""
        B, H, W = u8.shape
        kp, count, flags, ws = sift_detect(u8)
        desc = sift_describe(ws, kp, count)
        prob, owner = sift_scatter(kp, count, H, W)
        out = {'prob': prob, 'sift_keypoints': kp, 'sift_count': count, 'sift_desc': desc, 'sift_owner': owner, 'sift_flags': flags}
        if B == 1:
            out['desc'] = sift_dense_map(desc, owner)
        return out

    def _forward_rift(self, u8):
        """phase congruency -> FAST on the maximum-moment map.  `prob` carries the FAST score, so the
        pipeline's top-k is RIFT's "select strongest"."""
        B, H, W = u8.shape
        M, m, mim, _ = phase_congruency(u8, self.filter_bank(H, W, self.device))
        _, _, _, prob = rift_detect(M, self.fast_threshold, self.patch_size)
        out = {'prob': prob, 'mim': mim, 'pc_max': M, 'pc_min': m}
        if B == 1:
            # the dense map callers written against the reference's LGHD expect: raw counts at the keypoints
            kp = torch.nonzero(prob[0, 0] > 0).to(torch.int32)
            n = kp.shape[0]
            if n:
                raw = rift_describe(mim, kp.reshape(1, n, 2), torch.tensor([n], dtype=torch.int32, device=self.device),
                                    self.patch_size, raw=True)
                desc = torch.zeros((1, RIFT_DESCRIPTOR_SIZE, H, W), dtype=torch.float32, device=self.device)
                desc[0, :, kp[:, 0].long(), kp[:, 1].long()] = raw[0].t()
            else:
                desc = torch.zeros((1, 1, H, W), dtype=torch.float32, device=self.device)
            out['desc'] = desc
        return out

    def _smooth(self, out):
        prob = out['prob']
        if self.config['prob_smoothing']:
            # self.filter(F.pad(prob, padding)): zero padding, then the k x k filter over the padded map's interior
            k = int(self.config['smoothing_kernel_size'])
            v = (k - 1) // 2
            if v:
                # (the filter's own reflection only reaches the padding, which is cropped again)
                padded = torch.nn.functional.pad(prob, (v, v, v, v))
                out['prob'] = gaussian_filter(padded, k)[:, :, v:-v, v:-v].contiguous()
        return out

    __call__ = forward

    def describe(self, out, kp_yx, kp_count):
        """[B,K,384] unit rows for the keypoint lists of a forward's output.  This is what the reference's
        interpolate_descriptors yields on the dense map: its sample at (y, x) blends in (y-1, x), (y, x-1) and (y-1, x-1), which
        FAST's strict non-maximum suppression keeps free of keypoints, so the normalised sample is the normalised raw row."""
        if 'sift_owner' in out:
            # SIFT: the row of the keypoint that owns the pixel.  The reference's blend with (y-1, x), (y, x-1), (y-1, x-1) mixes
            # descriptors of DIFFERENT keypoints where one of those pixels holds one; that artefact is not reproduced
            return sift_owner_rows(out['sift_desc'], out['sift_owner'], kp_yx, kp_count)
        if 'mim' in out:
            # RIFT: [B,K,256] histograms of the maximum index map around each keypoint
            return rift_describe(out['mim'], kp_yx, kp_count, self.patch_size)
        return describe(out['orientation'], kp_yx, kp_count)
