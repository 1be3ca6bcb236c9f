"""ClassicDetectors (reference multipoint/models/ClassicDetectors.py) for `method: LGHD`: FAST-9/16 keypoints and log-Gabor
histogram descriptors, every stage a HIP kernel (csrc/lghd.hip, csrc/fft.hip).  PyTorch only holds the memory.

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
    with torch.cuda.device(dev):
        h.check(h.lib.mp_lghd_describe(h.ptr, _lib.ptr(orientation.contiguous()), B, H, W,
                                       _lib.ptr(kp_yx.to(dev, torch.int32).contiguous()),
                                       _lib.ptr(kp_count.to(dev, torch.int32).contiguous()), K,
                                       _lib.ptr(out) if raw else None, None if raw else _lib.ptr(out), _lib.stream_ptr(dev)))
    return out


class ClassicDetectors:
    default_config = {
        'method': 'SURF',
        'prob_smoothing': False,
        'smoothing_kernel_size': 5,
        'min_keypoints': 100,
        'image_H': 512,
        'image_W': 640,
    }

    def __init__(self, config=None):
        given = dict(config or {})
        self.config = U.dict_update(dict(self.default_config), given)
        method = self.config['method']
        if method in ('SURF', 'SIFT'):
            raise NotImplementedError('ClassicDetectors: %s lives inside opencv-contrib and is not rebuilt here; only LGHD is' % method)
        if method != 'LGHD':
            raise ValueError('Unknown alignment method: ' + str(method))
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
        if not (fft_length_ok(H) and fft_length_ok(W)):
            raise ValueError('LGHD: frame of %d x %d: both sizes must be 2^a 3^b 5^c in [8, 4096]' % (H, W))
        for name, want, got in (('image_H', self._frame[0], H), ('image_W', self._frame[1], W)):
            if want is not None and int(want) != got:
                raise ValueError('ClassicDetectors: the configuration says %s = %d, the frame has %d' % (name, int(want), got))
        u8 = quantize(image).reshape(B, H, W)
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
        return describe(out['orientation'], kp_yx, kp_count)
