"""Homographic augmentation of the dataset samples (multipoint/datasets/augmentation/augmentation.py:25-61), the step
that gives the prediction / evaluation configs their ground-truth homography and valid mask
(configs/config_image_pair_dataset_prediction.yaml: augmentation.homographic.enable = true).

The homography is sampled on the host exactly as the reference does (`utils.sample_homography`, numpy's global
generator); the pixel work runs in HIP behind the C ABI: `mp_warp_perspective_cv` restates
cv2.warpPerspective(INTER_LINEAR, BORDER_REFLECT_101 | BORDER_CONSTANT), `mp_ha_valid_mask` restates
compute_valid_mask.  No CPU fallback.

Photometric augmentation (augmentation.py:8-22, photometric_augmentation.py) is split the same way: the host draws a small
per-image plan with the reference's random / np.random calls in the reference's order (draw_photometric_plan), the pixel
work runs in HIP (mp_photometric_augment).  The caller chooses the noise mode with the config key
`noise`: 'host' draws the reference's per-pixel normal / uniform fields with np.random (and uploads them), 'device' draws
one 63-bit key per field from np.random instead and the GPU hashes (key, pixel) into the field."""
import ctypes
import random

import numpy as np
import torch

from .. import _lib
from ..utils import homographies as hom

__all__ = ['homographic_augmentation', 'homographic_augmentation_batch', 'warp_perspective_cv', 'dummy_valid_mask', 'cv_invert3',
           'photometric_augmentation', 'photometric_augmentation_batch', 'draw_photometric_plan', 'photometric_noise_mode',
           'PHOTOMETRIC_PRIMITIVES']


def cv_invert3(m):
    """cv::invert of a 3x3 float64 matrix (closed-form adjugate / determinant, what cv2.warpPerspective applies to
    M before it maps destination to source pixels).  A singular matrix gives zeros, as OpenCV does."""
    s = np.asarray(m, dtype=np.float64).reshape(3, 3)
    c00 = s[1, 1] * s[2, 2] - s[1, 2] * s[2, 1]
    c01 = s[1, 0] * s[2, 2] - s[1, 2] * s[2, 0]
    c02 = s[1, 0] * s[2, 1] - s[1, 1] * s[2, 0]
    det = s[0, 0] * c00 - s[0, 1] * c01 + s[0, 2] * c02
    if det == 0.0:
        return np.zeros((3, 3))
    d = 1.0 / det
    return np.array([[c00 * d, (s[0, 2] * s[2, 1] - s[0, 1] * s[2, 2]) * d, (s[0, 1] * s[1, 2] - s[0, 2] * s[1, 1]) * d],
                     [(s[1, 2] * s[2, 0] - s[1, 0] * s[2, 2]) * d, (s[0, 0] * s[2, 2] - s[0, 2] * s[2, 0]) * d,
                      (s[0, 2] * s[1, 0] - s[0, 0] * s[1, 2]) * d],
                     [c02 * d, (s[0, 1] * s[2, 0] - s[0, 0] * s[2, 1]) * d, (s[0, 0] * s[1, 1] - s[0, 1] * s[1, 0]) * d]])


def warp_perspective_cv(images, homographies, border_reflect=False):
    """cv2.warpPerspective(image, H, (W, H), borderMode=BORDER_CONSTANT | BORDER_REFLECT_101) with INTER_LINEAR for a
    batch of fp32 images (B,1,H,W) on the GPU (mp_warp_perspective_cv); homographies (B,3,3) map source to destination
    pixels.  Used by the dataset augmentation below and by predict_align_image_pair.py to warp the optical image onto
    the thermal one with the estimated homography (reference predict_align_image_pair.py:218)."""
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 1:
        raise ValueError('warp_perspective_cv: images must be a (B,1,H,W) tensor')
    dev = _lib.require_cuda(images.device if images.device.type == 'cuda' else None)
    src = images.to(dev, torch.float32).contiguous()
    B, _, H, W = src.shape
    h_np = np.asarray(homographies, dtype=np.float64).reshape(-1, 3, 3)
    if h_np.shape[0] != B:
        raise ValueError('warp_perspective_cv: one homography per image expected')
    inv_cv = torch.from_numpy(np.stack([cv_invert3(m) for m in h_np]).reshape(B, 9)).to(dev)
    out = torch.empty_like(src)
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_warp_perspective_cv(h.ptr, _lib.ptr(src), B, H, W, _lib.ptr(inv_cv),
                                             1 if border_reflect else 0, _lib.ptr(out), _lib.stream_ptr(dev)))
    return out


def homographic_augmentation_batch(images, homographies, border_reflect=True, valid_border_margin=0,
                                   mask_border=True):
    """images (B,1,H,W) fp32 on the GPU, homographies (B,3,3) source -> destination pixel maps (host).
    Returns the warped images (B,1,H,W) fp32 and the valid masks (B,1,H,W) bool, both on the GPU."""
    out = warp_perspective_cv(images, homographies, border_reflect)
    dev = out.device
    B, _, H, W = out.shape
    h_np = np.asarray(homographies, dtype=np.float64).reshape(-1, 3, 3)
    # compute_valid_mask(image_shape, homography, valid_border_margin * 2, mask_border)  (augmentation.py:38-40)
    mask = hom._valid_masks(np.linalg.inv(h_np), (H, W), int(valid_border_margin) * 2, mask_border, dev)
    return out, mask.view(B, 1, H, W).bool()


def homographic_augmentation(image, keypoints=None, return_homography=False, **config):
    """augmentation.py:25-54: warp an (H,W) image with a random homography drawn from config['params'], warp and
    filter the (N,2) (y,x) keypoints, compute the valid mask.  numpy in, numpy out, like the reference; a CUDA
    tensor image is accepted too and then image / mask stay on the GPU (warped_image (H,W) fp32, valid_mask (H,W))."""
    on_gpu = torch.is_tensor(image)
    image_shape = tuple(image.shape)
    if len(image_shape) != 2:
        raise ValueError('homographic_augmentation: expected an (H,W) image, got shape {}'.format(image_shape))
    homography = hom.sample_homography(image_shape, **config['params'])
    img = image if on_gpu else torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32))
    dev = _lib.require_cuda(img.device if img.device.type == 'cuda' else None)
    warped, mask = homographic_augmentation_batch(img.to(dev)[None, None], homography[None],
                                                  config['border_reflect'], config['valid_border_margin'],
                                                  config['mask_border'])
    if on_gpu:
        warped_image, valid_mask = warped[0, 0], mask[0, 0]
    else:
        warped_image = warped[0, 0].cpu().numpy()
        valid_mask = mask[0, 0].cpu().numpy().astype(np.float64)
    if keypoints is not None:
        if keypoints.size > 0:
            warped_points = hom.filter_points(hom.warp_keypoints(keypoints, homography), image_shape)
        else:
            warped_points = keypoints
    else:
        warped_points = None
    if return_homography:
        return warped_image, warped_points, valid_mask, homography
    return warped_image, warped_points, valid_mask


def dummy_valid_mask(image_shape):
    """augmentation.py:56-61."""
    return np.ones(image_shape)


# photometric_augmentation.py:4-11, in the reference's order ('all')
PHOTOMETRIC_PRIMITIVES = ['additive_gaussian_noise', 'additive_speckle_noise', 'random_brightness', 'random_contrast',
                          'additive_shade', 'motion_blur']
NOISE_MODES = ('host', 'device')
_KIND = {'additive_gaussian_noise': 0, 'additive_speckle_noise': 1, 'random_brightness': 2, 'random_contrast': 3,
         'additive_shade': 4, 'motion_blur': 5}
_GAUSSIAN_ADD = 6
_MOTION_MODES = ['h', 'v', 'diag_down', 'diag_up']


def photometric_noise_mode(config, who='photometric augmentation'):
    """The `noise` key of an enabled augmentation.photometric block: 'host' or 'device'.  Absent: NotImplementedError (the
    caller must choose); anything else: ValueError."""
    mode = config.get('noise')
    if mode is None:
        raise NotImplementedError(
            "%s: photometric augmentation needs augmentation.photometric.noise: 'host' (the reference's np.random "
            "per-pixel noise fields, drawn on the host) or 'device' (noise fields hashed on the GPU from one np.random "
            "key per field)" % who)
    if mode not in NOISE_MODES:
        raise ValueError("%s: augmentation.photometric.noise must be 'host' or 'device', got %r" % (who, mode))
    return mode


def _parse_primitives(names):
    """utils.parse_primitives (multipoint/utils/utils.py:52-56)."""
    p = PHOTOMETRIC_PRIMITIVES if names == 'all' else (names if isinstance(names, list) else [names])
    assert set(p) <= set(PHOTOMETRIC_PRIMITIVES)
    return p


def _motion_taps(mode, ksize):
    """motion_blur's kernel (photometric_augmentation.py:59-76) as the float32 weights of its non-zero entries in row-major
    order (what cv2.filter2D sums)."""
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
    return [float(k32[i, j]) for i in range(ksize) for j in range(ksize) if k32[i, j] != 0]


def _key():
    return int(np.random.randint(0, 2 ** 63, dtype=np.int64))


class PhotometricPlan:
    """The draws of one photometric_augmentation call: `ops` in the order they run, each a dict with the primitive's
    scalar draws; in 'host' noise mode the per-pixel fields ('normal' / 'uniform', float64 (H,W)), in 'device' mode a
    'key' instead."""

    def __init__(self, shape, noise, ops):
        self.shape, self.noise, self.ops = tuple(shape), noise, ops

    def inplace_prefix(self):
        """The part of the chain that mutates the INPUT array (photometric_augmentation.py: additive_speckle_noise works in
        place and returns its input, additive_gaussian_noise adds in place before np.clip returns a new array, every other
        primitive returns a new array): the leading speckle ops and a following gaussian add without its clip.  None when
        the chain leaves its input untouched."""
        ops = []
        for op in self.ops:
            if op['name'] == 'additive_speckle_noise':
                ops.append(op)
                continue
            if op['name'] == 'additive_gaussian_noise':
                ops.append(dict(op, name='gaussian_add'))
            break
        return PhotometricPlan(self.shape, self.noise, ops) if ops else None


def draw_photometric_plan(shape, config):
    """augmentation.py:8-22 without the pixel work: consumes `random` / `np.random` exactly as the reference's
    photometric_augmentation(image, **config) does for an image of `shape` (H, W) -- parse_primitives, the random.shuffle
    of the indices when random_order is set, then each primitive's draws in the shuffled order with its defaults
    (photometric_augmentation.py) -- except that config['noise'] == 'device' replaces each H x W field draw by one key."""
    noise = photometric_noise_mode(config)
    H, W = int(shape[0]), int(shape[1])
    primitives = _parse_primitives(config['primitives'])
    params = config.get('params', {}) or {}
    cfgs = [params.get(p, {}) for p in primitives]
    indices = np.arange(len(primitives))
    if config['random_order']:
        random.shuffle(indices)
    ops = []
    for i in range(len(primitives)):
        idx = indices[i]
        name, c = primitives[idx], cfgs[idx]
        op = {'name': name}
        if name == 'additive_gaussian_noise':
            op['value'] = np.random.uniform(*c.get('stddev_range', [0.0, 0.06]))
            if noise == 'host':
                op['normal'] = np.random.normal(loc=0.0, scale=op['value'], size=(H, W))
            else:
                op['key'] = _key()
        elif name == 'additive_speckle_noise':
            op['value'] = np.random.uniform(*c.get('prob_range', [0.0, 0.005]))
            if noise == 'host':
                op['uniform'] = np.random.uniform(size=(H, W))
            else:
                op['key'] = _key()
        elif name == 'random_brightness':
            m = c.get('max_abs_change', 0.2)
            op['value'] = np.random.uniform(-m, m)
        elif name == 'random_contrast':
            op['value'] = np.random.uniform(*c.get('strength_range', [0.5, 1.5]))
        elif name == 'additive_shade':
            min_dim = min(H, W) / 4
            ellipses = []
            for _ in range(c.get('nb_ellipses', 20)):
                ax = int(max(np.random.rand() * min_dim, min_dim / 5))
                ay = int(max(np.random.rand() * min_dim, min_dim / 5))
                max_rad = max(ax, ay)
                x = np.random.randint(max_rad, W - max_rad)
                y = np.random.randint(max_rad, H - max_rad)
                angle = np.random.rand() * 90
                ellipses.append((int(x), int(y), ax, ay, int(round(angle))))      # cv::ellipse: cvRound(angle)
            op['ellipses'] = ellipses
            op['value'] = np.random.uniform(*c.get('transparency_range', [-0.5, 0.8]))
            k = np.random.randint(*c.get('kernel_size_range', [250, 350]))
            op['ksize'] = int(k + 1 if k % 2 == 0 else k)
        elif name == 'motion_blur':
            mode = np.random.choice(_MOTION_MODES)
            ksize = np.random.randint(0, (c.get('max_kernel_size', 10) + 1) / 2) * 2 + 1
            op['mode'], op['ksize'] = _MOTION_MODES.index(str(mode)), int(ksize)
            op['taps'] = _motion_taps(str(mode), int(ksize))
        ops.append(op)
    return PhotometricPlan((H, W), noise, ops)


def _c_plans(plans, H, W, dev):
    """ctypes plans, the ellipse table and the stacked host noise fields (device float64) of a batch."""
    n = len(plans)
    c = (_lib.PhotometricPlan * n)()
    ellipses, normal, uniform = [], [], []
    for i, plan in enumerate(plans):
        if plan.shape != (H, W):
            raise ValueError('photometric augmentation: plan %d was drawn for %s, the images are %s' % (i, plan.shape, (H, W)))
        if len(plan.ops) > _lib.MP_PHOTO_MAX_OPS:
            raise ValueError('photometric augmentation: at most %d primitives per image' % _lib.MP_PHOTO_MAX_OPS)
        c[i].n_ops, c[i].noise_device = len(plan.ops), int(plan.noise == 'device')
        for j, op in enumerate(plan.ops):
            o = c[i].op[j]
            o.kind = _GAUSSIAN_ADD if op['name'] == 'gaussian_add' else _KIND[op['name']]
            o.value = float(op.get('value', 0.0))
            o.key = int(op.get('key', 0))
            if 'normal' in op:
                o.field = len(normal)
                normal.append(op['normal'])
            if 'uniform' in op:
                o.field = len(uniform)
                uniform.append(op['uniform'])
            if op['name'] == 'additive_shade':
                o.ksize, o.ellipse_offset, o.ellipse_count = op['ksize'], len(ellipses), len(op['ellipses'])
                ellipses.extend(op['ellipses'])
            elif op['name'] == 'motion_blur':
                o.ksize, o.mode = op['ksize'], op['mode']
                for t, w in enumerate(op['taps']):
                    o.taps[t] = w
    ell = np.ascontiguousarray(np.asarray(ellipses, np.int32).reshape(-1, 5))

    def fields(f):
        return torch.from_numpy(np.stack(f).astype(np.float64)).to(dev) if f else None
    return c, ell, fields(normal), fields(uniform)


def _workspace(n, H, W, n_ellipses, dev):
    nbytes = ctypes.c_longlong()
    _lib.check(_lib.load_library().mp_photometric_workspace_bytes(n, H, W, n_ellipses, ctypes.byref(nbytes)))
    return torch.empty(nbytes.value, dtype=torch.uint8, device=dev)


def prepare_photometric(plans, H, W, device=None):
    """The launch arguments of a batch of plans: ctypes plans, ellipse table, the host noise fields uploaded to the device
    (float64) and the workspace.  photometric_augmentation_batch runs prepare + launch; tools/bench_photometric.py times
    launch_photometric alone."""
    dev = _lib.require_cuda(device)
    c, ell, normal, uniform = _c_plans(plans, H, W, dev)
    return {'plans': c, 'ellipses': ell, 'normal': normal, 'uniform': uniform, 'n': len(plans), 'H': H, 'W': W,
            'workspace': _workspace(len(plans), H, W, ell.shape[0], dev), 'device': dev}


def launch_photometric(prep, src, dst):
    """mp_photometric_augment on (n,1,H,W) fp32 device tensors src -> dst (dst may be src)."""
    dev, ell, normal, uniform, ws = prep['device'], prep['ellipses'], prep['normal'], prep['uniform'], prep['workspace']
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_photometric_augment(
            h.ptr, _lib.ptr(src), _lib.ptr(dst), prep['n'], prep['H'], prep['W'], prep['plans'],
            ell.ctypes.data_as(ctypes.c_void_p), ell.shape[0], _lib.ptr(normal), 0 if normal is None else normal.shape[0],
            _lib.ptr(uniform), 0 if uniform is None else uniform.shape[0], _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    return dst


def photometric_augmentation_batch(images, plans, out=None):
    """images (B,1,H,W) fp32 on the GPU, plans: B PhotometricPlan (draw_photometric_plan).  Returns the augmented images
    (B,1,H,W) fp32 on the GPU (written into `out` when given; out may be `images`)."""
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 1:
        raise ValueError('photometric_augmentation_batch: images must be a (B,1,H,W) tensor')
    dev = _lib.require_cuda(images.device if images.device.type == 'cuda' else None)
    src = images.to(dev, torch.float32).contiguous()
    B, _, H, W = src.shape
    if len(plans) != B:
        raise ValueError('photometric_augmentation_batch: one plan per image expected')
    prep = prepare_photometric(plans, H, W, dev)
    return launch_photometric(prep, src, torch.empty_like(src) if out is None else out)


def photometric_shade_masks(plans, op_index, blurred=True, device=None):
    """The additive_shade masks of op `op_index` of each plan (B,H,W) fp32 on the GPU: the filled ellipses (cv2.ellipse) or,
    with blurred, the mask after cv2.GaussianBlur; zeros where that op is no shade."""
    dev = _lib.require_cuda(device)
    H, W = plans[0].shape
    c, ell, _, _ = _c_plans(plans, H, W, dev)
    ws = _workspace(len(plans), H, W, ell.shape[0], dev)
    out = torch.empty((len(plans), H, W), dtype=torch.float32, device=dev)
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_photometric_shade_mask(h.ptr, len(plans), H, W, c, ell.ctypes.data_as(ctypes.c_void_p),
                                                ell.shape[0], op_index, 1 if blurred else 0, _lib.ptr(out), _lib.ptr(ws),
                                                ws.numel(), _lib.stream_ptr(dev)))
    return out


def apply_photometric_plans(image, plans):
    """Run the plans of consecutive photometric_augmentation calls on the SAME input array, the way the reference's
    aliasing works (ImagePairDataset.py:178-193 with random_pairs: a single flip makes optical and thermal one array):
    each call first mutates the shared input with its in-place prefix, then returns its own new image.  image: an (H,W)
    CUDA tensor; returns one (H,W) CUDA tensor per plan."""
    cur = image.to(torch.float32).contiguous().clone()
    outs = []
    for k, plan in enumerate(plans):
        outs.append(photometric_augmentation_batch(cur[None, None], [plan])[0, 0])
        if k + 1 < len(plans):
            prefix = plan.inplace_prefix()
            if prefix is not None:
                photometric_augmentation_batch(cur[None, None], [prefix], out=cur[None, None])
    return outs


def photometric_augmentation(image, **config):
    """augmentation.py:8-22: the config's primitives (photometric_augmentation.py) applied to an (H,W) image, drawing from
    `random` / `np.random` as the reference does (config['noise'] chooses where the per-pixel noise comes from).  numpy in,
    numpy float32 out, like the reference -- including the reference's in-place update of the input by a leading
    speckle / gaussian noise -- or an (H,W) CUDA tensor in and out, staying on the GPU."""
    on_gpu = torch.is_tensor(image)
    if len(tuple(image.shape)) != 2:
        raise ValueError('photometric_augmentation: expected an (H,W) image, got shape {}'.format(tuple(image.shape)))
    plan = draw_photometric_plan(tuple(image.shape), config)
    img = image if on_gpu else torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32))
    dev = _lib.require_cuda(img.device if img.device.type == 'cuda' else None)
    src = img.to(dev, torch.float32).contiguous()
    out = photometric_augmentation_batch(src[None, None], [plan])[0, 0]
    prefix = plan.inplace_prefix()
    if prefix is not None:
        mutated = photometric_augmentation_batch(src[None, None], [prefix])[0, 0]
        if on_gpu:
            image.copy_(mutated)
        elif image.dtype == np.float32 and image.flags.writeable:
            image[...] = mutated.cpu().numpy()
    return out if on_gpu else out.cpu().numpy()
