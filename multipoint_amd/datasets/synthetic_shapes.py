"""The SyntheticShapes dataset (multipoint/datasets/SyntheticShapes.py): random backgrounds with one of nine geometric
primitives, whose corners are the keypoint labels the detector is first trained on.

The host draws every `random` / `np.random` call of the reference in the reference's order into a plan of draw commands
(utils/draw_primitives.py); the GPU does all pixel work (csrc/shapes.hip): noise threshold, blobs, box
blur, the primitive, the Gaussian blurs and the resize.  The image is fp32 from the canvas on, where the reference keeps
float64 until its final cast.  Only draw_checkerboard reads a number back from the device (the background mean its colour
loop depends on); `SyntheticShapes.sync_count` counts those reads.

`generation.noise` chooses the background's noise field: 'host' draws the reference's np.random.rand(H, W) and uploads it,
'device' draws one key from np.random and hashes it per pixel.  gaussian_noise (cv2.randu, which the reference never
seeds) always hashes, from `generation.randu_seed` and the sample counter, and consumes no `random` / `np.random` draw.
An enabled photometric block needs its own `noise` key, as in ImagePairDataset."""
import copy
import ctypes
import random

import numpy as np
import torch
from torch.utils.data.dataset import Dataset

from .. import _lib
from ..utils import draw_primitives
from ..utils.utils import dict_update
from . import augmentation
from .image_pair_dataset import _open_store, check_augmentation_config, generate_keypoint_map

NOISE_MODES = ('host', 'device')
_KIND = {'threshold': _lib.MP_SHAPES_THRESHOLD, 'mean': _lib.MP_SHAPES_MEAN, 'blobs': _lib.MP_SHAPES_BLOBS,
         'box_blur': _lib.MP_SHAPES_BOX_BLUR, 'line': _lib.MP_SHAPES_LINE, 'convex': _lib.MP_SHAPES_CONVEX,
         'poly': _lib.MP_SHAPES_POLY, 'ellipse': _lib.MP_SHAPES_ELLIPSE, 'randu': _lib.MP_SHAPES_RANDU}


def parse_primitives(names, all_primitives):
    """utils.parse_primitives (multipoint/utils/utils.py:52-56)."""
    p = all_primitives if (names == 'all') else (names if isinstance(names, list) else [names])
    assert set(p) <= set(all_primitives)
    return p


def _set_color(cmd, color):
    cmd.resolve = int(color.call >= 0)
    cmd.u, cmd.col_a, cmd.col_b, cmd.min_contrast = color.u, color.a, color.b, color.min_contrast


def encode_commands(command_lists, field_base):
    """The C arrays of the command lists of n images: (cmds, cmd_offset, verts, circles, circle_colors).  field_base[i] is
    the index of image i's first host noise field in the stacked fields."""
    total = sum(len(c) for c in command_lists)
    cmds = (_lib.ShapesCmd * max(total, 1))()
    offset = np.zeros(len(command_lists) + 1, np.int32)
    verts, circles, colors = [], [], []
    n_verts = n_circles = 0
    k = 0
    for i, commands in enumerate(command_lists):
        for c in commands:
            cmd = cmds[k]
            k += 1
            kind = c['kind']
            cmd.kind, cmd.target = _KIND[kind], int(c.get('target', 0))
            if kind == 'threshold':
                cmd.a[0] = field_base[i] + c['field'] if c['field'] >= 0 else -1
                cmd.t, cmd.key = c['t'], c['key']
            elif kind == 'randu':
                cmd.key = c['key']
            elif kind == 'blobs':
                cmd.a[0], cmd.a[1], cmd.a[2] = n_circles, len(c['circles']), int(c['base'] is not None)
                circles.append(np.asarray(c['circles'], np.int32).reshape(-1, 3))
                colors.append(np.asarray(c['colors'], np.float64).reshape(-1, 2))
                n_circles += len(c['circles'])
                if c['base'] is not None:
                    if (c['base'].call >= 0) != bool(c['resolve']):
                        raise ValueError('blobs: the fill and the circles are all resolved on the device or all literal')
                    _set_color(cmd, c['base'])
                cmd.resolve, cmd.min_contrast = int(bool(c['resolve'])), c['min_contrast']
            elif kind == 'box_blur':
                cmd.a[0] = c['k']
            elif kind == 'line':
                cmd.a[0], cmd.a[1], cmd.a[2], cmd.a[3], cmd.a[4] = c['p1'][0], c['p1'][1], c['p2'][0], c['p2'][1], c['thickness']
                _set_color(cmd, c['color'])
            elif kind in ('convex', 'poly'):
                pts = np.asarray(c['points'], np.int32).reshape(-1, 2)
                cmd.a[0], cmd.a[1], cmd.a[2] = n_verts, len(pts), int(bool(c.get('copy', False)))
                verts.append(pts)
                n_verts += len(pts)
                _set_color(cmd, c['color'])
            elif kind == 'ellipse':
                cmd.a[0], cmd.a[1], cmd.a[2], cmd.a[3], cmd.a[4] = (c['center'][0], c['center'][1], c['axes'][0], c['axes'][1],
                                                                    c['angle'])
                _set_color(cmd, c['color'])
        offset[i + 1] = k

    def cat(parts, width, dtype):
        return np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros((0, width), dtype), dtype)
    return cmds, offset, cat(verts, 2, np.int32), cat(circles, 3, np.int32), cat(colors, 2, np.float64)


def _workspace(n, H, W, n_cmds, n_verts, n_circles, dev, cache=None):
    nbytes = ctypes.c_longlong()
    _lib.check(_lib.load_library().mp_shapes_workspace_bytes(n, H, W, n_cmds, n_verts, n_circles, ctypes.byref(nbytes)))
    if cache is not None and cache.get('ws') is not None and cache['ws'].numel() >= nbytes.value and cache['ws'].device == dev:
        return cache['ws']
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    if cache is not None:
        cache['ws'] = ws
    return ws


def render(canvas, mean, command_lists, fields=(), field_base=None, cache=None):
    """mp_shapes_render: replay the command lists of n images on canvas (n,H,W) fp32 CUDA, in place; mean (n,) float64
    CUDA holds the device means (read and written).  fields: host float64 (H,W) noise fields."""
    n, H, W = canvas.shape
    dev = canvas.device
    cmds, offset, verts, circles, colors = encode_commands(command_lists, field_base or [0] * n)
    f = torch.from_numpy(np.stack(fields).astype(np.float64)).to(dev) if len(fields) else None
    ws = _workspace(n, H, W, int(offset[-1]), len(verts), len(circles), dev, cache)
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_shapes_render(
            h.ptr, _lib.ptr(canvas), _lib.ptr(mean), n, H, W, cmds, offset.ctypes.data_as(ctypes.c_void_p),
            verts.ctypes.data_as(ctypes.c_void_p), len(verts), circles.ctypes.data_as(ctypes.c_void_p),
            colors.ctypes.data_as(ctypes.c_void_p), len(circles), _lib.ptr(f), 0 if f is None else f.shape[0], _lib.ptr(ws),
            ws.numel(), _lib.stream_ptr(dev)))
    return canvas


def finish(canvas, blur1, blur2, out_size, cache=None):
    """mp_shapes_finish: the Gaussian blurs (blur2[i] == 0: none) in place on canvas (n,H,W), then the INTER_LINEAR resize to
    out_size (h, w); returns (n,h,w) fp32 CUDA."""
    n, H, W = canvas.shape
    dev = canvas.device
    b1 = np.ascontiguousarray(blur1, np.int32)
    b2 = np.ascontiguousarray(blur2, np.int32)
    out = torch.empty((n, int(out_size[0]), int(out_size[1])), dtype=torch.float32, device=dev)
    ws = _workspace(n, H, W, 0, 0, 0, dev, cache)
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_shapes_finish(h.ptr, _lib.ptr(canvas), n, H, W, b1.ctypes.data_as(ctypes.c_void_p),
                                       b2.ctypes.data_as(ctypes.c_void_p), _lib.ptr(out), out.shape[1], out.shape[2],
                                       _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    return out


class SyntheticShapes(Dataset):
    default_config = {
        'length': 1000,
        'primitives': 'all',
        'on-the-fly': True,
        'hdf5-file': None,
        'generation_size': [960, 1280],
        'image_size': [240, 320],
        'keypoints_as_map': True,
        'generation': {
            'min_contrast': 0.1,
            'noise': 'host',
            'randu_seed': 0,
            'generate_background': {
                'min_kernel_size': 150, 'max_kernel_size': 500,
                'min_rad_ratio': 0.02, 'max_rad_ratio': 0.031},
            'draw_lines': {'nb_lines': 10},
            'draw_polygons': {'max_sides': 8},
            'draw_stripes': {'transform_params': (0.1, 0.1)},
            'draw_multiple_polygons': {'kernel_boundaries': (50, 100)}
        },
        'processing': {
            'blur_size': 21,
            'additional_ir_blur': True,
            'additional_ir_blur_size': 51,
        },
        'augmentation': {
            'photometric': {
                'enable': True,
                'primitives': 'all',
                'params': {},
                'random_order': True,
            },
            'homographic': {
                'enable': True,
                'params': {},
                'border_reflect': True,
                'valid_border_margin': 0,
                'mask_border': True,
            },
        }
    }

    all_primitives = [
        'draw_lines',
        'draw_polygon',
        'draw_multiple_polygons',
        'draw_ellipses',
        'draw_star',
        'draw_checkerboard',
        'draw_stripes',
        'draw_cube',
        'gaussian_noise'
    ]

    def __init__(self, config=None):
        # the reference's yaml carries a `preprocessing:` block, but the class reads `processing`: dict_update merges the
        # yaml key and nothing uses it.  Reproduced: no key is renamed here.
        self.config = dict_update(copy.deepcopy(self.default_config), config or {})
        self.primitives = parse_primitives(self.config['primitives'], self.all_primitives)
        noise = self.config['generation'].get('noise', 'host')
        if noise not in NOISE_MODES:
            raise ValueError("SyntheticShapes: generation.noise must be 'host' or 'device', got %r" % (noise,))
        self.noise = noise
        check_augmentation_config(self.config, 'SyntheticShapes')
        self.sync_count = 0          # device-to-host reads of a background mean (draw_checkerboard only)
        self.samples_drawn = 0       # gaussian_noise keys its field on this counter
        self._cache = {}
        if self.config['on-the-fly'] is False:
            try:
                with _open_store(self.config['hdf5-file']) as f:
                    self.memberslist = list(f.keys())
            except (IOError, OSError, TypeError) as e:
                print("Config is set to load data from hdf5 file (on-the-fly False),")
                print("but file {} not found or invalid.".format(self.config['hdf5-file']))
                raise e
            self.config['length'] = len(self.memberslist)

    # ---- plan (host) -------------------------------------------------------------------------------------------
    def draw_plan(self, background_mean):
        """The draws of one image in the reference's order: is_optical, the background, np.random.choice of the primitive,
        the primitive.  background_mean(plan) is called only by draw_checkerboard and returns the mean of the background
        the plan holds so far.  Returns (plan, is_optical, primitive)."""
        gen = self.config['generation']
        plan = draw_primitives.ShapePlan(self.config['generation_size'], self.noise)
        is_optical = bool(random.randint(0, 1))
        draw_primitives.plan_background(plan, **gen['generate_background'])
        primitive = str(np.random.choice(self.primitives))
        kwargs = dict(gen.get(primitive, {}))
        if primitive == 'draw_checkerboard':
            kwargs['background_mean'] = background_mean(plan)
        elif primitive == 'gaussian_noise':
            kwargs['randu_key'] = (int(gen.get('randu_seed', 0)) * 0x9E3779B97F4A7C15 + self.samples_drawn) % 2 ** 64
        self.samples_drawn += 1
        plan.keypoints = draw_primitives.PLANNERS[primitive](plan, min_contrast=gen['min_contrast'], **kwargs)
        return plan, is_optical, primitive

    def scale_keypoints(self, keypoints):
        """(x, y) plan keypoints to the reference's (y, x) in the final image (SyntheticShapes.py:129-149)."""
        keypoints = np.flip(np.asarray(keypoints).reshape(-1, 2), 1)
        if self.config['generation_size'] != self.config['image_size']:
            keypoints = (np.array(self.config['image_size']).astype(float) / np.array(self.config['generation_size'])
                         * keypoints).round().astype(int)
        return keypoints

    # ---- replay (device) ---------------------------------------------------------------------------------------
    def generate_batch(self, n, device=None, return_canvas=False):
        """n images from one set of launches: (images (n,h,w) fp32 CUDA, [keypoints (N,2) (y,x) int], [is_optical])."""
        dev = _lib.require_cuda(device)
        H, W = (int(v) for v in self.config['generation_size'])
        canvas = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        mean = torch.zeros((n,), dtype=torch.float64, device=dev)
        plans, flags, done = [], [], [0] * n

        def background_mean(plan):
            i = len(plans)                     # the image being planned: render what it has, alone, and read its mean
            render(canvas[i:i + 1], mean[i:i + 1], [plan.commands], plan.fields, cache=self._cache)
            done[i] = len(plan.commands)
            self.sync_count += 1
            return float(mean[i].item())
        for i in range(n):
            plan, is_optical, _ = self.draw_plan(background_mean)
            plans.append(plan)
            flags.append(is_optical)
        fields, base = [], []
        for plan, d in zip(plans, done):
            base.append(len(fields))
            if d == 0:
                fields.extend(plan.fields)
        render(canvas, mean, [p.commands[d:] for p, d in zip(plans, done)], fields, base, cache=self._cache)
        pre = canvas.clone() if return_canvas else None
        proc = self.config['processing']
        blur2 = [proc['additional_ir_blur_size'] if (not o and proc['additional_ir_blur']) else 0 for o in flags]
        images = finish(canvas, [proc['blur_size']] * n, blur2, self.config['image_size'], cache=self._cache)
        keypoints = [self.scale_keypoints(p.keypoints) for p in plans]
        if return_canvas:
            return images, keypoints, flags, pre
        return images, keypoints, flags

    def generate_synthetic_image(self, index=0, device=None):
        """(image (h,w) fp32 CUDA tensor, keypoints (N,2) (y,x) int array, is_optical)."""
        images, keypoints, flags = self.generate_batch(1, device)
        return images[0], keypoints[0], flags[0]

    def get_stored_image(self, index):
        """on-the-fly False: image / 255, points, is_optical True (SyntheticShapes.py:153-168)."""
        with _open_store(self.config['hdf5-file']) as f:
            sample = f[self.memberslist[index]]
            image = np.asarray(sample['image'][...], dtype=np.float32) / (2.0 ** 8 - 1)
            keypoints = np.asarray(sample['points'][...], dtype=np.float32)
        return torch.from_numpy(image).to(_lib.require_cuda()), keypoints, True

    def apply_augmentation(self, image, keypoints, is_optical):
        """SyntheticShapes.py:170-214 on a CUDA image: keypoint clamp, photometric then homographic augmentation, the
        keypoint map, the sample dictionary."""
        size = self.config['image_size']
        keypoints[keypoints[:, 0] >= size[0], 0] = size[0] - 1
        keypoints[keypoints[:, 1] >= size[1], 1] = size[1] - 1
        aug = self.config['augmentation']
        if aug['photometric']['enable']:
            image = augmentation.photometric_augmentation(image, **aug['photometric'])
        if aug['homographic']['enable']:
            image, keypoints, valid_mask = augmentation.homographic_augmentation(image, keypoints, **aug['homographic'])
            valid_mask = valid_mask.cpu().to(torch.bool)
        else:
            valid_mask = torch.from_numpy(augmentation.dummy_valid_mask(tuple(image.shape)).astype(bool))
        if self.config['keypoints_as_map']:
            keypoints = torch.from_numpy(generate_keypoint_map(keypoints, tuple(image.shape)))
        else:
            keypoints = torch.from_numpy(np.asarray(keypoints).astype(np.float32))
        return {'image': image.cpu().to(torch.float32)[None], 'keypoints': keypoints, 'valid_mask': valid_mask[None],
                'is_optical': torch.BoolTensor([is_optical])}

    def __getitem__(self, index):
        if self.config['on-the-fly']:
            im, kp, isopt = self.generate_synthetic_image(index)
        else:
            im, kp, isopt = self.get_stored_image(index)
        return self.apply_augmentation(im, kp, isopt)

    def returns_pair(self):
        return False

    def __len__(self):
        return self.config['length']
