"""Planted pairs for the Fourier-Mellin registration tests: a scene of filled rectangles and ellipses on a canvas three times the
frame, an optical cut of 96 x 128 and a thermal frame 1 - cut^0.7 (contrast inverted and remapped) under a planted similarity
plus shift, at 96 x 128 or 72 x 96.  The scene is evaluated analytically at every sample (4 x 4 supersampling), so no frame is
resampled from another."""
import functools
import math

import numpy as np

OPTICAL_HW = (96, 128)
CANVAS = 3
SHAPES = 40
SUPER = 4

# name: (scene seed, thermal (H, W), angle in degrees, scale, (dx, dy) shift of the thermal frame in thermal pixels).  The planted
# transform maps the optical centre onto the thermal centre plus the shift; angles within +-10 degrees, scales in [0.75, 1.3],
# shifts <= 20 px.
CASES = {
    'same_size_rot': (105, (96, 128), 5.0, 1.0, (6.0, -4.0)),
    'same_size_scale_up': (111, (96, 128), -3.0, 1.2, (-12.5, 7.25)),
    'same_size_scale_down': (116, (96, 128), 8.0, 0.85, (15.0, 10.0)),
    'small_thermal_rig': (119, (72, 96), 2.0, 0.75, (3.0, -2.0)),
    'small_thermal_rot': (123, (72, 96), -7.0, 0.8, (-8.0, 5.5)),
    'small_thermal_far': (128, (72, 96), 10.0, 0.9, (14.0, -12.0)),
    'same_size_far_shift': (144, (96, 128), -9.0, 1.3, (20.0, -18.0)),
}
# one group of four pairs (four scenes) that share one transform
GROUP = dict(seeds=(146, 148, 151, 152), thermal_hw=(72, 96), angle=4.0, scale=0.78, shift=(-6.0, 9.0))
# six pairs that share the group's transform, written as PNG files for the command-line test (the group's four scenes and two more)
CLI_SEEDS = GROUP['seeds'] + (147, 149)
# three groups with three different planted shifts (the group indexing of the pooled path): sizes 2, 1, 3
SHIFT_GROUPS = dict(sizes=(2, 1, 3), seeds=(153, 155, 160, 170, 175, 176), thermal_hw=(72, 96), angle=-4.0, scale=0.8,
                    shifts=((10.0, 0.0), (-9.0, 6.0), (2.0, -11.0)))


def planted_transform(thermal_hw, angle_deg, scale, shift):
    """3x3 float64 optical pixel -> thermal pixel: q = s R(angle) (p - Co) + Ct + shift, R = [[cos, -sin], [sin, cos]]."""
    Ho, Wo = OPTICAL_HW
    Ht, Wt = thermal_hw
    a = math.radians(angle_deg)
    A = scale * np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
    co = np.array([(Wo - 1) / 2.0, (Ho - 1) / 2.0])
    ct = np.array([(Wt - 1) / 2.0, (Ht - 1) / 2.0])
    T = np.eye(3)
    T[:2, :2] = A
    T[:2, 2] = ct + np.asarray(shift, np.float64) - A @ co
    return T


def _scene(seed):
    """Shape list of one scene in canvas coordinates: (kind, cx, cy, half width, half height, rotation, value)."""
    rng = np.random.RandomState(seed)
    Hc, Wc = OPTICAL_HW[0] * CANVAS, OPTICAL_HW[1] * CANVAS
    shapes = []
    for _ in range(SHAPES):
        shapes.append((int(rng.randint(2)), rng.uniform(0, Wc), rng.uniform(0, Hc), rng.uniform(6, 40), rng.uniform(6, 40),
                       rng.uniform(0, math.pi), rng.uniform(0.05, 1.0)))
    return float(rng.uniform(0.2, 0.6)), shapes


def _evaluate(scene, x, y):
    """The scene's value at canvas coordinates (arrays): the background, then every shape painted over it in list order."""
    bg, shapes = scene
    v = np.full(x.shape, bg)
    for kind, cx, cy, a, b, rot, val in shapes:
        c, s = math.cos(rot), math.sin(rot)
        u = ((x - cx) * c + (y - cy) * s) / a
        w = (-(x - cx) * s + (y - cy) * c) / b
        inside = (np.maximum(np.abs(u), np.abs(w)) <= 1.0) if kind == 0 else (u * u + w * w <= 1.0)
        v = np.where(inside, val, v)
    return v


def _render(scene, hw, to_optical):
    """[H,W] float64: every pixel the mean of SUPER x SUPER samples, each mapped to optical pixel coordinates by the 3x3
    `to_optical` and from there to the canvas (the cut is the canvas's middle third)."""
    H, W = hw
    sub = (np.arange(SUPER) + 0.5) / SUPER - 0.5
    ys = (np.arange(H)[:, None] + sub[None, :]).reshape(-1)
    xs = (np.arange(W)[:, None] + sub[None, :]).reshape(-1)
    X, Y = np.meshgrid(xs, ys)
    px = to_optical[0, 0] * X + to_optical[0, 1] * Y + to_optical[0, 2]
    py = to_optical[1, 0] * X + to_optical[1, 1] * Y + to_optical[1, 2]
    v = _evaluate(scene, px + OPTICAL_HW[1], py + OPTICAL_HW[0])
    return v.reshape(H, SUPER, W, SUPER).mean(axis=(1, 3))


@functools.lru_cache(maxsize=None)
def make_pair(seed, thermal_hw, angle_deg, scale, shift):
    """(optical float32 [96,128], thermal float32 [Ht,Wt], T 3x3 float64 optical -> thermal)."""
    scene = _scene(seed)
    T = planted_transform(thermal_hw, angle_deg, scale, shift)
    optical = _render(scene, OPTICAL_HW, np.eye(3))
    thermal = 1.0 - _render(scene, thermal_hw, np.linalg.inv(T)) ** 0.7
    return optical.astype(np.float32), thermal.astype(np.float32), T


def case(name):
    seed, thw, ang, sc, sh = CASES[name]
    return make_pair(seed, thw, ang, sc, sh)


def group_case():
    """(optical [4,96,128], thermal [4,72,96], T): four scenes, one transform."""
    pairs = [make_pair(s, GROUP['thermal_hw'], GROUP['angle'], GROUP['scale'], GROUP['shift']) for s in GROUP['seeds']]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), pairs[0][2]


def cli_pairs():
    """(optical uint8 [6,96,128], thermal uint16 [6,72,96], T): the frames as 8- and 16-bit files hold them."""
    pairs = [make_pair(s, GROUP['thermal_hw'], GROUP['angle'], GROUP['scale'], GROUP['shift']) for s in CLI_SEEDS]
    optical = np.stack([np.rint(p[0].astype(np.float64) * 255.0) for p in pairs]).astype(np.uint8)
    thermal = np.stack([np.rint(p[1].astype(np.float64) * 65535.0) for p in pairs]).astype(np.uint16)
    return optical, thermal, pairs[0][2]


def shift_groups_case():
    """(optical [6,96,128], thermal [6,72,96], group ids [6], T [3,3,3]): three groups with three planted shifts."""
    cfg = SHIFT_GROUPS
    gid = np.repeat(np.arange(len(cfg['sizes'])), cfg['sizes'])
    pairs = [make_pair(s, cfg['thermal_hw'], cfg['angle'], cfg['scale'], cfg['shifts'][g]) for s, g in zip(cfg['seeds'], gid)]
    T = np.stack([planted_transform(cfg['thermal_hw'], cfg['angle'], cfg['scale'], sh) for sh in cfg['shifts']])
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), gid, T


def corner_error(T, T_true, hw=OPTICAL_HW):
    """Largest distance, in thermal pixels, between the images of the four optical corners under T and under T_true."""
    H, W = hw
    c = np.array([[0, 0, 1], [W - 1, 0, 1], [0, H - 1, 1], [W - 1, H - 1, 1]], np.float64).T
    a, b = T @ c, T_true @ c
    return float(np.max(np.hypot(*(a[:2] / a[2] - b[:2] / b[2]))))
