"""Planners for the synthetic shapes (multipoint/utils/draw_primitives.py of the reference) -- no pixel work.

Each planner makes exactly the `random` / `np.random` calls of its reference function, in the reference's order, with the
same parameter defaults, rejection rules, host geometry and integer truncation, and appends draw commands to a ShapePlan;
the GPU replays the commands (multipoint_amd/csrc/shapes.hip).  Keypoints come from the plan alone.

A colour is a ColorSpec: `get_random_color(bg, c)` always consumes one random.random() and only its VALUE depends on the
image mean, so a command carries the raw draw `u` and the two colours it can resolve to; the device picks
`b if abs(u - mean) < min_contrast else a` against the mean it computed at the last 'mean' command.  Colours that do not
depend on the device (shape backgrounds, whose mean is int(np.mean(img)) == 0; the checkerboard, whose planner is given
the background mean) are literal.

Command kinds ('target' 0 is the image, 1 the private shape background of draw_multiple_polygons):
    threshold  key / host field index, t        canvas = field > t
    mean                                        frame mean of the image, kept on the device
    blobs      target, circles, colours (a, b)  filled circles, the highest index wins; base: fill colour or None
    box_blur   target, k                        cv2.blur(img, (k, k))
    line       p1, p2, thickness, colour        cv2.line
    convex     points, colour                   cv2.fillConvexPoly
    poly       points, colour | copy            cv2.fillPoly; copy: the pixels take the shape background instead
    ellipse    centre, axes, angle, colour      cv2.ellipse(..., -1)
    randu      key                              cv2.randu(img, 0, 1)
"""
import math
import random

import numpy as np

from .homographies import get_perspective_transform

__all__ = ['ColorSpec', 'ShapePlan', 'plan_background', 'plan_shape_background', 'PLANNERS', 'get_affine_transform',
           'keep_points_inside'] + ['draw_lines', 'draw_polygon', 'draw_multiple_polygons', 'draw_ellipses', 'draw_star',
                                    'draw_checkerboard', 'draw_stripes', 'draw_cube', 'gaussian_noise']


class ColorSpec:
    """call: index of the deciding get_random_color call in plan.color_draws (-1: literal); the colour is
    `b if abs(u - mean) < min_contrast else a`."""
    __slots__ = ('call', 'u', 'a', 'b', 'min_contrast')

    def __init__(self, call, u, a, b, min_contrast):
        self.call, self.u, self.a, self.b, self.min_contrast = call, u, a, b, min_contrast

    def resolve(self, mean):
        if self.call < 0:
            return self.a
        return self.b if abs(self.u - mean) < self.min_contrast else self.a

    def shifted(self, fn):
        """The spec of a colour derived from this one by `fn` (applied to both outcomes)."""
        return ColorSpec(self.call, self.u, fn(self.a), fn(self.b), self.min_contrast)


def literal(c):
    return ColorSpec(-1, 0.0, float(c), float(c), 0.0)


class ShapePlan:
    """The draws of one synthetic image: `commands` in the order they run, `color_draws` the raw random.random() of every
    get_random_color call in call order, `fields` the host noise fields (float64 (H, W)) in 'host' noise mode."""

    def __init__(self, shape, noise='host'):
        self.shape = (int(shape[0]), int(shape[1]))
        self.noise = noise
        self.commands = []
        self.color_draws = []
        self.fields = []
        self.keypoints = np.empty((0, 2), dtype=int)

    def add(self, kind, **kw):
        kw['kind'] = kind
        self.commands.append(kw)

    def random_color(self, min_contrast, background=None):
        """get_random_color: one random.random().  background None: resolved on the device against the current mean."""
        u = random.random()
        call = len(self.color_draws)
        self.color_draws.append(u)
        alt = (u + 0.5) % 1.0
        if background is None:
            return ColorSpec(call, u, u, alt, min_contrast)
        return literal(alt if abs(u - background) < min_contrast else u)


def _key():
    return int(np.random.randint(0, 2 ** 63, dtype=np.int64))


def get_affine_transform(src, dst):
    """cv2.getAffineTransform: the 2x3 matrix mapping three (x, y) points onto three others, solved in float64 on the
    float32-rounded points."""
    src = np.asarray(src, dtype=np.float32).astype(np.float64)
    dst = np.asarray(dst, dtype=np.float32).astype(np.float64)
    if src.shape != (3, 2) or dst.shape != (3, 2):
        raise ValueError('get_affine_transform needs two (3,2) point arrays')
    a = np.zeros((6, 6))
    b = np.zeros(6)
    for i in range(3):
        a[i, 0:3] = [src[i, 0], src[i, 1], 1.0]
        a[i + 3, 3:6] = [src[i, 0], src[i, 1], 1.0]
        b[i], b[i + 3] = dst[i, 0], dst[i, 1]
    return np.linalg.solve(a, b).reshape(2, 3)


def _ccw(a, b, c):
    return (c[..., 1] - a[..., 1]) * (b[..., 0] - a[..., 0]) > (b[..., 1] - a[..., 1]) * (c[..., 0] - a[..., 0])


def _intersect(a, b, c, d):
    """True if a segment a-b crosses a segment c-d (arrays of points that broadcast against each other)."""
    return bool(np.any((_ccw(a, c, d) != _ccw(b, c, d)) & (_ccw(a, b, c) != _ccw(a, b, d))))


def _overlap(center, rad, centers, rads):
    for i in range(len(rads)):
        if np.linalg.norm(center - centers[i]) + min(rad, rads[i]) < max(rad, rads[i]):
            return True
    return False


def _angle_between(v1, v2):
    v1_u = v1 / np.linalg.norm(v1)
    v2_u = v2 / np.linalg.norm(v2)
    return np.arccos(np.clip(np.dot(v1_u, v2_u), -1.0, 1.0))


def keep_points_inside(points, size):
    mask = (points[:, 0] >= 0) & (points[:, 0] < size[1]) & (points[:, 1] >= 0) & (points[:, 1] < size[0])
    return points[mask, :]


def _blob_command(plan, target, xs, ys, rads, us, min_contrast, background, base):
    """Circles with the raw colour draws `us`.  background None: colours (a, b) = (u, alternative), resolved on the device
    against the current mean; otherwise resolved here, a == b.  call0 is the first circle's index in plan.color_draws."""
    u = np.asarray(us, dtype=np.float64)
    alt = (u + 0.5) % 1.0
    if background is None:
        colors = np.stack([u, alt], axis=1)
    else:
        c = np.where(np.abs(u - background) < min_contrast, alt, u)
        colors = np.stack([c, c], axis=1)
    call0 = len(plan.color_draws)
    plan.color_draws.extend(us)
    plan.add('blobs', target=target, circles=np.stack([xs, ys, rads], axis=1).astype(np.int64), colors=colors,
             resolve=background is None, min_contrast=float(min_contrast), call0=call0, base=base)


def plan_shape_background(plan, background_color, min_contrast=0.13, nb_blobs=3000, kernel_boundaries=(50, 100)):
    """generate_shape_background into target 1.  background_color is int(np.mean(img)) == 0: every colour is literal.
    The reference alternates one random.random() (colour) and one np.random.randint(20) (radius) per blob: two
    generators, so each is drawn in one go here."""
    H, W = plan.shape
    base = plan.random_color(min_contrast, background_color)
    xs = np.random.randint(0, W, size=(nb_blobs, 1))[:, 0]
    ys = np.random.randint(0, H, size=(nb_blobs, 1))[:, 0]
    us = [random.random() for _ in range(nb_blobs)]
    rads = np.random.randint(20, size=nb_blobs)
    kernel_size = np.random.randint(kernel_boundaries[0], kernel_boundaries[1])
    _blob_command(plan, 1, xs, ys, rads, us, min_contrast, background_color, base)
    plan.add('box_blur', target=1, k=int(kernel_size))


def plan_background(plan, nb_blobs=100, min_rad_ratio=0.01, max_rad_ratio=0.05, min_kernel_size=50, max_kernel_size=300,
                    min_contrast=0.13):
    """generate_background: the thresholded noise field, the blobs against its mean, the box blur; then the mean of the
    finished background, which most primitives read."""
    H, W = plan.shape
    if plan.noise == 'host':
        plan.fields.append(np.random.rand(H, W))
        field = {'field': len(plan.fields) - 1, 'key': 0}
    else:
        field = {'field': -1, 'key': _key()}
    dim = max(H, W)
    plan.add('threshold', t=random.random(), **field)
    plan.add('mean')
    xs = np.random.randint(0, W, size=(nb_blobs, 1))[:, 0]
    ys = np.random.randint(0, H, size=(nb_blobs, 1))[:, 0]
    us, rads = [], []
    for _ in range(nb_blobs):
        us.append(random.random())
        rads.append(random.randint(int(dim * min_rad_ratio), int(dim * max_rad_ratio)))
    kernel_size = random.randint(min_kernel_size, max_kernel_size)
    _blob_command(plan, 0, xs, ys, np.array(rads, dtype=np.int64), us, min_contrast, None, None)
    plan.add('box_blur', target=0, k=int(kernel_size))
    plan.add('mean')


def draw_lines(plan, nb_lines=10, min_contrast=0.13):
    H, W = plan.shape
    num_lines = random.randint(1, nb_lines)
    segments = np.empty((0, 4), dtype=int)
    points = np.empty((0, 2), dtype=int)
    min_dim = min(H, W)
    for _i in range(num_lines):
        x1 = np.random.randint(W)
        y1 = np.random.randint(H)
        x2 = np.random.randint(W)
        y2 = np.random.randint(H)
        if _intersect(segments[:, 0:2], segments[:, 2:4], np.array([[x1, y1]]), np.array([[x2, y2]])):
            continue
        segments = np.concatenate([segments, np.array([[x1, y1, x2, y2]])], axis=0)
        plan.add('mean')
        col = plan.random_color(min_contrast)
        thickness = random.randint(int(math.ceil(min_dim * 0.01)), int(min_dim * 0.02))
        plan.add('line', p1=(int(x1), int(y1)), p2=(int(x2), int(y2)), thickness=int(thickness), color=col)
        points = np.concatenate([points, np.array([[x1, y1], [x2, y2]])], axis=0)
    return points


def _polygon_corners(x, y, rad, num_corners):
    """The corner sampling and the too-close / too-flat filters shared by draw_polygon and draw_multiple_polygons."""
    slices = np.linspace(0, 2 * math.pi, num_corners + 1)
    angles = [slices[i] + random.random() * (slices[i + 1] - slices[i]) for i in range(num_corners)]
    points = np.array([[int(x + max(random.random(), 0.4) * rad * math.cos(a)),
                        int(y + max(random.random(), 0.4) * rad * math.sin(a))] for a in angles])
    norms = [np.linalg.norm(points[(i - 1) % num_corners, :] - points[i, :]) for i in range(num_corners)]
    points = points[np.array(norms) > 0.01, :]
    num_corners = points.shape[0]
    corner_angles = [_angle_between(points[(i - 1) % num_corners, :] - points[i, :],
                                    points[(i + 1) % num_corners, :] - points[i, :]) for i in range(num_corners)]
    return points[np.array(corner_angles) < (2 * math.pi / 3), :]


def draw_polygon(plan, max_sides=8, min_contrast=0.13):
    H, W = plan.shape
    num_corners = random.randint(3, max_sides)
    min_dim = min(H, W)
    rad = max(random.random() * min_dim / 2, min_dim / 10)
    x = random.randint(int(rad), int(W - rad))
    y = random.randint(int(rad), int(H - rad))
    points = _polygon_corners(x, y, rad, num_corners)
    if points.shape[0] < 3:
        return draw_polygon(plan, max_sides)          # the reference's retry drops min_contrast back to its default
    col = plan.random_color(min_contrast)
    plan.add('poly', points=points.astype(np.int64), color=col, copy=False)
    return points


def draw_multiple_polygons(plan, max_sides=8, nb_polygons=30, **extra):
    H, W = plan.shape
    existing = np.empty((0, 4))
    centers, rads = [], []
    points = np.empty((0, 2), dtype=int)
    background_color = 0                              # int(np.mean(img)) of an image in [0, 1)
    for _i in range(nb_polygons):
        num_corners = random.randint(3, max_sides)
        min_dim = min(H, W)
        rad = max(random.random() * min_dim / 2, min_dim / 10)
        x = np.random.randint(rad, W - rad)
        y = np.random.randint(rad, H - rad)
        new_points = _polygon_corners(x, y, rad, num_corners)
        num_corners = new_points.shape[0]
        if num_corners < 3:
            continue
        new_segments = np.concatenate([new_points, np.roll(new_points, -1, axis=0)], axis=1).astype(np.float64)
        if _intersect(existing[:, None, 0:2], existing[:, None, 2:4], new_segments[None, :, 0:2],
                      new_segments[None, :, 2:4]) or _overlap(np.array([x, y]), rad, centers, rads):
            continue
        centers.append(np.array([x, y]))
        rads.append(rad)
        existing = np.concatenate([existing, new_segments], axis=0)
        plan_shape_background(plan, background_color, **extra)
        plan.add('poly', points=new_points.astype(np.int64), color=literal(1.0), copy=True)
        points = np.concatenate([points, new_points], axis=0)
    return points


def draw_ellipses(plan, nb_ellipses=20, min_contrast=0.13):
    H, W = plan.shape
    centers = np.empty((0, 2), dtype=int)
    rads = np.empty((0, 1), dtype=int)
    min_dim = min(H, W) / 4
    for _i in range(nb_ellipses):
        ax = int(max(random.random() * min_dim, min_dim / 5))
        ay = int(max(random.random() * min_dim, min_dim / 5))
        max_rad = max(ax, ay)
        x = random.randint(max_rad, W - max_rad)
        y = random.randint(max_rad, H - max_rad)
        new_center = np.array([[x, y]])
        diff = centers - new_center
        if np.any(max_rad > (np.sqrt(np.sum(diff * diff, axis=1)) - rads)):
            continue
        centers = np.concatenate([centers, new_center], axis=0)
        rads = np.concatenate([rads, np.array([[max_rad]])], axis=0)
        plan.add('mean')
        col = plan.random_color(min_contrast)
        angle = random.random() * 90
        plan.add('ellipse', center=(x, y), axes=(ax, ay), angle=int(round(angle)), color=col)     # cv::ellipse: cvRound
    return np.empty((0, 2), dtype=int)


def draw_star(plan, nb_branches=6, min_contrast=0.13):
    H, W = plan.shape
    num_branches = random.randint(3, nb_branches)
    min_dim = min(H, W)
    thickness = random.randint(int(math.ceil(min_dim * 0.01)), int(min_dim * 0.02))
    rad = max(random.random() * min_dim / 2, min_dim / 5)
    x = np.random.randint(rad, W - rad)
    y = np.random.randint(rad, H - rad)
    slices = np.linspace(0, 2 * math.pi, num_branches + 1)
    angles = [slices[i] + random.random() * (slices[i + 1] - slices[i]) for i in range(num_branches)]
    points = np.array([[int(x + max(random.random(), 0.3) * rad * math.cos(a)),
                        int(y + max(random.random(), 0.3) * rad * math.sin(a))] for a in angles])
    points = np.concatenate(([[x, y]], points), axis=0)
    for i in range(1, num_branches + 1):
        col = plan.random_color(min_contrast)
        plan.add('line', p1=(int(points[0][0]), int(points[0][1])), p2=(int(points[i][0]), int(points[i][1])),
                 thickness=int(thickness), color=col)
    return points


def _warp_grid(shape, points, transform_params):
    """The affine + perspective warp of draw_checkerboard / draw_stripes: one random.random() and two np.random.uniform
    (4, 2) draws; returns the warped integer points."""
    alpha_affine = np.max(shape) * (transform_params[0] + random.random() * transform_params[1])
    center_square = np.float16(shape) // 2
    square_size = min(shape) // 3
    pts1 = np.float32([center_square + square_size,
                       [center_square[0] + square_size, center_square[1] - square_size],
                       center_square - square_size,
                       [center_square[0] - square_size, center_square[1] + square_size]])
    pts2 = pts1 + np.random.uniform(-alpha_affine, alpha_affine, size=pts1.shape).astype(np.float32)
    affine_transform = get_affine_transform(pts1[:3], pts2[:3])
    pts2 = pts1 + np.random.uniform(-alpha_affine / 2, alpha_affine / 2, size=pts1.shape).astype(np.float32)
    perspective_transform = get_perspective_transform(pts1, pts2)
    n = points.shape[0]
    points = np.transpose(np.concatenate((points, np.ones((n, 1))), axis=1))
    warped_points = np.transpose(np.dot(affine_transform, points))
    cols = [np.add(np.sum(np.multiply(warped_points, perspective_transform[r, :2]), axis=1), perspective_transform[r, 2])
            for r in range(3)]
    warped = np.concatenate([np.divide(cols[0], cols[2])[:, None], np.divide(cols[1], cols[2])[:, None]], axis=1)
    return warped.astype(int)


def _different_color(plan, previous_colors, min_contrast, max_count=20):
    """get_different_color: a data-dependent number of random.random() draws against float16 neighbours."""
    color = random.random()
    count = 0
    while np.any(np.abs(previous_colors - color) < min_contrast) and count < max_count:
        count += 1
        color = random.random()
    return color


def _quad(wp, idx):
    return np.array([(wp[i, 0], wp[i, 1]) for i in idx], dtype=np.int64)


def draw_checkerboard(plan, max_rows=7, max_cols=7, transform_params=(0.05, 0.15), min_contrast=0.13,
                      background_mean=None):
    """The one planner that needs the background mean as a number: the first cell's resolved colour feeds
    get_different_color, whose loop consumes a data-dependent number of draws."""
    if background_mean is None:
        raise ValueError('draw_checkerboard: the planner needs background_mean (the mean of the rendered background)')
    H, W = plan.shape
    background_color = float(background_mean)
    rows = random.randint(3, max_rows)
    cols = random.randint(3, max_cols)
    s = min((W - 1) // cols, (H - 1) // rows)
    x_coord = np.tile(range(cols + 1), rows + 1).reshape(((rows + 1) * (cols + 1), 1))
    y_coord = np.repeat(range(rows + 1), cols + 1).reshape(((rows + 1) * (cols + 1), 1))
    points = s * np.concatenate([x_coord, y_coord], axis=1)
    min_dim = min(H, W)
    wp = _warp_grid((H, W), points, transform_params)
    colors = np.zeros((rows * cols,), np.float16)
    for i in range(rows):
        for j in range(cols):
            if i == 0 and j == 0:
                col = plan.random_color(min_contrast, background_color).a
            else:
                neighboring_colors = []
                if i != 0:
                    neighboring_colors.append(colors[(i - 1) * cols + j])
                if j != 0:
                    neighboring_colors.append(colors[i * cols + j - 1])
                col = _different_color(plan, np.array(neighboring_colors), min_contrast)
            colors[i * cols + j] = col
            c = cols + 1
            plan.add('convex', points=_quad(wp, [i * c + j, i * c + j + 1, (i + 1) * c + j + 1, (i + 1) * c + j]),
                     color=literal(col))
    nb_rows = random.randint(2, rows + 2)
    nb_cols = random.randint(2, cols + 2)
    thickness = random.randint(int(math.ceil(min_dim * 0.01)), int(min_dim * 0.015))
    for _i in range(nb_rows):
        row_idx = np.random.randint(rows + 1)
        col_idx1 = np.random.randint(cols + 1)
        col_idx2 = np.random.randint(cols + 1)
        col = plan.random_color(min_contrast, background_color)
        a, b = row_idx * (cols + 1) + col_idx1, row_idx * (cols + 1) + col_idx2
        plan.add('line', p1=(int(wp[a, 0]), int(wp[a, 1])), p2=(int(wp[b, 0]), int(wp[b, 1])), thickness=int(thickness),
                 color=col)
    for _i in range(nb_cols):
        col_idx = np.random.randint(cols + 1)
        row_idx1 = np.random.randint(rows + 1)
        row_idx2 = np.random.randint(rows + 1)
        col = plan.random_color(min_contrast, background_color)
        a, b = row_idx1 * (cols + 1) + col_idx, row_idx2 * (cols + 1) + col_idx
        plan.add('line', p1=(int(wp[a, 0]), int(wp[a, 1])), p2=(int(wp[b, 0]), int(wp[b, 1])), thickness=int(thickness),
                 color=col)
    return keep_points_inside(wp, (H, W))


def draw_stripes(plan, max_nb_cols=13, min_width_ratio=0.04, transform_params=(0.05, 0.15), min_contrast=0.13):
    H, W = plan.shape
    board_size = (int(H * (1 + random.random())), int(W * (1 + random.random())))
    col = random.randint(5, max_nb_cols)
    cols = np.concatenate([board_size[1] * np.random.rand(col - 1), np.array([0, board_size[1] - 1])], axis=0)
    cols = np.unique(cols.astype(int))
    min_dim = min(H, W)
    min_width = min_dim * min_width_ratio
    cols = cols[(np.concatenate([cols[1:], np.array([board_size[1] + min_width])], axis=0) - cols) >= min_width]
    col = cols.shape[0] - 1
    cols = np.reshape(cols, (col + 1, 1))
    cols1 = np.concatenate([cols, np.zeros((col + 1, 1), np.int32)], axis=1)
    cols2 = np.concatenate([cols, (board_size[0] - 1) * np.ones((col + 1, 1), np.int32)], axis=1)
    points = np.concatenate([cols1, cols2], axis=0)
    wp = _warp_grid((H, W), points, transform_params)
    color = plan.random_color(min_contrast)
    for i in range(col):
        r = random.random()
        color = color.shifted(lambda c, r=r: (c + 0.4 + r * 0.2) % 1.0)
        plan.add('convex', points=_quad(wp, [i, i + 1, i + col + 2, i + col + 1]), color=color)
    nb_rows = random.randint(2, 5)
    nb_cols = random.randint(2, col + 2)
    thickness = random.randint(int(math.ceil(min_dim * 0.01)), int(min_dim * 0.015))
    for _i in range(nb_rows):
        row_idx = random.choice([0, col + 1])
        col_idx1 = np.random.randint(col + 1)
        col_idx2 = np.random.randint(col + 1)
        c = plan.random_color(min_contrast)
        a, b = row_idx + col_idx1, row_idx + col_idx2
        plan.add('line', p1=(int(wp[a, 0]), int(wp[a, 1])), p2=(int(wp[b, 0]), int(wp[b, 1])), thickness=int(thickness),
                 color=c)
    for _i in range(nb_cols):
        col_idx = np.random.randint(col + 1)
        c = plan.random_color(min_contrast)
        a, b = col_idx, col_idx + col + 1
        plan.add('line', p1=(int(wp[a, 0]), int(wp[a, 1])), p2=(int(wp[b, 0]), int(wp[b, 1])), thickness=int(thickness),
                 color=c)
    return keep_points_inside(wp, (H, W))


def draw_cube(plan, min_size_ratio=0.2, min_angle_rot=math.pi / 10, scale_interval=(0.4, 0.6), trans_interval=(0.5, 0.2),
              min_contrast=0.13):
    H, W = plan.shape
    min_dim = min(H, W)
    min_side = min_dim * min_size_ratio
    lx = min_side + random.random() * 2 * min_dim / 3
    ly = min_side + random.random() * 2 * min_dim / 3
    lz = min_side + random.random() * 2 * min_dim / 3
    cube = np.array([[0, 0, 0], [lx, 0, 0], [0, ly, 0], [lx, ly, 0], [0, 0, lz], [lx, 0, lz], [0, ly, lz], [lx, ly, lz]])
    rot_angles = np.random.rand(3) * 3 * math.pi / 10. + math.pi / 10.
    c, s = [math.cos(a) for a in rot_angles], [math.sin(a) for a in rot_angles]
    rotation_1 = np.array([[c[0], -s[0], 0], [s[0], c[0], 0], [0, 0, 1]])
    rotation_2 = np.array([[1, 0, 0], [0, c[1], -s[1]], [0, s[1], c[1]]])
    rotation_3 = np.array([[c[2], 0, -s[2]], [0, 1, 0], [s[2], 0, c[2]]])
    scaling = np.array([[scale_interval[0] + random.random() * scale_interval[1], 0, 0],
                        [0, scale_interval[0] + random.random() * scale_interval[1], 0],
                        [0, 0, scale_interval[0] + random.random() * scale_interval[1]]])
    # the reference hands random.randint these float bounds: it raises unless they are whole numbers
    trans = np.array([W * trans_interval[0] + random.randint(-W * trans_interval[1], W * trans_interval[1]),
                      H * trans_interval[0] + random.randint(-H * trans_interval[1], H * trans_interval[1]), 0])
    cube = trans + np.transpose(np.dot(scaling, np.dot(rotation_1, np.dot(rotation_2, np.dot(rotation_3,
                                                                                           np.transpose(cube))))))
    cube = cube[:, :2].astype(int)
    points = cube[1:, :]
    faces = np.array([[7, 3, 1, 5], [7, 5, 4, 6], [7, 6, 2, 3]])
    col_face = plan.random_color(min_contrast)
    for i in [0, 1, 2]:
        plan.add('poly', points=cube[faces[i]].astype(np.int64), color=col_face, copy=False)
    thickness = random.randint(int(math.ceil(min_dim * 0.003)), int(min_dim * 0.015))
    for i in [0, 1, 2]:
        for j in [0, 1, 2, 3]:
            r = random.random()
            a, b = cube[faces[i][j]], cube[faces[i][(j + 1) % 4]]
            plan.add('line', p1=(int(a[0]), int(a[1])), p2=(int(b[0]), int(b[1])), thickness=int(thickness),
                     color=col_face.shifted(lambda v, r=r: (v + 0.25 + r * 0.5) % 1.0))
    return keep_points_inside(points, (H, W))


def gaussian_noise(plan, min_contrast=0.0, randu_key=0):
    """cv2.randu draws from OpenCV's own generator, which the reference never seeds: no `random` / `np.random` draw."""
    plan.add('randu', key=int(randu_key))
    return np.empty((0, 2), dtype=int)


PLANNERS = {f.__name__: f for f in (draw_lines, draw_polygon, draw_multiple_polygons, draw_ellipses, draw_star,
                                    draw_checkerboard, draw_stripes, draw_cube, gaussian_noise)}
