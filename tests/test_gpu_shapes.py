"""SyntheticShapes on the GPU (multipoint_amd/csrc/shapes.hip) against the fixture the reference wrote
(tests/golden/synthetic_shapes.npz) and against the OpenCV restatement (tests/shapes_restatement.py).

Canvas tolerance.  The reference draws on float64 and the kernels on fp32 canvases: a colour is rounded to fp32 when it is
written (relative 2^-24), the box blur rounds its double sum to fp32 (2^-24) and the fixture stores the reference canvas
as fp32 (2^-24).  Three roundings of values below 1 stay under 2^-22; a pixel rasterised on the wrong side of an edge shows
the other colour, which min_contrast keeps at least 0.1 away.  No pixel may differ by more.

Final-image bound.  Measured on an MI355X per case: the largest difference to the fixture image is
1.79e-07, so the bound is 4 x 1.79e-07 rounded up to one significant digit = 8e-07 (1e-5 is what
test_gpu_photometric.py holds the other fp32 restatements of cv2 filters to; this one is tighter)."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shapes_cases as C  # noqa: E402
import shapes_restatement as S  # noqa: E402

from multipoint_amd.datasets import augmentation  # noqa: E402
from multipoint_amd.datasets import synthetic_shapes as SS  # noqa: E402
from multipoint_amd.datasets.synthetic_shapes import SyntheticShapes  # noqa: E402
from multipoint_amd.utils.draw_primitives import ColorSpec, literal  # noqa: E402

pytestmark = pytest.mark.gpu

CANVAS_TOL = 2.0 ** -22
IMAGE_BOUND = 8e-7
IMAGE_CASES = [n for n in C.CASE_NAMES if 'gaussian_noise' not in n]      # cv2.randu's field is the generator's own
CANVAS_CASES = [n for n in IMAGE_CASES if n.startswith('a_')]


def seed_case(name):
    seed = int(C.case(name)['setup'][0])
    random.seed(seed)
    np.random.seed(seed + 7)


_generated = {}


def generated(name):
    """One generation per fixture case, shared by the tests that look at it."""
    if name not in _generated:
        ds = SyntheticShapes(C.case_config(name))
        seed_case(name)
        images, keypoints, flags, canvas = ds.generate_batch(1, return_canvas=True)
        _generated[name] = (images[0].cpu().numpy(), keypoints[0], flags[0], canvas[0].cpu().numpy(), ds.sync_count)
    return _generated[name]


@pytest.mark.parametrize('name', CANVAS_CASES)
def test_canvas_matches_the_reference_at_every_pixel(name):
    canvas = generated(name)[3]
    want = C.case(name)['canvas']
    diff = np.abs(canvas.astype(np.float64) - want.astype(np.float64))
    print('%s canvas: max difference %.3g, pixels over 2^-22: %d' % (name, diff.max(), int((diff > CANVAS_TOL).sum())))
    assert int((diff > CANVAS_TOL).sum()) == 0


@pytest.mark.parametrize('name', IMAGE_CASES)
def test_final_image_matches_the_reference(name):
    image = generated(name)[0]
    want = C.case(name)['image']
    assert image.shape == want.shape and image.dtype == np.float32
    diff = float(np.abs(image.astype(np.float64) - want.astype(np.float64)).max())
    print('%s image: max difference %.3g' % (name, diff))
    assert diff <= IMAGE_BOUND


@pytest.mark.parametrize('name', C.CASE_NAMES)
def test_keypoints_and_modality_are_exact(name):
    _, keypoints, is_optical, _, syncs = generated(name)
    case = C.case(name)
    assert np.array_equal(keypoints, case['keypoints']) and is_optical == bool(case['setup'][8])
    assert syncs == (1 if 'checkerboard' in name else 0)      # only the checkerboard reads a mean back


# ---- raster edge cases against the restatement, through the thin Python entry ---------------------------------------
def run(commands, H, W, fields=()):
    canvas = torch.zeros((1, H, W), dtype=torch.float32, device='cuda')
    mean = torch.zeros((1,), dtype=torch.float64, device='cuda')
    SS.render(canvas, mean, [commands], fields)
    return canvas[0].cpu().numpy(), float(mean[0].item())


def blobs(circles, colors, base=None, target=0):
    colors = np.asarray(colors, np.float64)
    return {'kind': 'blobs', 'target': target, 'circles': np.asarray(circles, np.int64).reshape(-1, 3),
            'colors': np.stack([colors, colors], axis=1), 'resolve': False, 'min_contrast': 0.0, 'call0': 0,
            'base': None if base is None else literal(base)}


def check(commands, H, W):
    got, _ = run(commands, H, W)
    want, _ = C.replay(commands, H, W)
    assert np.array_equal(got, want), 'pixels differ: %d' % int((got != want).sum())
    return got


def test_circles_on_corners_beyond_the_frame_and_small_radii():
    H, W = 45, 61
    for r in (0, 1, 39):
        for cx, cy in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W + 5, H // 2), (-7, -3), (W // 2, H + 38),
                       (W + 40, H + 40)):
            got = check([blobs([[cx, cy, r]], [0.75])], H, W)
            if r == 0:
                assert got.sum() == (0.75 if 0 <= cx < W and 0 <= cy < H else 0)


def test_overlapping_circles_in_both_orders():
    a, b = [20, 20, 9], [26, 23, 7]
    first = check([blobs([a, b], [0.25, 0.5])], 45, 61)
    second = check([blobs([b, a], [0.5, 0.25])], 45, 61)
    assert first[22, 24] == 0.5 and second[22, 24] == 0.25 and not np.array_equal(first, second)


def test_three_thousand_blobs():
    rng = np.random.default_rng(5)
    H, W = 32, 40
    circles = np.stack([rng.integers(0, W, 3000), rng.integers(0, H, 3000), rng.integers(0, 20, 3000)], axis=1)
    colors = rng.random(3000)
    check([blobs(circles, colors, base=0.125)], H, W)        # every 16 x 16 tile lists far more than a fixed capacity
    circles[:, 0], circles[:, 1] = 17, 13
    got = check([blobs(circles, colors)], H, W)              # all at one point: the last covering circle wins
    assert got[13, 17] == np.float32(colors[-1])


def test_lines():
    H, W = 45, 61
    ends = [((-20, 10), (90, 30)), ((-5, -9), (30, 60)), ((70, 50), (12, -30)),       # both ends outside
            ((10, 10), (80, 20)), ((-15, 40), (30, 5)),                               # one end outside
            ((25, 17), (25, 17)), ((3, 4), (50, 41)), ((50, 4), (3, 41)), ((7, 40), (7, 2)), ((2, 9), (58, 9))]
    for p1, p2 in ends:
        for t in range(1, 7):
            check([{'kind': 'line', 'p1': p1, 'p2': p2, 'thickness': t, 'color': literal(0.5)}], H, W)
    assert run([{'kind': 'line', 'p1': (-9, -9), 'p2': (-2, -30), 'thickness': 1, 'color': literal(0.5)}], H, W)[0].sum() == 0


def test_polygons():
    H, W = 45, 61
    shapes = [[[-10, -6], [30, 2], [44, 30], [8, 50]],                # negative vertices, leaves the frame
              [[5, 5], [55, 8], [50, 40], [9, 38]],
              [[-40, -40], [-5, -30], [-12, -3]],                      # wholly outside
              [[4, 4], [20, 20], [36, 36]],                            # degenerate: collinear
              [[10, 3], [50, 3], [50, 3], [30, 3]],                    # degenerate: one row
              [[70, 10], [40, 60], [20, -10]]]
    for pts in shapes:
        for kind in ('convex', 'poly'):
            check([{'kind': kind, 'points': np.array(pts), 'color': literal(0.625), 'copy': False}], H, W)
    star = [[30, 2], [36, 40], [5, 14], [56, 14], [22, 40]]           # self-intersecting: the even-odd rule
    concave = [[5, 5], [55, 5], [55, 40], [30, 12], [5, 40]]
    for pts in (star, concave, [[-20, 30], [30, -20], [80, 30], [30, 70], [30, 20]]):
        check([{'kind': 'poly', 'points': np.array(pts), 'color': literal(0.625), 'copy': False}], H, W)
    for el in ((30, 20, 12, 7, 33), (2, 2, 9, 3, 80), (70, 50, 15, 15, 0), (30, 20, 1, 1, 10), (30, 20, 0, 0, 0)):
        check([{'kind': 'ellipse', 'center': el[:2], 'axes': el[2:4], 'angle': el[4], 'color': literal(0.375)}], H, W)


def test_masked_copy_and_device_colour_resolve():
    H, W = 45, 61
    rng = np.random.default_rng(9)
    circles = np.stack([rng.integers(0, W, 200), rng.integers(0, H, 200), rng.integers(0, 12, 200)], axis=1)
    commands = [blobs([[30, 20, 15]], [0.5]), {'kind': 'mean'},
                blobs(circles, rng.random(200), base=0.25, target=1), {'kind': 'box_blur', 'target': 1, 'k': 6},
                {'kind': 'poly', 'points': np.array([[3, 3], [50, 9], [28, 40]]), 'color': literal(1.0), 'copy': True}]
    got, _ = run(commands, H, W)
    want, _ = C.replay(commands, H, W)
    assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -23
    # a colour resolved against the device mean: |u - mean| below min_contrast takes the alternative
    field = rng.random((H, W))
    for u in (0.3, 0.9):
        commands = [{'kind': 'threshold', 'field': 0, 'key': 0, 't': 0.7}, {'kind': 'mean'},
                    {'kind': 'line', 'p1': (2, 2), 'p2': (40, 30), 'thickness': 3, 'color': ColorSpec(0, u, u, 0.0625, 0.13)}]
        got, mean = run(commands, H, W, [field])
        want, want_mean = C.replay(commands, H, W, [field])
        assert abs(mean - want_mean) < 1e-12 and np.array_equal(got, want)
        assert got[16, 21] == np.float32(0.0625 if abs(u - mean) < 0.13 else u)


@pytest.mark.parametrize('k', [1, 2, 7, 36, 37, 80, 200])
def test_box_blur(k):
    H, W = 37, 53
    field = np.random.default_rng(k).random((H, W))
    commands = [{'kind': 'threshold', 'field': 0, 'key': 0, 't': 0.5}, blobs([[20, 15, 9], [40, 30, 5]], [0.3, 0.8]),
                {'kind': 'box_blur', 'target': 0, 'k': k}]
    got, _ = run(commands, H, W, [field])
    want, _ = C.replay(commands, H, W, [field])
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -23       # one rounding to fp32


@pytest.mark.parametrize('shape', [((96, 128), (48, 64)), ((90, 120), (60, 80)), ((37, 53), (37, 53))])
def test_resize(shape):
    (H, W), (h, w) = shape
    x = np.random.default_rng(3).random((2, H, W), dtype=np.float32)
    out = SS.finish(torch.from_numpy(x).cuda(), [0, 0], [0, 0], (h, w)).cpu().numpy()
    for i in range(2):
        want = S.resize(x[i].astype(np.float64), (w, h))
        assert np.abs(out[i] - want).max() <= 2.0 ** -22              # at most eight half-ulp fp32 roundings of values below 1


def test_gaussian_51_taps_on_a_frame_smaller_than_the_radius():
    H, W = 37, 53
    x = np.random.default_rng(4).random((2, H, W), dtype=np.float32)
    out = SS.finish(torch.from_numpy(x).cuda(), [51, 5], [0, 51], (H, W)).cpu().numpy()
    want0 = S.gaussian_blur64(x[0], 51)
    want1 = S.gaussian_blur64(S.gaussian_blur64(x[1], 5), 51)
    assert np.abs(out[0] - want0).max() <= 1e-5 and np.abs(out[1] - want1).max() <= 1e-5


def test_device_noise_is_reproducible_and_uniform():
    cfg = C.case_config('a_draw_polygon')
    cfg['generation']['noise'] = 'device'
    runs = []
    for _ in range(2):
        ds = SyntheticShapes(cfg)
        random.seed(11)
        np.random.seed(12)
        runs.append(ds.generate_batch(2)[0].cpu().numpy())
    assert np.array_equal(runs[0], runs[1])
    H, W, t = 96, 128, 0.3
    got, mean = run([{'kind': 'threshold', 'field': -1, 'key': 12345, 't': t}, {'kind': 'mean'}], H, W)
    assert set(np.unique(got)) == {0.0, 1.0} and mean == got.mean(dtype=np.float64)
    assert abs(mean - (1 - t)) <= 5 * np.sqrt(t * (1 - t) / (H * W))
    u, _ = run([{'kind': 'randu', 'key': 777}], H, W)
    n = H * W
    assert 0 <= u.min() and u.max() <= 1
    assert abs(u.mean(dtype=np.float64) - 0.5) <= 5 * np.sqrt(1 / 12 / n)
    assert abs(u.var(dtype=np.float64) - 1 / 12) <= 5 * np.sqrt(1 / 180 / n)      # Var((U - 1/2)^2) = 1/180
    other, _ = run([{'kind': 'randu', 'key': 778}], H, W)
    assert not np.array_equal(u, other)


def test_batch_equals_single_images():
    cfg = C.case_config('a_draw_lines')
    cfg['primitives'] = 'all'
    cfg['generation']['draw_cube'] = {'trans_interval': (0.5, 0.25)}
    ds = SyntheticShapes(cfg)
    random.seed(21)
    np.random.seed(22)
    images, keypoints, flags = ds.generate_batch(4)
    ds = SyntheticShapes(cfg)
    random.seed(21)
    np.random.seed(22)
    for i in range(4):
        image, kp, flag = ds.generate_synthetic_image(i)
        assert torch.equal(image, images[i]) and np.array_equal(kp, keypoints[i]) and flag == flags[i]


def test_dataset_sample():
    cfg = C.case_config('a_draw_star')
    cfg['primitives'] = ['draw_star', 'draw_polygon', 'draw_lines']
    cfg['augmentation'] = {'photometric': {'enable': True, 'noise': 'device', 'primitives': 'all', 'params': {},
                                           'random_order': True},
                           'homographic': {'enable': True, 'params': {}, 'border_reflect': True, 'valid_border_margin': 0,
                                           'mask_border': True}}
    ds = SyntheticShapes(cfg)
    random.seed(31)
    np.random.seed(32)
    sample = ds[0]
    assert ds.sync_count == 0
    assert sample['image'].shape == (1, 48, 64) and sample['image'].dtype == torch.float32
    assert sample['keypoints'].shape == (48, 64) and sample['keypoints'].dtype == torch.bool
    assert sample['valid_mask'].shape == (1, 48, 64) and sample['valid_mask'].dtype == torch.bool
    assert sample['is_optical'].shape == (1,) and sample['is_optical'].dtype == torch.bool
    # the same generator state, augmented by hand
    ds = SyntheticShapes(cfg)
    random.seed(31)
    np.random.seed(32)
    image, keypoints, is_optical = ds.generate_synthetic_image(0)
    keypoints[keypoints[:, 0] >= 48, 0] = 47
    keypoints[keypoints[:, 1] >= 64, 1] = 63
    image = augmentation.photometric_augmentation(image, **ds.config['augmentation']['photometric'])
    image, keypoints, mask = augmentation.homographic_augmentation(image, keypoints, **ds.config['augmentation']['homographic'])
    assert torch.equal(sample['image'][0], image.cpu()) and torch.equal(sample['valid_mask'][0], mask.cpu().bool())
    assert bool(sample['is_optical'][0]) == is_optical
    kmap = np.zeros((48, 64), bool)
    kmap[keypoints[:, 0], keypoints[:, 1]] = True
    assert np.array_equal(sample['keypoints'].numpy(), kmap)
    cfg['keypoints_as_map'] = False
    ds = SyntheticShapes(cfg)
    random.seed(31)
    np.random.seed(32)
    listed = ds[0]['keypoints']
    assert listed.dtype == torch.float32 and np.array_equal(listed.numpy(), keypoints.astype(np.float32))


def test_stored_samples(tmp_path):
    rng = np.random.default_rng(6)
    store = {}
    for i in range(3):
        store['s%d/image' % i] = rng.integers(0, 256, (48, 64)).astype(np.uint8)
        store['s%d/points' % i] = np.stack([rng.integers(0, 48, 5), rng.integers(0, 64, 5)], axis=1).astype(np.float64)
    path = str(tmp_path / 'shapes.npz')
    np.savez(path, **store)
    cfg = {'on-the-fly': False, 'hdf5-file': path, 'image_size': [48, 64],
           'augmentation': {'photometric': {'enable': False}, 'homographic': {'enable': False}}}
    ds = SyntheticShapes(cfg)
    assert len(ds) == 3
    sample = ds[1]
    assert torch.equal(sample['image'][0], torch.from_numpy(store['s1/image'].astype(np.float32) / 255.0))
    assert bool(sample['is_optical'][0]) and bool(sample['valid_mask'].all())
    want = np.zeros((48, 64), bool)
    want[store['s1/points'][:, 0].astype(int), store['s1/points'][:, 1].astype(int)] = True
    assert np.array_equal(sample['keypoints'].numpy(), want)
    with pytest.raises((IOError, OSError)):
        SyntheticShapes(dict(cfg, **{'hdf5-file': str(tmp_path / 'missing.npz')}))


def test_the_entry_point_refuses_what_it_cannot_index():
    H, W = 45, 61
    bad = [[blobs([[5, 5, 256]], [0.5])],                                                         # radius above the table
           [{'kind': 'line', 'p1': (0, 0), 'p2': (5, 5), 'thickness': 0, 'color': literal(0.5)}],
           [{'kind': 'line', 'p1': (0, 0), 'p2': (2 ** 21, 5), 'thickness': 1, 'color': literal(0.5)}],
           [{'kind': 'poly', 'points': np.zeros((65, 2), int), 'color': literal(0.5), 'copy': False}],
           [{'kind': 'box_blur', 'target': 0, 'k': 0}], [{'kind': 'box_blur', 'target': 0, 'k': 9000}],
           [{'kind': 'threshold', 'field': 0, 'key': 0, 't': 0.5}],                                # no field uploaded
           [{'kind': 'line', 'target': 1, 'p1': (0, 0), 'p2': (5, 5), 'thickness': 1, 'color': literal(0.5)}]]
    for commands in bad:
        with pytest.raises(ValueError):
            run(commands, H, W)
    with pytest.raises(ValueError):
        SS.finish(torch.zeros((1, H, W), device='cuda'), [4], [0], (H, W))                        # even blur size
