"""SyntheticShapes without a GPU: the planners of multipoint_amd/utils/draw_primitives.py against the fixture the reference
wrote (tests/golden/synthetic_shapes.npz), the dataset's config handling, and the edge cases of the OpenCV restatement the
kernels are pinned against (tests/shapes_restatement.py)."""
import copy
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shapes_cases as C  # noqa: E402
import shapes_restatement as S  # noqa: E402

import multipoint_amd.datasets as datasets  # noqa: E402
from multipoint_amd.datasets.synthetic_shapes import SyntheticShapes, parse_primitives  # noqa: E402
from multipoint_amd.utils import draw_primitives as D  # noqa: E402


def test_dataset_is_exported():
    assert getattr(datasets, 'SyntheticShapes') is SyntheticShapes
    assert not SyntheticShapes(C.case_config('a_draw_lines')).returns_pair()


def plan_case(name):
    case = C.case(name)
    seed = int(case['setup'][0])
    ds = SyntheticShapes(C.case_config(name))
    random.seed(seed)
    np.random.seed(seed + 7)
    plan, is_optical, primitive = ds.draw_plan(lambda plan: float(case['bg_mean']))
    return ds, case, plan, is_optical, primitive


@pytest.mark.parametrize('name', C.CASE_NAMES)
def test_planner_reproduces_the_reference(name):
    ds, case, plan, is_optical, primitive = plan_case(name)
    next_draws = np.array([random.random(), np.random.random()])
    assert primitive == C.PRIMITIVES[int(case['setup'][9])]
    assert is_optical == bool(case['setup'][8])
    # every get_random_color call: the raw draw, exactly
    assert np.array_equal(np.array(plan.color_draws), case['colors'][:, 0])
    # every drawing call: integer geometry, thickness, radius, kernel size and the colour each resolves to, exactly
    assert np.array_equal(C.plan_log(plan, case['colors'][:, 1]), case['log'])
    assert np.array_equal(ds.scale_keypoints(plan.keypoints), case['keypoints'])
    assert np.array_equal(next_draws, case['next_draws'])
    if plan.noise == 'host':
        np.random.seed(int(case['setup'][0]) + 7)
        assert np.array_equal(plan.fields[0], np.random.rand(*plan.shape))


def test_only_the_checkerboard_asks_for_the_background_mean():
    asked = []
    for name in C.CASE_NAMES:
        case = C.case(name)
        ds = SyntheticShapes(C.case_config(name))
        random.seed(int(case['setup'][0]))
        np.random.seed(int(case['setup'][0]) + 7)
        _, _, primitive = ds.draw_plan(lambda plan: asked.append(name) or float(case['bg_mean']))
    assert asked == [n for n in C.CASE_NAMES if 'checkerboard' in n]
    with pytest.raises(ValueError):
        D.draw_checkerboard(D.ShapePlan((96, 128)))


def test_fixture_keeps_the_colour_margin():
    for name in C.CASE_NAMES:
        u, bg, _, mc = C.case(name)['colors'].T
        assert np.all(np.abs(np.abs(u - bg) - mc) >= 1e-4)


def test_config_defaults_and_merging():
    before = copy.deepcopy(SyntheticShapes.default_config)
    quiet = {'augmentation': {'photometric': {'enable': False}}}
    ds = SyntheticShapes(quiet)
    assert SyntheticShapes.default_config == before           # merged into a copy, not into the class
    assert len(ds) == 1000 and ds.primitives == SyntheticShapes.all_primitives and len(ds.primitives) == 9
    assert ds.config['generation_size'] == [960, 1280] and ds.config['image_size'] == [240, 320]
    assert ds.config['processing'] == {'blur_size': 21, 'additional_ir_blur': True, 'additional_ir_blur_size': 51}
    assert ds.config['generation']['generate_background']['max_kernel_size'] == 500
    assert ds.config['generation']['draw_stripes'] == {'transform_params': (0.1, 0.1)}
    assert 'draw_polygon' not in ds.config['generation']      # the reference's key is 'draw_polygons': never looked up
    assert ds.config['augmentation']['homographic']['enable'] is True
    ds = SyntheticShapes(dict(quiet, length=7, generation={'generate_background': {'min_kernel_size': 9}}))
    assert len(ds) == 7
    assert ds.config['generation']['generate_background'] == {'min_kernel_size': 9, 'max_kernel_size': 500,
                                                              'min_rad_ratio': 0.02, 'max_rad_ratio': 0.031}
    # the reference yaml's `preprocessing:` block is merged and never read
    ds = SyntheticShapes(dict(quiet, preprocessing={'blur_size': 11}))
    assert ds.config['preprocessing'] == {'blur_size': 11} and ds.config['processing']['blur_size'] == 21


def test_primitives_and_noise_rules():
    quiet = {'augmentation': {'photometric': {'enable': False}}}
    assert SyntheticShapes(dict(quiet, primitives=['draw_star', 'draw_cube'])).primitives == ['draw_star', 'draw_cube']
    assert SyntheticShapes(dict(quiet, primitives='draw_star')).primitives == ['draw_star']
    assert parse_primitives('all', ['a', 'b']) == ['a', 'b']
    with pytest.raises(AssertionError):
        SyntheticShapes(dict(quiet, primitives=['draw_circle']))
    assert SyntheticShapes(quiet).noise == 'host'
    assert SyntheticShapes(dict(quiet, generation={'noise': 'device'})).noise == 'device'
    with pytest.raises(ValueError):
        SyntheticShapes(dict(quiet, generation={'noise': 'gpu'}))
    with pytest.raises(NotImplementedError):                  # an enabled photometric block must name its noise mode
        SyntheticShapes({})
    SyntheticShapes({'augmentation': {'photometric': {'noise': 'device'}}})
    assert datasets.loader_num_workers(SyntheticShapes(dict(quiet, augmentation={
        'photometric': {'enable': False}, 'homographic': {'enable': False}})), 4) == 0


def test_device_noise_draws_one_key_instead_of_the_field():
    cfg = C.case_config('a_draw_polygon')
    cfg['generation']['noise'] = 'device'
    ds = SyntheticShapes(cfg)
    random.seed(3)
    np.random.seed(4)
    plan, _, _ = ds.draw_plan(None)
    assert plan.fields == [] and plan.commands[0]['kind'] == 'threshold' and plan.commands[0]['field'] == -1
    np.random.seed(4)
    assert plan.commands[0]['key'] == int(np.random.randint(0, 2 ** 63, dtype=np.int64))


def test_gaussian_noise_consumes_no_draw():
    cfg = C.case_config('a_gaussian_noise')
    cfg['generation']['randu_seed'] = 5
    ds = SyntheticShapes(cfg)
    keys = []
    for _ in range(2):
        plan, _, _ = ds.draw_plan(None)
        keys.append(plan.commands[-1]['key'])
        assert plan.commands[-1]['kind'] == 'randu'
    assert keys[0] != keys[1]                                # the sample counter is part of the key
    random.seed(1)
    np.random.seed(2)
    state, np_state = random.getstate(), np.random.get_state()[1].copy()
    D.gaussian_noise(D.ShapePlan((8, 8)))
    assert random.getstate() == state and np.array_equal(np.random.get_state()[1], np_state)


# ---- the restatement's own edge cases --------------------------------------------------------------------------------
def canvas(H=21, W=25):
    return np.zeros((H, W))


def test_circle_radius_zero_is_one_pixel():
    img = S.circle(canvas(), (7, 5), 0, 1.0)
    assert img.sum() == 1 and img[5, 7] == 1
    assert S.circle(canvas(), (-1, 5), 0, 1.0).sum() == 0
    assert S.circle_halfwidths(1) == [1, 0] and S.circle_halfwidths(3) == [3, 2, 2, 0]
    img = S.circle(canvas(), (0, 0), 3, 1.0)                  # centred on a corner: the quarter inside the frame
    assert img[0, :5].tolist() == [1, 1, 1, 1, 0] and img[3, :3].tolist() == [1, 0, 0]


def test_line_thickness_one_two_three():
    thin = S.line(canvas(), (3, 4), (20, 11), 1.0, 1)
    assert thin.sum() == 18                                   # 8-connected: one pixel per column of the major axis
    two = S.line(canvas(), (3, 4), (20, 11), 1.0, 2)
    three = S.line(canvas(), (3, 4), (20, 11), 1.0, 3)
    assert np.all(two >= thin) and np.all(three >= two) and thin.sum() < two.sum() < three.sum()
    assert S.thick_line_rect((3, 4), (3, 4), 3)[0] is None    # zero length: the end circles alone
    dot = S.line(canvas(), (3, 4), (3, 4), 1.0, 3)
    assert np.array_equal(dot, S.circle(canvas(), (3, 4), 2, 1.0))
    assert S.line(canvas(), (-30, -5), (-2, -40), 1.0, 1).sum() == 0
    crossing = S.line(canvas(), (-10, 10), (40, 10), 1.0, 1)  # both ends outside
    assert crossing[10].sum() == 25 and crossing.sum() == 25


def test_polygon_outside_the_frame_writes_nothing():
    pts = np.array([[-30, -30], [-5, -28], [-12, -3]])
    assert S.fill_poly(canvas(), pts, 1.0).sum() == 0
    assert S.fill_convex_poly(canvas(), pts + [100, 0], 1.0).sum() == 0
    inside = S.fill_poly(canvas(), np.array([[2, 2], [12, 3], [6, 15]]), 0.5)
    assert inside[2, 2] == 0.5 and inside[15, 6] == 0.5 and inside[7, 6] == 0.5 and inside[7, 20] == 0
    convex = S.fill_convex_poly(canvas(), np.array([[2, 2], [12, 3], [6, 15]]), 1.0)
    # the convex walk rounds its right edge where the edge table takes the floor: a few more pixels, never fewer
    assert np.all(convex[inside != 0] == 1) and inside.astype(bool).sum() == 79 and convex.sum() == 85
    line = S.fill_poly(canvas(), np.array([[2, 2], [6, 6], [10, 10]]), 1.0)     # collinear: the outline alone
    assert line.sum() == 9


def test_box_blur_anchor_and_large_kernels():
    img = np.zeros((5, 9))
    img[2, 4] = 4.0
    even = S.blur(img, 2)                                     # anchor 1: the window of (y, x) is rows y-1..y, cols x-1..x
    assert even[2, 4] == 1 and even[3, 5] == 1 and even[1, 3] == 0 and even[2, 3] == 0
    rng = np.random.default_rng(0)
    img = rng.random((5, 7))
    for k in (1, 3, 11, 16, 40):                              # 40 > twice the frame: the reflection repeats
        direct = np.empty_like(img)
        a = k // 2
        for y in range(5):
            for x in range(7):
                rows = [S.P.border_interpolate(y - a + j, 5) for j in range(k)]
                cols = [S.P.border_interpolate(x - a + j, 7) for j in range(k)]
                direct[y, x] = img[np.ix_(rows, cols)].sum() / (k * k)
        assert np.allclose(S.blur(img, k), direct, rtol=0, atol=1e-13)


def test_resize_and_affine():
    img = np.arange(12.0).reshape(3, 4)
    assert np.array_equal(S.resize(img, (4, 3)), img)
    half = S.resize(np.arange(16.0).reshape(4, 4), (2, 2))
    assert np.allclose(half, [[2.5, 4.5], [10.5, 12.5]])
    m = S.get_affine_transform([[0, 0], [1, 0], [0, 1]], [[2, 3], [4, 3], [2, 6]])
    assert np.allclose(m, [[2, 0, 2], [0, 3, 3]])
    assert np.allclose(D.get_affine_transform([[0, 0], [1, 0], [0, 1]], [[2, 3], [4, 3], [2, 6]]), m)
