"""CPU: the host side of the motion models of the mutual-information refinement: parameter extraction,
default limits, candidate names, the affine geometric checks, the stage sequence and the command lines' flags."""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def A():
    from multipoint_amd.utils import alignment
    return alignment


def test_model_parameters_by_hand(A):
    # T[2,2] = 2: everything is divided by it first.  T00 = 0.6, T01 = 0.8: a 3-4-5 triangle
    T = np.array([[1.2, 1.6, 6.0], [-1.6, 1.2, -8.0], [0.0, 0.0, 2.0]])
    p = A.model_parameters(T, 'similarity')
    assert p.shape == (4,) and p.dtype == np.float64
    assert abs(p[0] - math.atan2(0.8, 0.6)) <= 2 ** -52 and abs(p[1] - 1.0) <= 2 ** -52 and p[2] == 3.0 and p[3] == -4.0
    # the second row is not read
    T2 = T.copy()
    T2[1, :2] = [5.0, -7.0]
    assert np.array_equal(A.model_parameters(T2, 'similarity'), p)
    # a quarter turn: cos is 0, the scale is no quotient by it
    Q = np.array([[0.0, 1.5, 7.0], [-1.5, 0.0, -2.0], [0.0, 0.0, 1.0]])
    q = A.model_parameters(Q, 'similarity')
    assert abs(q[0] - math.pi / 2) <= 2 ** -52 and np.array_equal(q[1:], [1.5, 7.0, -2.0])
    assert np.array_equal(A.model_parameters(T, 'affine'), [0.6, 0.8, 3.0, -0.8, 0.6, -4.0])
    assert np.array_equal(A.model_parameters(T, 'homography'), T.ravel())            # the nine entries as given
    # several matrices, as (P, 3, 3) or (P, 9)
    both = A.model_parameters(np.stack([T, Q]), 'similarity')
    assert both.shape == (2, 4) and np.array_equal(both[0], p) and both[1, 1] == 1.5
    assert A.model_parameters(np.stack([T, Q]).reshape(2, 9), 'affine').shape == (2, 6)
    assert A.model_parameters(T.ravel(), 'affine').shape == (6,)
    with pytest.raises(ValueError, match='unknown transform model'):
        A.model_parameters(T, 'rigid')
    with pytest.raises(ValueError, match=r'T\[2,2\]'):
        A.model_parameters(np.zeros((3, 3)), 'similarity')
    with pytest.raises(NotImplementedError, match='warpAffine'):
        A.model_parameters(T[:2], 'affine')                                          # a 2x3 input is still refused
    assert A.MODEL_PARAMETERS == {'homography': 9, 'similarity': 4, 'affine': 6}


def test_default_limits_are_scipys(A):
    assert [A.default_limit(m) for m in ('homography', 'similarity', 'affine')] == [1800, 800, 1200]
    with pytest.raises(ValueError, match='unknown transform model'):
        A.default_limit('rigid')


def test_alignment_type_name(A):
    assert A.alignment_type_name(64, True, 0) == 'bin64_normalized_s0'
    assert A.alignment_type_name(64, True, 0, 'homography') == 'bin64_normalized_s0'
    assert A.alignment_type_name(64, True, 0, model='similarity') == 'bin64_normalized_s0_similarity'
    assert A.alignment_type_name(16, False, 1.5, 'affine') == 'bin16_s1.5_affine'


def _limits():
    return {'alignment/check/both/max_diff_dx': 2.5, 'alignment/check/both/max_diff_dy': 3.5,
            'alignment/check/affine/max_diff_scale': 0.005, 'alignment/check/affine/max_diff_rotation': 0.1,
            'alignment/check/affine/max_diff_shear': 5.72}


def test_affine_geometry_checks_by_hand(A):
    """align.py:391-404 for init = identity (rot 0, shear 0, s_x = s_y = 1) and T = [[1, 0, 2], [0.1, 1, -3]]:
    rot = arctan2(0, 1) = 0; shear = arctan2(1, 0.1) - pi/2 - 0 = -arctan(0.1) = -5.7106 deg; s_x = sqrt(0.1^2 + 1) =
    1.0049876; s_y = sqrt(1 + 0) cos(shear) = 1 / sqrt(1.01) = 0.9950372; |d dx| = 2, |d dy| = 3."""
    init = np.eye(3)
    T = np.array([[1.0, 0.0, 2.0], [0.1, 1.0, -3.0], [0.0, 0.0, 1.0]])
    assert abs(math.degrees(math.atan(0.1)) - 5.7106) < 1e-4 and abs(math.sqrt(1.01) - 1.0049876) < 1e-7
    assert A.check_affine_geometry(init, T, _limits()) is True
    assert A.check_affine_geometry(init * 2.0, T * 2.0, _limits()) is True                      # divided by [2,2] first
    for key, value in (('alignment/check/both/max_diff_dx', 2.0),                             # strict: 2 < 2 fails
                       ('alignment/check/both/max_diff_dy', 3.0),
                       ('alignment/check/affine/max_diff_scale', 0.00497),                    # s_x: 0.0049876; s_y: 0.0049628
                       ('alignment/check/affine/max_diff_shear', 5.71)):
        assert A.check_affine_geometry(init, T, dict(_limits(), **{key: value})) is False, key
    # s_y alone: T11 = 1.01
    Sy = np.diag([1.0, 1.01, 1.0])
    assert A.check_affine_geometry(init, Sy, dict(_limits(), **{'alignment/check/affine/max_diff_scale': 0.0101}))
    assert not A.check_affine_geometry(init, Sy, dict(_limits(), **{'alignment/check/affine/max_diff_scale': 0.0099}))
    # a rotation by 0.3 deg in the reference's convention: rot = 0.3 deg, shear = (pi/2 + t) - pi/2 - t = 0, scales 1
    t = math.radians(0.3)
    Rm = np.array([[math.cos(t), math.sin(t), 0.0], [-math.sin(t), math.cos(t), 0.0], [0.0, 0.0, 1.0]])
    assert A.check_affine_geometry(init, Rm, dict(_limits(), **{'alignment/check/affine/max_diff_rotation': 0.31}))
    assert not A.check_affine_geometry(init, Rm, dict(_limits(), **{'alignment/check/affine/max_diff_rotation': 0.29}))
    # differences, not absolute values: the same rotation on both sides passes the tightest limit
    assert A.check_affine_geometry(Rm, Rm, dict(_limits(), **{'alignment/check/affine/max_diff_rotation': 1e-9}))
    for key in A.AFFINE_CHECK_KEYS:
        p = _limits()
        del p[key]
        with pytest.raises(KeyError, match=re.escape(key)):
            A.check_affine_geometry(init, T, p)


def test_fences_stay_with_a_model(A):
    import torch
    img = torch.zeros((8, 8))
    base = {'alignment/bin_sizes': [16], 'alignment/model': 'similarity'}
    with pytest.raises(NotImplementedError, match='warpAffine'):
        A.align_images(img, img, np.eye(3), dict(base, **{'alignment/decomposed_transformation': True}))
    with pytest.raises(ValueError, match='unknown transform model'):
        A.align_images(img, img, np.eye(3), dict(base, **{'alignment/model': 'rigid'}))
    # geometric checks: the homography raises as before, a constrained model names the limit that is missing
    with pytest.raises(NotImplementedError, match='decomposeHomographyMat'):
        A.align_images(img, img, np.eye(3), {'alignment/bin_sizes': [16], 'alignment/model': 'homography'}, geometric_checks=True)
    with pytest.raises(KeyError, match='alignment/check/both/max_diff_dx'):
        A.align_images(img, img, np.eye(3), base, geometric_checks=True)
    with pytest.raises(ValueError, match='unknown transform model'):
        A.refine_alignment_batch(img, img, [0], [16], np.eye(3)[None], model='rigid')
    with pytest.raises(ValueError, match='unknown transform model'):
        A.model_transform(np.zeros(4), 'rigid')
    with pytest.raises(ValueError, match='parameters must be'):
        A.model_transform(np.zeros(5), 'similarity')


class _Recorder:
    """a stand-in aligner: every pair succeeds, the parameters of every call are kept"""

    def __init__(self):
        self.seen = []

    def blur(self, frames, k, decimate):
        return frames[:, ::2, ::2].copy() if decimate else frames.copy()

    def __call__(self, optical, thermal, T, params, filter_images):
        self.seen.append((optical.shape[1:], filter_images, params.get('alignment/model')))
        n = optical.shape[0]
        return [T[j].copy() for j in range(n)], ['bin16_s0_similarity'] * n, [[] for _ in range(n)]


def test_stages_hand_the_model_to_every_stage(A):
    frames = np.zeros((2, 8, 12))
    params = {'use_image_pyramid': True, 'use_smoothing_stage': True, 'alignment/n_pyramid_levels': 2,
              'alignment/filter_size': 5, 'alignment/model': 'similarity'}
    rec = _Recorder()
    out = A.run_alignment_stages(frames, frames.copy(), np.stack([np.eye(3)] * 2), params, rec, rec.blur)
    assert [s[:2] for s in rec.seen] == [((2, 3), False), ((4, 6), False), ((8, 12), True), ((8, 12), False)]
    assert all(s[2] == 'similarity' for s in rec.seen)
    for ok, T, kind, cands, stages in out:
        assert ok and kind == 'bin16_s0_similarity' and all(s['type'].endswith('_similarity') for s in stages)
    with pytest.raises(ValueError, match='unknown transform model'):
        A.run_alignment_stages(frames, frames, np.stack([np.eye(3)] * 2), dict(params, **{'alignment/model': 'rigid'}), rec, rec.blur)
    # the older fences are in front of nothing new
    with pytest.raises(NotImplementedError, match='warpAffine'):
        A.run_alignment_stages(frames, frames, np.stack([np.eye(3)] * 2), dict(params, perspective=False), rec, rec.blur)


def test_cli_parsers():
    import align_images as AI
    import predict_align_image_pair as P
    assert AI.build_parser().parse_args([]).transform is None                        # (None: alignment/model decides)
    assert P.build_parser().parse_args([]).mi_transform is None
    for m in ('homography', 'similarity', 'affine'):
        assert AI.build_parser().parse_args(['--transform', m]).transform == m
        args = P.build_parser().parse_args(['--mi-refine', '--mi-transform', m])
        assert args.mi_transform == m and args.mi_refine and args.transform is None   # the estimate's own model is another flag
    for parser, argv in ((AI.build_parser(), ['--transform', 'rigid']), (P.build_parser(), ['--mi-transform', 'rigid'])):
        with pytest.raises(SystemExit):
            parser.parse_args(argv)


def test_config_default_is_the_homography(A):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'config_align_images.yaml')))
    assert cfg['alignment/model'] == 'homography'
    assert all(key in cfg for key in A.AFFINE_CHECK_KEYS)


def test_parameter_count_is_the_headers():
    from multipoint_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'multipoint_hip.h')).read()
    common = open(os.path.join(ROOT, 'multipoint_amd', 'csrc', 'mp_common.h')).read()
    assert int(re.search(r'#define MP_MI_PARAMS_MAX (\d+)', header).group(1)) == _lib.MP_MI_PARAMS_MAX == 9
    assert int(re.search(r'#define MI_PARAMS_MAX (\d+)', common).group(1)) == _lib.MP_MI_PARAMS_MAX
    assert _lib.MP_MI_PARAMS_MAX + 1 <= _lib.MP_MI_SLOTS
