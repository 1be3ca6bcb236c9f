"""CPU: the sub-pixel keypoint rule in float64 (tests/subpixel_restatement.py) on planted Gaussian blobs and on every "axis
not refined" branch, the fixture that pins the oracle's descriptor sampling at FRACTIONAL keypoints to the reference's, and
the host-side plumbing of the option (PairResults.kp_sub, prediction.subpixel, the library's symbols)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subpixel_restatement as R  # noqa: E402


@pytest.mark.parametrize('sigma', [0.8, 1.2, 2.0])
def test_restatement_recovers_planted_gaussians(sigma):
    """Isotropic Gaussians of any width are recovered exactly: their logarithm is a parabola on each axis."""
    rng = np.random.default_rng(int(sigma * 10))
    H, W = 120, 160
    centres, base = R.planted_centres(rng, H, W, 100)
    frac = centres - base
    assert np.abs(frac).max() <= 0.45 and base.min() >= 6 and (base[:, 0] <= H - 7).all() and (base[:, 1] <= W - 7).all()
    d = np.abs(base[:, None] - base[None]).max(-1) + 1000 * np.eye(len(base), dtype=np.int64)
    assert d.min() >= 10
    prob = R.render_blobs(H, W, centres, sigma)[None]
    sub, refined, _ = R.refine_keypoints(prob, base[None], [len(base)])
    assert refined.all()
    err = np.abs(sub[0] - centres).max()
    print('sigma %.1f: largest error %.3e px' % (sigma, err))
    assert err <= 1e-9


def _one(prob, y, x):
    sub, refined, _ = R.refine_keypoints(np.asarray(prob, np.float64)[None], np.array([[[y, x]]]), [1])
    return sub[0, 0], refined[0, 0]


def test_restatement_unrefined_axes():
    base = np.full((5, 7), 0.1)
    base[2, 3] = 0.5
    base[1, 3], base[3, 3], base[2, 2], base[2, 4] = 0.2, 0.3, 0.25, 0.15
    sub, ref = _one(base, 2, 3)
    assert ref.all() and 2 < sub[0] < 2.5 and 2.5 < sub[1] < 3 and np.abs(sub - (2, 3)).max() <= 0.5
    # a neighbour outside the frame: first / last row and column
    for (y, x), axis in (((0, 3), 0), ((4, 3), 0), ((2, 0), 1), ((2, 6), 1)):
        m = np.full((5, 7), 0.1); m[y, x] = 0.5
        sub, ref = _one(m, y, x)
        assert not ref[axis] and ref[1 - axis] and sub[axis] == (y, x)[axis]
    # a value that is zero, negative, infinite or NaN -- as a neighbour on one axis (the other axis is still refined) ...
    for bad in (0.0, -0.1, np.inf, np.nan):
        m = base.copy(); m[1, 3] = bad
        sub, ref = _one(m, 2, 3)
        assert not ref[0] and ref[1] and sub[0] == 2.0 and sub[1] != 3.0
        m = base.copy(); m[2, 4] = bad
        sub, ref = _one(m, 2, 3)
        assert ref[0] and not ref[1] and sub[1] == 3.0
    # ... and as the centre (both axes)
    for bad in (0.0, -0.1, np.inf, np.nan):
        m = base.copy(); m[2, 3] = bad
        sub, ref = _one(m, 2, 3)
        assert not ref.any() and tuple(sub) == (2.0, 3.0)
    # a centre lower than a neighbour
    m = base.copy(); m[3, 3] = 0.6
    sub, ref = _one(m, 2, 3)
    assert not ref[0] and ref[1] and sub[0] == 2.0
    # three equal values: den == 0
    m = base.copy(); m[2, 2] = m[2, 4] = 0.5
    sub, ref = _one(m, 2, 3)
    assert ref[0] and not ref[1] and sub[1] == 3.0
    # two equal neighbours: refined, and the vertex is the pixel itself
    m = base.copy(); m[2, 2] = m[2, 4] = 0.2
    sub, ref = _one(m, 2, 3)
    assert ref[1] and sub[1] == 3.0
    # a neighbour EQUAL to the centre: refined, half a pixel towards it (the largest offset the rule can give)
    m = base.copy(); m[2, 4] = 0.5
    sub, ref = _one(m, 2, 3)
    assert ref[1] and sub[1] == 3.5


def test_restatement_rows_beyond_the_count_are_zero():
    prob = np.random.default_rng(0).uniform(0.1, 1.0, (2, 6, 6))
    kp = np.full((2, 4, 2), 3)
    sub, ref, _ = R.refine_keypoints(prob, kp, [2, 9])         # (a count above K is clamped)
    assert (sub[0, 2:] == 0).all() and not ref[0, 2:].any() and (sub[0, :2] != 0).all() and (sub[1] != 0).all()


def test_oracle_sampling_at_fractional_keypoints_matches_the_reference(oracle, golden_dir):
    """tests/golden/sampling_fractional.npz holds the reference's interpolate_descriptors output for float keypoints
    (tests/golden/make_golden_sampling_fractional.py): the oracle's restatement, which the GPU tests compare the float
    sampling kernel against, must reproduce it."""
    g = np.load(os.path.join(golden_dir, 'sampling_fractional.npz'))
    desc, kp, H, W = g['desc'], g['kp'], int(g['H']), int(g['W'])
    assert desc.shape == (64, 6, 8) and kp.shape == (32, 2) and kp.dtype == np.float32
    assert (kp != np.round(kp)).any(axis=1).sum() >= 20                                   # fractional positions
    assert ((kp[:, 0] < 0) | (kp[:, 1] < 0) | (kp[:, 0] > H) | (kp[:, 1] > W)).sum() >= 4    # slightly outside the frame
    assert (kp[:, 0] == H - 1).any() and (kp[:, 1] == W - 1).any()                        # the last row and column
    assert {(0.0, 0.0), (float(H), float(W))} <= {tuple(p) for p in kp.tolist()}          # exactly on the coarse grid
    got = oracle.interpolate_descriptors(kp, desc, H, W)
    err = np.abs(got - g['out']).max()
    print('oracle vs reference at fractional keypoints: %.3e' % err)
    assert err <= 1e-6


def test_pair_results_carry_kp_sub():
    from multipoint_amd.pipeline import PairResults
    kp = torch.tensor([[[1, 2], [3, 4]], [[5, 6], [0, 0]]], dtype=torch.int32)
    cnt = torch.tensor([2, 1], dtype=torch.int32)
    desc = torch.zeros((2, 2, 64))
    midx = torch.tensor([[0, -1]], dtype=torch.int32)
    md = torch.zeros((1, 2))
    plain = PairResults(kp, None, cnt, desc, midx, md, torch.tensor([1]), 8, 8, 'mutual')          # positional callers
    assert plain.kp_sub is None and 'kp_optical_sub' not in plain.to_host()[0]
    sub = kp.float() + 0.25
    res = PairResults(kp, None, cnt, desc, midx, md, torch.tensor([1]), 8, 8, kp_sub=sub)
    host = res.to_host()[0]
    assert host['kp_optical_sub'].dtype == np.float32
    assert np.array_equal(host['kp_optical_sub'], sub[0].numpy()) and np.array_equal(host['kp_thermal_sub'], sub[1, :1].numpy())
    assert np.array_equal(host['kp_optical'], kp[0].numpy())
    with pytest.raises(TypeError):
        PairResults(kp, None, cnt, desc, midx, md, torch.tensor([1]), 8, 8, 'mutual', sub)         # keyword only


def test_pipeline_reads_the_subpixel_key():
    from multipoint_amd.models import ClassicDetectors
    from multipoint_amd.pipeline import PairPipeline
    assert PairPipeline(None, {}).subpixel is False
    assert PairPipeline(None, {'subpixel': {'enable': False}}).subpixel is False
    assert PairPipeline(None, {'subpixel': {'enable': True}}).subpixel is True
    with pytest.raises(ValueError, match='unknown key'):
        PairPipeline(None, {'subpixel': {'enable': True, 'window': 5}})
    classic = ClassicDetectors.__new__(ClassicDetectors)         # (no GPU here: the check reads the type, not the weights)
    with pytest.raises(ValueError, match='ClassicDetectors'):
        PairPipeline(classic, {'subpixel': {'enable': True}})
    assert PairPipeline(classic, {'subpixel': {'enable': False}}).subpixel is False


def test_shipped_configs_and_parsers_name_the_option():
    import yaml
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name in ('config_image_pair_dataset_prediction.yaml', 'config_hdf5_pair_prediction.yaml'):
        cfg = yaml.safe_load(open(os.path.join(root, 'configs', name)))
        assert cfg['prediction']['subpixel'] == {'enable': False}
    import estimate_initial_transform
    import predict_align_image_pair
    assert predict_align_image_pair.build_parser().parse_args(['--subpixel']).subpixel is True
    assert predict_align_image_pair.build_parser().parse_args([]).subpixel is False
    assert estimate_initial_transform.build_parser().parse_args(['-i', 'x', '--subpixel']).subpixel is True


def test_library_exports_the_subpixel_entries():
    import ctypes

    import __graft_entry__ as g
    g.build()
    from multipoint_amd import _lib
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('mp_refine_keypoints', 'mp_sample_descriptors_f', 'mp_find_homography_f', 'mp_refine_homography_f',
                 'mp_pool_matches_f'):
        assert name in _lib.SIGNATURES and hasattr(dll, name)
    # the float entries take what their int namesakes take
    for name in ('mp_sample_descriptors', 'mp_find_homography', 'mp_refine_homography', 'mp_pool_matches'):
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name + '_f']
