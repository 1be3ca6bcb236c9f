"""ImagePairDataset / SyntheticPairs with photometric augmentation on the GPU against the samples the REFERENCE's
ImagePairDataset emitted for the same arrays and seeds (tests/golden/photometric_augmentation.npz,
make_golden_photometric.py): photometric before the homographic warp, optical then thermal, the aliased pair of a single
random_pairs flip included.  Schema, homographies, valid masks and label maps exactly, images within 1e-5."""
import os
import random

import numpy as np
import pytest
import torch

from test_photometric_host import TRAIN_PARAMS, TRAIN_PRIMS

pytestmark = pytest.mark.gpu
HCFG = {'enable': True,
        'params': {'translation': True, 'rotation': True, 'scaling': True, 'perspective': True,
                   'scaling_amplitude': 0.2, 'perspective_amplitude_x': 0.2, 'perspective_amplitude_y': 0.2,
                   'patch_ratio': 0.85, 'max_angle': 1.57, 'allow_artifacts': True, 'translation_overflow': 0.05},
        'valid_border_margin': 0, 'border_reflect': True}


def _store(tmp_path, g):
    arrays, labels = {}, {}
    for i in range(3):
        arrays['s%d/optical' % i], arrays['s%d/thermal' % i] = g['in_optical_%d' % i], g['in_thermal_%d' % i]
        labels['s%d/keypoints' % i] = g['in_keypoints_%d' % i]
    fn, kfn = str(tmp_path / 'pairs.npz'), str(tmp_path / 'labels.npz')
    np.savez(fn, **arrays); np.savez(kfn, **labels)
    return fn, kfn


def _check(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.dtype == np.float32 and what[-1] == 'image':
        assert float(np.abs(got - want).max()) <= 1e-5, what
    else:
        assert np.array_equal(got, want), what


def test_dataset_photometric_against_reference_golden(tmp_path, golden_dir):
    from multipoint_amd.datasets import ImagePairDataset
    g = np.load(os.path.join(golden_dir, 'photometric_augmentation.npz'))
    fn, kfn = _store(tmp_path, g)
    pcfg = {'enable': True, 'primitives': TRAIN_PRIMS, 'params': TRAIN_PARAMS, 'random_order': True, 'noise': 'host'}
    common = {'filename': fn, 'keypoints_filename': kfn, 'height': 48, 'width': 80,
              'augmentation': {'photometric': pcfg, 'homographic': HCFG}}
    pair = ImagePairDataset(dict(common, single_image=False, random_pairs=True))
    aliased = 0
    for i, (rs, ns) in enumerate(g['pair_seeds']):
        random.seed(int(rs)); np.random.seed(int(ns))
        s = pair[i]
        assert s['name'] == 's%d' % i and set(s) == {'optical', 'thermal', 'name'}
        for side in ('optical', 'thermal'):
            assert set(s[side]) == {'image', 'valid_mask', 'keypoints', 'homography', 'is_optical'}
            for k in ('image', 'valid_mask', 'keypoints', 'homography', 'is_optical'):
                _check(s[side][k].numpy(), g['pair_%d_%s_%s' % (i, side, k)], (i, side, k))
        aliased += bool(s['optical']['is_optical']) == bool(s['thermal']['is_optical'])
    assert aliased >= 1                                 # the fixture's first seed makes one array of the pair
    single = ImagePairDataset(dict(common, single_image=True))
    random.seed(77); np.random.seed(78)
    s = single[1]
    assert set(s) == {'image', 'valid_mask', 'keypoints', 'is_optical', 'name'}
    for k in ('image', 'valid_mask', 'keypoints', 'is_optical'):
        _check(s[k].numpy(), g['single_1_%s' % k], ('single', k))


def test_synthetic_pairs_photometric():
    """SyntheticPairs goes through build_sample: device noise reproducible for fixed seeds; photometric without the warp
    keeps the all-valid masks; the images are augmented (differ from make_pair's)."""
    from multipoint_amd.datasets import SyntheticPairs
    cfg = {'num_samples': 2, 'height': 64, 'width': 96, 'random_pairs': False,
           'augmentation': {'photometric': {'enable': True, 'primitives': TRAIN_PRIMS, 'params': TRAIN_PARAMS,
                                            'random_order': True, 'noise': 'device'}}}
    ds = SyntheticPairs(cfg)
    random.seed(1); np.random.seed(2)
    a = ds[1]
    random.seed(1); np.random.seed(2)
    b = ds[1]
    opt, th = SyntheticPairs.make_pair(0, 1, 64, 96)
    for side, raw in (('optical', opt), ('thermal', th)):
        assert torch.equal(a[side]['image'], b[side]['image'])
        assert a[side]['image'].shape == (1, 64, 96) and a[side]['image'].dtype == torch.float32
        assert bool(a[side]['valid_mask'].all()) and not torch.equal(a[side]['image'], torch.from_numpy(raw))
        assert float(a[side]['image'].min()) >= 0 and float(a[side]['image'].max()) <= 1
