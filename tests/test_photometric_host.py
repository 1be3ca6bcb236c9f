"""Photometric augmentation, host side (no GPU): the plan drawer against the reference's draws (tests/golden/
photometric_augmentation.npz, make_golden_photometric.py), the opt-in / refusal semantics of augmentation.photometric.noise
and --photometric, and the defining properties of the OpenCV restatements (tests/photometric_restatement.py)."""
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import yaml

import photometric_restatement as R
from multipoint_amd.datasets import augmentation as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_PRIMS = ['random_brightness', 'random_contrast', 'additive_speckle_noise', 'additive_gaussian_noise', 'additive_shade',
               'motion_blur']
TRAIN_PARAMS = {'random_brightness': {'max_abs_change': 0.15}, 'random_contrast': {'strength_range': [0.3, 1.8]},
                'additive_gaussian_noise': {'stddev_range': [0, 0.06]}, 'additive_speckle_noise': {'prob_range': [0, 0.0035]},
                'additive_shade': {'transparency_range': [-0.5, 0.8], 'kernel_size_range': [50, 100]},
                'motion_blur': {'max_kernel_size': 3}}
PRIMS = ['additive_gaussian_noise', 'additive_speckle_noise', 'random_brightness', 'random_contrast', 'additive_shade',
         'motion_blur']                                  # photometric_augmentation.py:4-11, the order of 'all'


def golden_cases(golden_dir):
    """(name, config, input image, reference output, next draws) of every single-call case of the fixture."""
    g = np.load(os.path.join(golden_dir, 'photometric_augmentation.npz'))
    out = []
    for name in g['case_names']:
        name = str(name)
        seed, H, W, order, strided = (int(v) for v in g['case_%s_setup' % name])
        if name.startswith('alone_'):
            prim = [p for p in PRIMS if name.startswith('alone_' + p)][0]
            prims = [prim]
            params = {} if name.endswith('_default') else TRAIN_PARAMS
        elif name.startswith('chain_train'):
            prims, params = TRAIN_PRIMS, TRAIN_PARAMS
        else:
            prims, params = 'all', {}
        cfg = {'primitives': prims, 'params': params, 'random_order': bool(order)}
        img = np.random.default_rng(seed).random((H, W), dtype=np.float32)
        out.append((name, seed, cfg, img, g['case_%s_output' % name], g['case_%s_next_draws' % name]))
    return out


def test_plan_drawer_consumes_the_reference_stream(golden_dir):
    """Seeded like the reference's call, the plan drawer leaves `random` and `np.random` where the reference left them, and
    its scalars run through the CPU restatement of the kernels give the reference's output bit for bit."""
    cases = golden_cases(golden_dir)
    assert len(cases) == 19
    for name, seed, cfg, img, want, next_draws in cases:
        random.seed(seed); np.random.seed(seed + 7)
        plan = A.draw_photometric_plan(img.shape, dict(cfg, noise='host'))
        assert [random.random(), np.random.random()] == list(next_draws), name
        got = R.apply_plan(img, plan)
        assert got.dtype == np.float32 and np.array_equal(got, want), (name, float(np.abs(got - want).max()))


def test_plan_contents():
    assert A.PHOTOMETRIC_PRIMITIVES == PRIMS
    random.seed(3); np.random.seed(4)
    plan = A.draw_photometric_plan((64, 96), {'primitives': 'all', 'params': {}, 'random_order': False, 'noise': 'host'})
    assert [op['name'] for op in plan.ops] == PRIMS
    gauss, speckle, bright, contrast, shade, motion = plan.ops
    assert gauss['normal'].shape == (64, 96) and gauss['normal'].dtype == np.float64 and 0 <= gauss['value'] <= 0.06
    assert speckle['uniform'].shape == (64, 96) and speckle['uniform'].dtype == np.float64
    assert len(shade['ellipses']) == 20 and 251 <= shade['ksize'] <= 351 and shade['ksize'] % 2 == 1
    assert motion['ksize'] in (1, 3, 5, 7, 9) and len(motion['taps']) == motion['ksize']
    assert abs(sum(motion['taps']) - 1) < 1e-6
    # device noise: one 63-bit key per field instead of the H x W draws
    random.seed(3); np.random.seed(4)
    dplan = A.draw_photometric_plan((64, 96), {'primitives': 'all', 'params': {}, 'random_order': False, 'noise': 'device'})
    assert 'normal' not in dplan.ops[0] and 'uniform' not in dplan.ops[1]
    assert 0 <= dplan.ops[0]['key'] < 2 ** 63 and dplan.ops[0]['key'] != dplan.ops[1]['key']
    assert dplan.ops[0]['value'] == gauss['value']             # the first draw precedes the field


def test_inplace_prefix():
    random.seed(0); np.random.seed(0)
    cfg = {'primitives': ['additive_speckle_noise', 'additive_gaussian_noise', 'random_brightness'], 'params': {},
           'random_order': False, 'noise': 'host'}
    p = A.draw_photometric_plan((8, 8), cfg).inplace_prefix()
    assert [op['name'] for op in p.ops] == ['additive_speckle_noise', 'gaussian_add']
    p = A.draw_photometric_plan((8, 8), dict(cfg, primitives=['random_brightness', 'additive_speckle_noise']))
    assert p.inplace_prefix() is None
    p = A.draw_photometric_plan((8, 8), dict(cfg, primitives=['additive_speckle_noise', 'random_contrast']))
    assert [op['name'] for op in p.inplace_prefix().ops] == ['additive_speckle_noise']


def test_reference_errors():
    with pytest.raises(AssertionError):                      # parse_primitives
        A.draw_photometric_plan((16, 16), {'primitives': ['sharpen'], 'params': {}, 'random_order': False, 'noise': 'host'})
    with pytest.raises(ValueError):                          # np.random.randint(0, 0): no room for the ellipse centres
        A.draw_photometric_plan((16, 0), {'primitives': 'additive_shade', 'params': {}, 'random_order': False,
                                          'noise': 'device'})


def test_noise_key_semantics(tmp_path):
    from multipoint_amd.datasets import ImagePairDataset, SyntheticPairs
    fn = str(tmp_path / 'p.npz')
    np.savez(fn, **{'p0/optical': np.zeros((16, 16), np.float32), 'p0/thermal': np.zeros((16, 16), np.float32)})
    for cls, cfg in ((ImagePairDataset, {'filename': fn}), (SyntheticPairs, {'height': 16, 'width': 16})):
        with pytest.raises(NotImplementedError) as e:
            cls(dict(cfg, augmentation={'photometric': {'enable': True}}))
        assert 'augmentation.photometric.noise' in str(e.value) and "'host'" in str(e.value) and "'device'" in str(e.value)
        with pytest.raises(ValueError):
            cls(dict(cfg, augmentation={'photometric': {'enable': True, 'noise': 'gpu'}}))
        for mode in ('host', 'device'):
            cls(dict(cfg, augmentation={'photometric': {'enable': True, 'noise': mode}}))
        cls(dict(cfg, augmentation={'photometric': {'enable': False, 'noise': 'bogus'}}))      # disabled: not looked at
    with pytest.raises(NotImplementedError):
        A.photometric_augmentation(np.zeros((8, 8), np.float32), primitives='all', params={}, random_order=True)
    with pytest.raises(ValueError):
        A.photometric_augmentation(np.zeros((8, 8), np.float32), primitives='all', params={}, random_order=True,
                                   noise='cpu')


def _cli(tmp_path, args, noise=None):
    photometric = {'enable': True}
    if noise:
        photometric['noise'] = noise
    config = {'dataset': {'type': 'ImagePairDataset', 'augmentation': {'photometric': photometric}},
              'model': {'type': 'MultiPoint'}, 'loss': {'type': 'SuperPointLoss'},
              'training': {'batchsize': 1, 'validation': {'filename': str(tmp_path / 'missing.npz')}}}
    path = tmp_path / 'c.yaml'
    with open(path, 'w') as f:
        yaml.safe_dump(config, f)
    return subprocess.run([sys.executable, os.path.join(ROOT, 'compute_validation_loss.py'), '-y', str(path),
                           '-m', str(tmp_path)] + args, cwd=ROOT, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES='', CUDA_VISIBLE_DEVICES=''))


def test_cli_photometric_flags(tmp_path):
    r = _cli(tmp_path, ['--photometric', 'host', '--no-photometric'])
    assert r.returncode == 2 and 'not allowed with' in r.stderr
    r = _cli(tmp_path, ['--photometric', 'gpu'])
    assert r.returncode == 2 and 'invalid choice' in r.stderr
    r = _cli(tmp_path, [])                                      # neither flag, no noise key: refused, naming both ways out
    assert r.returncode != 0 and '--no-photometric' in r.stderr and '--photometric host' in r.stderr
    for args, noise in ((['--photometric', 'device'], None), ([], 'host')):
        r = _cli(tmp_path, args, noise)                         # accepted: it gets as far as the GPU check
        assert r.returncode != 0 and 'photometric' not in r.stderr, r.stderr


def test_gaussian_kernel_sums_to_one():
    for k in (1, 3, 51, 101, 251, 351):
        w = R.gaussian_kernel(k)
        assert w.dtype == np.float32 and abs(float(w.astype(np.float64).sum()) - 1.0) < 1e-5
        assert np.array_equal(w, w[::-1]) and w.argmax() == k // 2


def test_ellipse_fill_properties():
    """Filled ellipses at 0 and 90 degrees are mirror-symmetric about their centre row and column to within one pixel at
    every span end (FillConvexPoly starts each edge at its upper vertex's x and rounds both span ends up, so the
    rasterisation is not an exact mirror), span the full axes, and their pixel count differs from pi a b by at most the
    perimeter in pixels."""
    cy, cx = 40, 50
    for ax, ay in ((20, 10), (7, 13), (15, 15), (3, 2), (30, 4)):
        for angle in (0, 90):
            m = np.zeros((80, 100), np.float32)
            R.cv_ellipse_fill(m, (cx, cy), (ax, ay), angle)
            a, b = (ax, ay) if angle == 0 else (ay, ax)
            area = math.pi * a * b
            perimeter = math.pi * (3 * (a + b) - math.sqrt((3 * a + b) * (a + 3 * b)))
            assert abs(m.sum() - area) <= perimeter, (ax, ay, angle, m.sum(), area)
            ys, xs = np.nonzero(m)
            for lo, hi, c, r in ((xs.min(), xs.max(), cx, a), (ys.min(), ys.max(), cy, b)):
                assert abs(lo - (c - r)) <= 1 and abs(hi - (c + r)) <= 1, (ax, ay, angle)
            for img in (m, m.T):                                 # rows, then columns
                c = cx if img is m else cy
                for row in img:
                    if row.any():
                        nz = np.nonzero(row)[0]
                        assert np.all(np.diff(nz) == 1)           # one convex span
                        assert abs((c - nz[0]) - (nz[-1] - c)) <= 1, (ax, ay, angle)


def test_border_reflect_repeats():
    """borderInterpolate(BORDER_REFLECT_101) reflects again while the index is outside (radius >= frame size)."""
    assert [R.border_interpolate(p, 4) for p in (-1, -3, -4, -6, -7, 3, 4, 6, 9, 10)] == [1, 3, 2, 0, 1, 3, 2, 0, 3, 2]
    for n in (2, 3, 24):
        for p in range(-5 * n, 6 * n):
            q = abs(p) % (2 * n - 2)
            assert R.border_interpolate(p, n) == (q if q < n else 2 * n - 2 - q)
    assert R.border_interpolate(-5, 1) == 0


def test_image_mean_matches_numpy():
    rng = np.random.default_rng(5)
    for H, W in ((24, 32), (240, 320), (37, 53), (120, 160)):
        big = rng.random((H + 3, W + 5), dtype=np.float32)
        for img in (big[:H, :W], np.ascontiguousarray(big[:H, :W]), big[1:1 + H, 2:2 + W]):
            assert R.image_mean(img) == img.mean()
