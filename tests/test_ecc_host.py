"""CPU: the premises the ECC tests rest on, checked on the float64 restatement (tests/ecc_restatement.py), and what of
multipoint_amd.utils.ecc and the library's mp_ecc_* entries needs no device: names, status codes, the sum count, the limits."""
import ctypes

import numpy as np
import pytest

import ecc_cases as C
import ecc_restatement as E
from multipoint_amd import _lib
from multipoint_amd.utils import ecc as U

MODELS = ('translation', 'similarity', 'affine', 'homography')


def test_vocabulary():
    assert {m: k for m, (_, k) in U.ECC_MODELS.items()} == E.PARAMS
    assert (U.ECC_OK, U.ECC_FEW_VALID, U.ECC_NOT_POSITIVE, U.ECC_LAMBDA, U.ECC_NONFINITE) == \
        (E.OK, E.FEW_VALID, E.NOT_POSITIVE, E.LAMBDA, E.NONFINITE)
    for m in MODELS:
        assert U.ecc_sum_count(m) == E.n_sums(E.PARAMS[m])
    assert U.ecc_sum_count('homography') == 66
    with pytest.raises(ValueError):
        U.ecc_sum_count('projective')
    import multipoint_amd.utils as top
    assert top.refine_alignment_ecc_batch is U.refine_alignment_ecc_batch


def test_workspace_limits():
    lib = _lib.load_library()
    for name in ('mp_ecc_workspace_bytes', 'mp_ecc_prepare', 'mp_ecc_sums', 'mp_ecc_begin', 'mp_ecc_step', 'mp_ecc_result'):
        assert hasattr(lib, name)
    need = _lib.c_ll()
    assert lib.mp_ecc_workspace_bytes(3, 72, 96, ctypes.byref(need)) == _lib.MP_OK
    chunks = (72 * 96 + 4095) // 4096
    assert need.value >= 3 * chunks * 66 * 8
    for P, H, W in ((0, 72, 96), (4097, 72, 96), (1, 7, 96), (1, 72, 7), (1, 4097, 96), (1, 72, 4097)):
        assert lib.mp_ecc_workspace_bytes(P, H, W, ctypes.byref(need)) == -1, (P, H, W)
    assert lib.mp_ecc_workspace_bytes(4096, 8, 8, ctypes.byref(need)) == _lib.MP_OK


@pytest.mark.parametrize('model', MODELS)
def test_jacobian_against_finite_differences(model):
    rng = np.random.default_rng(3)
    T = E.start_transform(np.array([[0.93, -0.08, 11.0], [0.07, 0.95, -6.0], [2e-4, -1e-4, 1.0]]), model)
    if model == 'translation':
        T[2] = (0.0, 0.0, 1.0)
    x, y = rng.uniform(0, 95, 50), rng.uniform(0, 71, 50)
    xs, ys = E.warp(T, x, y)
    den = T[2, 0] * x + T[2, 1] * y + T[2, 2]
    dxs, dys = E.jacobian(model, x, y, xs, ys, den)
    K = E.PARAMS[model]
    assert dxs.shape == dys.shape == (K, 50)
    assert np.allclose(E.updated(T, np.zeros(K), model), T, rtol=0, atol=0)
    for k in range(K):
        h = 1e-6 if model != 'homography' or k < 6 else 1e-9
        d = np.zeros(K)
        d[k] = h
        xp, yp = E.warp(E.updated(T, d, model), x, y)
        xm, ym = E.warp(E.updated(T, -d, model), x, y)
        scale = 1.0 + np.abs(dxs[k]).max() + np.abs(dys[k]).max()
        assert np.abs((xp - xm) / (2 * h) - dxs[k]).max() < 1e-5 * scale, (model, k)
        assert np.abs((yp - ym) / (2 * h) - dys[k]).max() < 1e-5 * scale, (model, k)


@pytest.mark.parametrize('model', ('similarity', 'homography'))
def test_gain_and_bias_leave_the_trajectory_alone(model):
    name = 'small_thermal_far'
    optical, thermal, _ = C.pair(name)
    planes = E.image_planes(E.features(optical))
    template = E.features(thermal)
    a, b = 3.7, -0.4
    h0, h1, h2 = [], [], []
    E.refine_features(planes, template, C.start(name, 'near'), model, eps=0.0, maxiter=8, history=h0)
    E.refine_features((a * planes[0] + b, a * planes[1], a * planes[2]), template, C.start(name, 'near'), model, eps=0.0,
                      maxiter=8, history=h1)
    E.refine_features(planes, 0.3 * template + 2.0, C.start(name, 'near'), model, eps=0.0, maxiter=8, history=h2)
    assert len(h0) == len(h1) == len(h2) == 8
    for (T0, r0), (T1, r1), (T2, r2) in zip(h0, h1, h2):
        assert np.abs(T1 - T0).max() < 1e-9 and np.abs(T2 - T0).max() < 1e-9
        assert abs(r1 - r0) < 1e-9 and abs(r2 - r0) < 1e-9


def test_converges_on_a_smooth_analytic_pair():
    """A sum of Gaussians (sigma >= 5 px) under a known similarity, gain 0.7 and bias 0.1, raw intensities, no blur: the
    iteration ends within a tenth of a pixel (bilinear sampling of so smooth a frame is off by far less)."""
    T_true = np.array([[0.8 * np.cos(0.05), -0.8 * np.sin(0.05), 14.0], [0.8 * np.sin(0.05), 0.8 * np.cos(0.05), 9.0], [0, 0, 1.0]])
    optical = C.gaussians((96, 128))
    thermal = C.gaussians((72, 96), T_true, gain=0.7, bias=0.1)
    T0 = C.perturbed(T_true, (72, 96), 1.5)
    assert 3.0 < C.corner_distance(T0, T_true, (72, 96)) < 8.0
    for model in ('similarity', 'affine', 'homography'):
        r = E.refine(optical, thermal, T0, model, 'intensity', 1, 1e-10, 100)
        assert r['success'] and r['converged'], model
        assert C.corner_distance(r['transform'], T_true, (72, 96)) < 0.1, model


@pytest.mark.parametrize('name', C.NAMES)
def test_intensity_on_an_inverted_pair_stops_at_once(name):
    """Documented behaviour: the contrast-inverted thermal frame correlates negatively with the optical one, lambda's
    denominator is not positive and the refinement stops before its first update."""
    r = C.restated(name, 'near', 'similarity', 50, 1e-6, False, 'intensity')
    assert r['status'] == U.ECC_LAMBDA and r['nit'] == 0 and not r['success']
    assert r['rho'] < -0.9
    assert np.array_equal(r['transform'], E.start_transform(C.start(name, 'near'), 'similarity'))


def test_fixture_condition_keeps_enough_cases():
    assert len(C.FIXTURES) >= 5 and set(C.FIXTURES) <= set(C.NAMES)


@pytest.mark.parametrize('name', C.NAMES)
def test_starts(name):
    assert abs(C.error(C.start(name, 'near'), name) - 3.0) < 1e-6
    assert abs(C.error(C.start(name, 'far'), name) - 7.0) < 1e-6


@pytest.mark.parametrize('name', C.FIXTURES)
def test_fixture_condition_similarity(name):
    near = C.restated(name, 'near', 'similarity', 50, C.FIXTURE_EPS)
    far = C.restated(name, 'far', 'similarity', 50, C.FIXTURE_EPS)
    for r in (near, far):
        assert r['success'] and r['converged']
        print(name, 'similarity', C.error(r['transform'], name), r['nit'])
        assert C.error(r['transform'], name) <= C.SIMILARITY_CAP
    assert C.corner_distance(near['transform'], far['transform'], C.pair(name)[1].shape) <= C.SAME_POINT


@pytest.mark.parametrize('name', C.FIXTURES)
@pytest.mark.parametrize('model', ('affine', 'homography'))
def test_recorded_affine_and_homography(name, model):
    """No cap fixed in advance: ecc_cases.REACHED records what the restatement reaches, and this keeps the record true."""
    want = C.REACHED[name][1 if model == 'affine' else 2]
    near = C.restated(name, 'near', model, 50, C.FIXTURE_EPS)
    far = C.restated(name, 'far', model, 50, C.FIXTURE_EPS)
    for r in (near, far):
        assert r['success'] and r['converged']
        print(name, model, C.error(r['transform'], name), r['nit'])
        assert abs(C.error(r['transform'], name) - want) < 2e-3
    assert C.corner_distance(near['transform'], far['transform'], C.pair(name)[1].shape) <= C.SAME_POINT


def test_float32_terms_stay_close():
    """The restatement's float32 mode (what the kernel rounds) against float64: the noise floor the GPU test multiplies by 4."""
    for model in ('similarity', 'homography'):
        for maxiter in (1, 3, 10):
            f = C.noise_floor('small_thermal_far', 'near', model, maxiter)
            print(model, maxiter, f)
            assert 0.0 < f < 1e-2
