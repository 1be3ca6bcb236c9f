"""CPU: the restatement of the frame preparation (tests/frames_restatement.py) against what does not depend on OpenCV -- numpy's
own percentile and assignment, the identity map, a physics anchor through the distortion model, the geometry of the new camera
matrix -- and against tests/golden/frames.npz, the reference's own preprocess_images run over the restated cv2 calls
(tests/golden/make_golden_frames.py).  The GPU tests hold the kernels to this restatement bit for bit."""
import os

import numpy as np
import pytest
import yaml

import frames_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'frames.npz')
SHAPES = [(24, 32), (37, 53), (64, 80)]


def test_identity_map_copies_both_types():
    for H, W in SHAPES + [(1, 9), (9, 1)]:
        K = R.test_camera(H, W)
        bgr, u16 = R.noise_bgr8(1, H, W), R.noise_u16(2, H, W)
        assert np.array_equal(R.undistort(bgr, K, R.DISTORTIONS[0], K), bgr)
        assert np.array_equal(R.undistort(u16, K, R.DISTORTIONS[0], K), u16)
        assert np.array_equal(R.undistort(u16, K, R.DISTORTIONS[0], K, rotate180=True), u16[::-1, ::-1])
        assert np.array_equal(R.resize_bgr8(bgr, (H, W)), bgr)


def test_coefficient_count():
    K = R.test_camera(8, 8)
    for n in (3, 6, 8):
        with pytest.raises(ValueError):
            R.undistort(R.noise_u16(1, 8, 8), K, np.zeros(n), K)
    four = R.undistort(R.noise_u16(1, 8, 8), K, (0.1, 0.01, 1e-3, 1e-3), K)
    assert np.array_equal(four, R.undistort(R.noise_u16(1, 8, 8), K, (0.1, 0.01, 1e-3, 1e-3, 0.0), K))


@pytest.mark.parametrize('name', ['fractional_bounds', 'constant', 'rank_on_element', 'noise_33x47', 'all_65535'])
def test_percentile_path_is_numpys(name):
    x = R.rescale_cases()[name]
    lower, upper = R.percentile_bounds(x)
    assert lower == np.percentile(x, 1) and upper == np.percentile(x, 99)
    if name == 'fractional_bounds':
        assert lower != int(lower) and upper != int(upper)
    if name == 'rank_on_element':
        flat = np.sort(x.reshape(-1))
        assert R.percentile_ranks(x.size, 1 / 100)[2] == 0.0 and lower == flat[2] and upper == flat[198]
    # the clip as the reference writes it: float64 bounds assigned into the uint16 array
    ref = x.copy()
    ref[ref < np.percentile(x, 1)] = np.percentile(x, 1)
    ref[ref > np.percentile(x, 99)] = np.percentile(x, 99)
    clipped, rescaled, saved = R.thermal_rescale(x)
    assert clipped.dtype == np.uint16 and np.array_equal(clipped, ref)
    assert np.array_equal(saved, (rescaled * 65535).astype('uint16'))
    # after the clip the extremes are the truncated bounds (what csrc/frames.hip relies on)
    assert clipped.min() == int(lower) and clipped.max() == int(upper)
    if name in ('constant', 'all_65535'):
        assert not rescaled.any() and not saved.any() and not np.signbit(rescaled).any()
    else:
        assert rescaled.min() >= -1e-6 and abs(float(rescaled.max()) - 1.0) < 1e-6
    # the normalisation against float64
    if clipped.max() > clipped.min():
        exact = (clipped.astype(np.float64) - clipped.min()) / (float(clipped.max()) - float(clipped.min()))
        span = float(clipped.max()) / (float(clipped.max()) - float(clipped.min()))
        assert np.abs(rescaled - exact).max() <= 4 * 2.0 ** -24 * max(span, 1.0)      # three fp32 roundings of values <= span
    # without outlier rejection: nothing is clipped
    plain, rescaled0, _ = R.thermal_rescale(x, outlier_rejection=False)
    assert np.array_equal(plain, x)
    if x.max() > x.min():
        assert rescaled0.min() >= -1e-6 and abs(float(rescaled0.max()) - 1.0) < 1e-6


def _inverse_map(K, D, u, v):
    """distorted pixel -> undistorted pixel (K_new = K), iterated to convergence"""
    x, y = R.undistort_points_normalised(u, v, K, D, iterations=200)
    return K[0, 0] * x + K[0, 2], K[1, 1] * y + K[1, 2]


@pytest.mark.parametrize('dtype', ['bgr8', 'u16'])
@pytest.mark.parametrize('D', R.DISTORTIONS[1:])
def test_physics_anchor(dtype, D):
    """A pattern f, rendered through the distortion model into the camera's frame and undistorted with K_new = K, must give f
    back on the pixel grid.  With h = f o N the rendered frame as a function of the distorted position (N: distorted ->
    undistorted pixel), the bilinear tap at a position quantised to 1/32 pixel differs from f by at most

        sqrt(2) / 64 * max|grad h|  +  (max|h_xx| + max|h_yy|) / 8  +  0.5 (rendered frame rounded)  +  0.5 (result rounded)

    with |grad h| <= L G, |h_ii| <= L^2 F + G C: G = max|grad f| and F = max|f''| analytic, L = max|J_N| and C = max|N_ii| from
    finite differences of the camera model (a safety factor 1.1 on both).  Nothing here is measured on the code under test."""
    H, W = 48, 64
    K = R.test_camera(H, W)
    amp, mid = (100.0, 127.5) if dtype == 'bgr8' else (25000.0, 32000.0)
    a, b = 0.12, 0.09
    phases = [(0.3, 1.1), (2.0, 0.4), (4.1, 2.9)] if dtype == 'bgr8' else [(0.7, 1.9)]

    def f(u, v):
        return np.stack([mid + amp * np.sin(a * u + p) * np.cos(b * v + q) for p, q in phases], -1)
    G, F = amp * np.sqrt(a * a + b * b), amp * (a * a + b * b)
    # the camera model's inverse map on a half-pixel grid over the frame and one pixel around it
    step = 0.5
    gv, gu = np.mgrid[-1:H + step:step, -1:W + step:step]
    nu, nv = _inverse_map(K, D, gu, gv)
    d1 = [np.gradient(n, step) for n in (nu, nv)]                                   # [d/dv, d/du] of each component
    L = 1.1 * np.sqrt(sum(g ** 2 for pair in d1 for g in pair)).max()
    d2 = [[np.gradient(pair[0], step, axis=0), np.gradient(pair[1], step, axis=1)] for pair in d1]
    C = 1.1 * max(np.sqrt(d2[0][k] ** 2 + d2[1][k] ** 2).max() for k in (0, 1))
    bound = np.sqrt(2) / 64 * L * G + 2 * (L * L * F + G * C) / 8 + 0.5 + 0.5 + (0.02 if dtype == 'u16' else 0.0)
    assert bound < 0.1 * amp                                                        # (the bound means something)
    # render, undistort, compare
    sv, su = np.mgrid[0:H, 0:W].astype(np.float64)
    rendered = f(*_inverse_map(K, D, su, sv))
    assert rendered.min() >= 0 and rendered.max() <= (255 if dtype == 'bgr8' else 65535)
    frame = np.rint(rendered).astype(np.uint8) if dtype == 'bgr8' else np.rint(rendered[..., 0]).astype(np.uint16)
    out = R.undistort(frame, K, D, K).astype(np.float64).reshape(H, W, -1)
    sx, sy, _, _ = R.undistort_taps(K, D, K, H, W)
    inside = (sx >= 0) & (sx + 1 < W) & (sy >= 0) & (sy + 1 < H)
    assert inside.mean() > 0.6
    err = np.abs(out - f(su, sv))[inside].max()
    print('physics anchor %s D=%s: error %.3f, bound %.3f (L %.3f, C %.4f)' % (dtype, D[:2], err, bound, L, C))
    assert err <= bound


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('D', R.DISTORTIONS)
def test_optimal_new_camera_matrix_geometry(shape, D):
    H, W = shape
    K = R.test_camera(H, W)
    # alpha = 0: every destination pixel looks inside the source frame.  The grid spans (0, 0) .. (w, h), so that frame is
    # [0, w] x [0, h], one pixel wider than the pixel centres: towards the far edges a tap can fall on column w or row h and
    # read the border, never beyond, and none does at the near edges.  A position within half a step of the 1/32-pixel
    # quantisation of an edge is quantised onto it.
    K0 = R.optimal_new_camera_matrix(K, D, (W, H), 0)
    us, vs = R.source_position(K, D, K0, H, W)
    tol = 1 / 64
    assert us.min() >= -tol and us.max() <= W + tol and vs.min() >= -tol and vs.max() <= H + tol
    sx, sy, ax, ay = R.undistort_taps(K, D, K0, H, W)
    assert sx.min() >= 0 and sy.min() >= 0 and sx.max() <= W and sy.max() <= H
    # alpha = 1: every corner pixel of the source frame lies inside the destination frame (its undistorted position by the
    # same five iterations; float64 rounding of a dozen operations on values below 1e3)
    K1 = R.optimal_new_camera_matrix(K, D, (W, H), 1)
    cu, cv = np.array([0.0, W - 1, 0.0, W - 1]), np.array([0.0, 0.0, H - 1, H - 1])
    x, y = R.undistort_points_normalised(cu, cv, K, D)
    du, dv = K1[0, 0] * x + K1[0, 2], K1[1, 1] * y + K1[1, 2]
    assert du.min() >= -1e-9 and du.max() <= W - 1 + 1e-9 and dv.min() >= -1e-9 and dv.max() <= H - 1 + 1e-9
    # in between the entries are interpolated
    Kh = R.optimal_new_camera_matrix(K, D, (W, H), 0.25)
    assert np.allclose(Kh, 0.75 * K0 + 0.25 * K1, rtol=1e-14, atol=0)
    if not any(D):
        assert np.allclose(K0, K1, rtol=1e-12)


def test_package_camera_matrix_is_the_restatement():
    from multipoint_amd.utils import frames
    for (H, W) in SHAPES:
        K = R.test_camera(H, W)
        for D in R.DISTORTIONS:
            for alpha in (0, 1, 0.4):
                assert np.array_equal(frames.optimal_new_camera_matrix(K, D, (W, H), alpha),
                                      R.optimal_new_camera_matrix(K, D, (W, H), alpha))
    with pytest.raises(ValueError):
        frames.optimal_new_camera_matrix(K, np.zeros(6), (W, H), 0)
    with pytest.raises(ValueError):
        frames.optimal_new_camera_matrix(np.eye(2), np.zeros(4), (W, H), 0)
    K, D = frames.camera_from_calibration(R.calibration_of([('thermal', R.DISTORTIONS[2])], (4, 4), (24, 32)), 'thermal')
    assert np.array_equal(K, R.test_camera(24, 32)) and tuple(D) == R.DISTORTIONS[2]


def test_resize_weights():
    for n_in, n_out in [(52, 34), (53, 34), (36, 24), (32, 32), (7, 2), (9, 3), (1, 4), (5, 9)]:
        i, a0, a1 = R.resize_axis(n_in, n_out)
        assert ((a0 + a1) == 2048).all() and i.min() >= 0 and i.max() <= n_in - 1
        assert (a1[i == n_in - 1] == 0).all()
    flat = np.full((9, 7, 3), 200, np.uint8)
    assert (R.resize_bgr8(flat, (3, 2)) == 200).all()
    ramp = np.broadcast_to((np.arange(52) * 4)[None, :, None], (36, 52, 3)).astype(np.uint8)
    out = R.resize_bgr8(ramp, (24, 34)).astype(np.float64)
    centre = ((np.arange(34) + 0.5) * 52 / 34 - 0.5) * 4
    assert np.abs(out[:, 1:-1, 0] - centre[None, 1:-1]).max() <= 1.0          # 11-bit weights and two roundings


def test_golden_fixture():
    """The restatement's prepare_frames against the reference's own preprocess_images (sequencing, aliasing, size arithmetic)."""
    z = np.load(GOLDEN)
    assert len(z['case_names']) == 2
    for name in z['case_names']:
        optical, thermal, params, calibration, want = R.golden_case(z, str(name))
        got = R.prepare_frames(optical, thermal, params, calibration)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.shape == w.shape
            assert np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)
        # the raw thermal frame the reference returns is the CLIPPED one
        assert want[1].min() == int(R.percentile_bounds(_thermal_before_clip(thermal, params, calibration))[0])


def _thermal_before_clip(thermal, params, calibration):
    from multipoint_amd.utils.frames import camera_from_calibration
    K, D = camera_from_calibration(calibration, 'thermal')
    out = R.undistort(thermal, K, D, R.optimal_new_camera_matrix(K, D, thermal.shape[::-1], params['image/undistort_alpha']))
    return out[::-1, ::-1] if params['image/thermal/rotate'] else out


def test_unknown_camera_label():
    calibration = R.calibration_of([('optical', R.DISTORTIONS[1]), ('lidar', R.DISTORTIONS[1])], (12, 16), (12, 16))
    params = {'undistort_images': True, 'image/undistort_alpha': 0.0, 'image/thermal/rotate': False,
              'image/optical/downscale': False, 'image/thermal/rescale_outlier_rejection': True}
    with pytest.raises(ValueError, match='ERROR unknown camera label: lidar'):
        R.prepare_frames(R.noise_bgr8(1, 12, 16), R.noise_u16(2, 12, 16), params, calibration)


def test_config_and_cli_surface():
    import prepare_images
    with open(os.path.join(ROOT, 'configs', 'config_prepare_images.yaml'), 'rt') as fh:
        params = yaml.safe_load(fh)
    for key in ('undistort_images', 'image/undistort_alpha', 'image/calibration_params', 'image/optical/downscale',
                'image/thermal/rotate', 'image/thermal/rescale_outlier_rejection'):
        assert key in params
    args = prepare_images.build_parser().parse_args(['-y', 'c.yaml', '-i', 'in', '-o', 'out'])
    assert (args.yaml_config, args.input_dir, args.output_dir, args.batch) == ('c.yaml', 'in', 'out', 16)
    assert [prepare_images.index_key(i) for i in ('10', '9', 'a')] == [(0, 10, '10'), (0, 9, '9'), (1, 0, 'a')]
