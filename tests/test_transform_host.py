"""Host tests of the similarity / affine estimators: the numpy restatement the GPU tests hold the kernels to (planted models,
the least-squares refit against np.linalg.lstsq, the round rule of the refinement), the few-inlier case the models exist for,
decompose_similarity, the configuration default, the two CLIs' parsers and report, and the C ABI's tables.  No GPU."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import yaml

import pooled_cases as C
import transform_cases as T
import transform_restatement as R
from multipoint_amd.utils import decompose_similarity, find_transform  # noqa: F401  (the feature under test)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LGHD_DIR = os.path.join(ROOT, 'tests', 'golden', 'lghd')
ENTRIES = ('mp_find_transform', 'mp_find_transform_f', 'mp_refine_transform', 'mp_refine_transform_f', 'mp_find_transform_pooled',
           'mp_refine_transform_pooled')


def test_exports():
    import multipoint_amd.utils as U
    for name in ('find_transform', 'refine_transform', 'find_transform_points', 'find_transform_pooled', 'refine_transform_pooled',
                 'estimate_shared_transform', 'decompose_similarity', 'compose_similarity'):
        assert hasattr(U, name), name
    assert U.TRANSFORM_MODELS == {'homography': 0, 'similarity': 1, 'affine': 2}
    assert [U.transform_min_inliers(m) for m in ('homography', 'similarity', 'affine')] == [4, 3, 4]
    with pytest.raises(ValueError, match='unknown transform model'):
        U.transform_model('rigid')


# ----------------------------------------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('outliers', [0.0, 0.5])
@pytest.mark.parametrize('model', T.MODELS)
def test_restatement_recovers_planted_models(model, outliers):
    """Noise-free data under a model with dyadic coefficients is exact in float32: the winner's refit is the planted matrix to
    fp64 rounding, and every clean correspondence is an inlier."""
    rng = np.random.default_rng(5)
    a, b = T.exact_points(rng, 200, model)
    bad = rng.random(200) < outliers
    b[bad] = np.stack([rng.integers(0, T.HW[1], bad.sum()), rng.integers(0, T.HW[0], bad.sum())], 1)
    H, mask = R.ransac_transform(a, b, model, 3.0, 256, 1, 0)
    assert H is not None and mask[~bad].all()
    clean = R.as_matrix(R.fit(model, a, b, ~bad))
    assert np.abs(clean - T.EXACT_MODELS[model]).max() < 1e-9
    if not mask[bad].any():                                 # (a chance hit within 3 px moves the fit: then only the clean fit is exact)
        assert np.abs(H - T.EXACT_MODELS[model]).max() < 1e-9
    assert C.corner_error(H, T.EXACT_MODELS[model], *T.HW) < (1e-9 if not mask[bad].any() else 1.0)


def test_restatement_minimal_solves_interpolate_their_sample():
    rng = np.random.default_rng(0)
    for model in T.MODELS:
        a, b, _, _ = C.planted_points(rng, 50, *T.HW, 0.0, hm=T.random_model(rng, model), integer=False)
        for t in range(20):
            idx = R.sample(3, 1, t, len(a), T.SAMPLE[model])
            assert len(set(idx)) == T.SAMPLE[model]
            m = R.minimal(model, a, b, idx)
            assert np.sqrt(R.error2(m, a[idx], b[idx])).max() < 1e-9
            if model == 'similarity':
                assert m[0] == m[4] and m[1] == -m[3]
    line = np.stack([np.arange(5.0), 2 * np.arange(5.0)], 1)
    assert R.minimal('affine', line, line, [0, 2, 4]) is None                       # collinear
    assert R.minimal('similarity', np.ones((3, 2)), line[:3], [0, 1]) is None       # coincident


@pytest.mark.parametrize('model', T.MODELS)
def test_refit_is_the_least_squares_solution(model):
    """fit() -- closed form on centred points / 3x3 normal equations on centred source points -- against np.linalg.lstsq on the
    design matrix of the same set (forward error, unknowns (a, b, tx, ty) / (a, b, tx, c, d, ty))."""
    rng = np.random.default_rng(11)
    for n in (T.SAMPLE[model] + 1, 8, 300):
        a, b, _, _ = C.planted_points(rng, n, *T.HW, 0.0, hm=T.random_model(rng, model), noise=0.5, integer=False)
        inl = np.ones(n, bool); inl[::5] = n < 8
        x, y = a[inl].T
        o, z = np.ones_like(x), np.zeros_like(x)
        if model == 'similarity':
            A = np.concatenate([np.stack([x, -y, o, z], 1), np.stack([y, x, z, o], 1)])
            p = np.linalg.lstsq(A, np.concatenate([b[inl, 0], b[inl, 1]]), rcond=None)[0]
            ref = np.array([p[0], -p[1], p[2], p[1], p[0], p[3]])
        else:
            A = np.stack([x, y, o], 1)
            ref = np.concatenate([np.linalg.lstsq(A, b[inl, 0], rcond=None)[0], np.linalg.lstsq(A, b[inl, 1], rcond=None)[0]])
        got = R.fit(model, a, b, inl)
        assert np.abs(got - ref).max() < 1e-9 * max(1.0, np.abs(ref).max())
        # the minimiser: no nearby model has a lower cost over the set
        cost = R.error2(got, a[inl], b[inl]).sum()
        for k in range(6):
            for d in (-1e-4, 1e-4):
                other = got.copy(); other[k] += d
                if model == 'similarity':
                    other[4], other[3] = other[0], -other[1]
                assert R.error2(other, a[inl], b[inl]).sum() >= cost


@pytest.mark.parametrize('model', T.MODELS)
def test_restated_refinement_rounds(model):
    rng = np.random.default_rng(2)
    a, b = T.exact_points(rng, 120, model)
    start = T.EXACT_MODELS[model].copy(); start[0, 2] += 2.0                      # 2 px off at every corner
    assert abs(C.corner_error(start, T.EXACT_MODELS[model], *T.HW) - 2.0) < 1e-12
    H0, m0, n0, c0, done0 = R.refine_transform(a, b, model, start, 3.0, 0)
    assert np.array_equal(H0, start) and n0 == 120 and done0 == 0 and c0[0] == c0[1] == pytest.approx(4.0 * 120)
    H, mask, n, cost, done = R.refine_transform(a, b, model, start, 3.0, 10)
    assert done == 1 and n == 120 and cost[1] <= cost[0] and cost[0] == pytest.approx(480.0) and cost[1] < 1e-18
    assert C.corner_error(H, T.EXACT_MODELS[model], *T.HW) < 1e-9
    H2, mask2, n2, cost2, _ = R.refine_transform(a, b, model, H, 3.0, 1)          # a fixed point
    assert np.array_equal(H2, H) and np.array_equal(mask2, mask) and cost2[0] == cost2[1]
    # with outliers and noise: the set grows or shrinks over the rounds, the cost over each round's set never rises
    a, b, bad, hm = C.planted_points(rng, 300, *T.HW, 0.4, hm=T.random_model(rng, model), integer=False)
    He, me = R.ransac_transform(a, b, model, 3.0, 64, 0, 0)
    Hr, mr, nr, cr, _ = R.refine_transform(a, b, model, He, 3.0, 10)
    assert nr >= me.sum() - 2 and cr[1] <= cr[0] and C.corner_error(Hr, hm, *T.HW) < 0.5
    for bad_input in (np.zeros((3, 3)), np.full((3, 3), np.nan), np.diag([1.0, 1.0, 0.0])):
        Hz, mz, nz, cz, _ = R.refine_transform(a, b, model, bad_input, 3.0, 3)
        assert not Hz.any() and not mz.any() and nz == 0 and not cz.any()


# ----------------------------------------------------------------------------------------------------------------------
# the case the models exist for (CPU; tests/test_gpu_transform.py runs the kernels on the same seeds)
# ----------------------------------------------------------------------------------------------------------------------
def test_few_inlier_seed_table():
    assert len(T.FEW_SEEDS) >= 4
    for seed, (k, _, _) in T.FEW_SEEDS.items():
        a, b, good, hm = T.few_inlier_points(seed)
        assert len(a) == T.FEW_N and good.sum() == k and 6 <= k <= 8


@pytest.mark.parametrize('seed', sorted(T.FEW_SEEDS))
def test_few_inliers_similarity_recovers_where_the_homography_fails(oracle, seed):
    """40 matches in a 120 x 160 frame, 6-8 of them correct (0.3 px noise): the 2-point similarity is within 1 px of the planted
    transform at the four corners; the 4-point homography of oracle.ransac_homography on the same lists, same T and seed, is
    more than 3 px off or finds nothing.  Planted data only."""
    a, b, good, hm = T.few_inlier_points(seed)
    Hs, ms = R.ransac_transform(a, b, 'similarity', T.FEW_THR, T.FEW_T, T.FEW_RANSAC_SEED, 0)
    es = C.corner_error(Hs, hm, *T.FEW_HW)
    Hh, _ = oracle.ransac_homography(a, b, T.FEW_THR, T.FEW_T, T.FEW_RANSAC_SEED, 0)
    eh = None if Hh is None else C.corner_error(Hh, hm, *T.FEW_HW)
    print('seed %d: %d inliers planted, similarity %.3f px, homography %s px' % (seed, good.sum(), es, eh))
    assert es < 1.0 and ms[good].sum() >= good.sum() - 1
    assert eh is None or eh > 3.0
    assert es == pytest.approx(T.FEW_SEEDS[seed][1], abs=2e-3)


# ----------------------------------------------------------------------------------------------------------------------
# decompose_similarity, configuration, parsers, report
# ----------------------------------------------------------------------------------------------------------------------
def test_decompose_similarity_round_trip():
    import multipoint_amd.utils as U
    rng = np.random.default_rng(3)
    for _ in range(20):
        angle, scale, dx, dy = rng.uniform(-3.1, 3.1), rng.uniform(0.3, 3.0), rng.normal(0, 30), rng.normal(0, 30)
        # the reference's own recomposition (align.py:210-211)
        M = np.array([[scale * np.cos(angle), scale * np.sin(angle), dx], [-scale * np.sin(angle), scale * np.cos(angle), dy], [0, 0, 1]])
        got = U.decompose_similarity(M * rng.uniform(0.5, 2.0))                   # (any h22)
        assert np.allclose(got, (angle, scale, dx, dy), rtol=0, atol=1e-12)
        assert np.allclose(U.compose_similarity(*got), M, rtol=0, atol=1e-12)
        # the reference's own decomposition (align.py:196-200) where its division is well conditioned
        if abs(np.cos(angle)) > 0.1:
            assert got[1] == pytest.approx(M[0, 0] / np.cos(np.arctan2(M[0, 1], M[0, 0])), rel=1e-12)
    assert U.decompose_similarity(np.eye(3)) == (0.0, 1.0, 0.0, 0.0)
    quarter = U.decompose_similarity([[0, -2, 1], [2, 0, 1], [0, 0, 1]])          # a = 0, b = 2: x' = -2y: angle -pi/2 in this convention
    assert quarter[0] == pytest.approx(-np.pi / 2) and quarter[1] == pytest.approx(2.0)
    with pytest.raises(ValueError):
        U.decompose_similarity(np.zeros((3, 3)))


def test_config_default_is_the_homography():
    for name in ('config_image_pair_dataset_prediction.yaml', 'config_hdf5_pair_prediction.yaml'):
        cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', name)))
        assert cfg['prediction'].get('transform_model', 'homography') == 'homography'


def test_cli_parsers():
    import estimate_initial_transform as E
    import predict_align_image_pair as P
    assert E.build_parser().parse_args(['-i', 'x']).transform == 'homography'
    assert P.build_parser().parse_args([]).transform is None                      # (None: prediction.transform_model decides)
    for m in ('homography', 'similarity', 'affine'):
        assert E.build_parser().parse_args(['-i', 'x', '--transform', m]).transform == m
        assert P.build_parser().parse_args(['--transform', m]).transform == m
    for parser, argv in ((E.build_parser(), ['-i', 'x', '--transform', 'rigid']), (P.build_parser(), ['--transform', 'rigid'])):
        with pytest.raises(SystemExit):
            parser.parse_args(argv)


def test_python_refusals_need_no_device():
    import multipoint_amd.utils as U
    for model, n in (('similarity', 1), ('affine', 2)):
        H, mask = U.find_transform_points(np.zeros((n, 2)), np.zeros((n, 2)), model)
        assert H is None and mask.shape == (n,) and not mask.any()
    with pytest.raises(ValueError, match='unknown transform model'):
        U.find_transform_points(np.zeros((5, 2)), np.zeros((5, 2)), 'rigid')
    with pytest.raises(ValueError, match='optical and'):
        U.find_transform_points(np.zeros((5, 2)), np.zeros((4, 2)), 'affine')
    with pytest.raises(ValueError, match='at most'):
        U.find_transform_points(np.zeros((3201, 2)), np.zeros((3201, 2)), 'affine')
    with pytest.raises(ValueError, match='rounds'):
        U.refine_transform(None, np.eye(3), 'similarity', rounds=-1)
    with pytest.raises(ValueError, match='reproj_threshold'):
        U.refine_transform(None, np.eye(3), 'similarity', reproj_threshold=0.0)
    with pytest.raises(ValueError, match='unknown transform model'):
        U.refine_alignment(_Mutual(), model='rigid')


class _Mutual:
    match_mode = 'mutual'


def _write_pairs(directory, n):
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    for i in range(n):
        Image.fromarray(np.full((8, 10), i, np.uint8)).save(os.path.join(directory, '%d_optical.png' % i))
        Image.fromarray(np.full((8, 8), i, np.uint16)).save(os.path.join(directory, '%d_thermal.png' % i))


def _fake_estimator(H, inliers_per_pair, matches_per_pair=6, seen=None):
    def estimator(args, config, names):
        if seen is not None:
            seen.append(args.transform)
        mask = np.concatenate([np.arange(matches_per_pair) < inliers_per_pair for _ in names])
        po = np.arange(len(names) + 1) * matches_per_pair
        return np.asarray(H, np.float64), mask.astype(np.uint8), po, int(mask.sum()), (12.5, 3.25)
    return estimator


def _args(directory, *extra):
    return ['-y', os.path.join(ROOT, 'configs', 'config_image_pair_dataset_prediction.yaml'), '-m', LGHD_DIR, '-v', 'none',
            '-i', str(directory)] + list(extra)


def test_initial_transform_report_and_yaml(tmp_path):
    import estimate_initial_transform as E
    import multipoint_amd.utils as U
    _write_pairs(tmp_path, 2)
    H = U.compose_similarity(0.1, 1.25, 7.0, -3.0)
    seen = []
    assert E.main(_args(tmp_path, '--transform', 'similarity'), estimator=_fake_estimator(H, 2, seen=seen)) == 0
    assert seen == ['similarity']
    report = json.load(open(tmp_path / 'initial_transform_report.json'))
    assert report['transform'] == 'similarity' and report['inliers'] == 4
    assert [report['similarity'][k] for k in ('angle', 'scale', 'dx', 'dy')] == pytest.approx([0.1, 1.25, 7.0, -3.0], abs=1e-12)
    got = np.array(yaml.safe_load(open(tmp_path / 'initial_transform.yaml'))['perspective'], np.float64)
    assert got.shape == (3, 3) and np.allclose(got @ H, np.eye(3), atol=1e-12) and got[2].tolist() == [0.0, 0.0, 1.0]
    assert E.main(_args(tmp_path, '--transform', 'affine', '--force'), estimator=_fake_estimator(H, 2)) == 0
    report = json.load(open(tmp_path / 'initial_transform_report.json'))
    assert report['transform'] == 'affine' and 'similarity' not in report
    # the fewest inliers: 3 for a similarity, 4 for the two others
    one = tmp_path / 'one'
    _write_pairs(one, 1)
    assert E.main(_args(one, '--transform', 'similarity'), estimator=_fake_estimator(H, 3)) == 0
    assert E.main(_args(one, '--transform', 'affine', '--force'), estimator=_fake_estimator(H, 3)) == 1
    assert E.main(_args(one, '--transform', 'similarity', '--force'), estimator=_fake_estimator(H, 2)) == 1
    assert E.main(_args(one, '--force'), estimator=_fake_estimator(H, 3)) == 1
    # the default report has no new key
    assert E.main(_args(one, '--force'), estimator=_fake_estimator(H, 5)) == 0
    assert not {'transform', 'similarity'} & set(json.load(open(one / 'initial_transform_report.json')))


# ----------------------------------------------------------------------------------------------------------------------
# C ABI tables
# ----------------------------------------------------------------------------------------------------------------------
def test_header_library_and_ctypes_table_agree():
    from multipoint_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'multipoint_hip.h')).read()
    for name, value in (('MP_MODEL_HOMOGRAPHY', 0), ('MP_MODEL_SIMILARITY', 1), ('MP_MODEL_AFFINE', 2)):
        assert re.search(r'#define %s %d\b' % (name, value), header)
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        decl = re.search(r'\bint %s\(([^;]*)\);' % name, header)
        assert decl, name
        params = [p.strip() for p in re.sub(r'/\*.*?\*/', '', decl.group(1), flags=re.S).split(',')]
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        assert hasattr(dll, name), name
        # `int model` sits behind the list / group sizes, in front of the threshold
        k = [i for i, p in enumerate(params) if p == 'int model']
        assert len(k) == 1 and params[k[0] + 1] == 'double reproj_threshold' and argtypes[k[0]] is ctypes.c_int
        assert argtypes[k[0] + 1] is ctypes.c_double
        counterpart = name.replace('transform', 'homography')
        assert len(_lib.SIGNATURES[counterpart][1]) == len(argtypes) - 1
        assert ('int rounds' in params) == ('refine' in name) and ('int max_iters' in params) == ('find' in name)
