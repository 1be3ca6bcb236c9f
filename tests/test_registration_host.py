"""Host checks of the Fourier-Mellin registration (no GPU): the planted fixtures meet the conditions the GPU tests build on, the
restatement's stages behave as specified, and estimate_initial_transform.py's --method handling and report."""
import functools
import json
import os

import numpy as np
import pytest
import yaml

import registration_cases as C
import registration_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORNER_BOUND = 1.0        # thermal px, restatement against the planted transform
RATIO_BOUND = 1.25        # peak over second, both stages


@functools.lru_cache(maxsize=None)
def _estimate(name):
    o, t, T = C.case(name)
    return R.estimate(o[None], t[None]), T


def test_there_are_at_least_six_cases_in_range():
    assert len(C.CASES) >= 6
    for seed, thw, ang, sc, sh in C.CASES.values():
        assert abs(ang) <= 10 and 0.75 <= sc <= 1.3 and max(abs(v) for v in sh) <= 20 and thw in ((96, 128), (72, 96))
    assert {c[1] for c in C.CASES.values()} == {(96, 128), (72, 96)}


@pytest.mark.parametrize('name', sorted(C.CASES))
def test_restatement_recovers_the_planted_transform(name):
    e, T = _estimate(name)
    err = C.corner_error(e['T'][0], T)
    r1 = e['pk1'][0]['peak'] / e['pk1'][0]['second']
    r2 = e['pk2'][0]['peak'] / e['pk2'][0]['second']
    print('%s: corner error %.3f px, ratios %.2f %.2f, branch %d' % (name, err, r1, r2, e['branch'][0]))
    assert err <= CORNER_BOUND
    assert r1 >= RATIO_BOUND and r2 >= RATIO_BOUND
    assert e['branch'][0] == 0


def test_group_and_shift_groups_meet_the_conditions():
    o, t, T = C.group_case()
    e = R.estimate(o, t, [0, 4])
    assert C.corner_error(e['T'][0], T) <= CORNER_BOUND
    assert min(e['pk1'][0]['peak'] / e['pk1'][0]['second'], e['pk2'][0]['peak'] / e['pk2'][0]['second']) >= RATIO_BOUND
    # pooled surfaces are the sums of the single-pair ones (numpy's inverse divides each by h w)
    singles = R.estimate(o, t)
    assert np.abs(e['surface1'][0] - singles['surface1'].sum(0)).max() <= 1e-12
    o, t, gid, T = C.shift_groups_case()
    go = np.searchsorted(gid, np.arange(4))
    e = R.estimate(o, t, go)
    for g in range(3):
        assert C.corner_error(e['T'][g], T[g]) <= CORNER_BOUND
        assert min(e['pk1'][g]['peak'] / e['pk1'][g]['second'], e['pk2'][g]['peak'] / e['pk2'][g]['second']) >= RATIO_BOUND


def test_stage_one_peak_is_minus_theta_and_log_scale():
    """The convention DESIGN 3.20 derives: the stage-1 peak of (optical, thermal) lies at (-theta A / pi, ln(s) / step)."""
    from multipoint_amd.utils.registration import logpolar_tables
    for name in ('same_size_scale_up', 'small_thermal_rot'):
        e, _ = _estimate(name)
        _, _, ang, sc, _ = C.CASES[name]
        step = logpolar_tables(e['N'], e['A'], e['R'])[4]
        sy, sx = e['pk1'][0]['signed']
        assert abs(sy - (-np.radians(ang) * e['A'] / np.pi)) <= 1.0 and abs(sx - np.log(sc) / step) <= 1.0


def test_prepare_identity_is_the_windowed_central_difference():
    from multipoint_amd.utils.registration import hann_table
    rng = np.random.RandomState(0)
    f = rng.rand(1, 9, 13).astype(np.float32)
    got = R.prepare(f, 16)[0]
    oy, ox = (16 - 9) // 2, (16 - 13) // 2
    win = got[oy:oy + 9, ox:ox + 13]
    assert np.count_nonzero(got) == np.count_nonzero(win)
    d = f[0].astype(np.float64)
    for y in range(9):
        for x in range(13):
            # every tap's bilinear footprint (x0, x0 + 1) must lie inside: x + 1 + 1 <= W - 1 and x - 1 >= 0
            if 1 <= x <= 13 - 3 and 1 <= y <= 9 - 3:
                want = np.hypot(0.5 * (d[y, x + 1] - d[y, x - 1]), 0.5 * (d[y + 1, x] - d[y - 1, x]))
                want *= float(hann_table(9)[y]) * float(hann_table(13)[x])
                assert abs(win[y, x] - want) <= 1e-15
            else:
                assert win[y, x] == 0.0


def test_cross_power_and_peak_rules():
    rng = np.random.RandomState(1)
    a = rng.randn(5, 4, 6) + 1j * rng.randn(5, 4, 6)
    b = rng.randn(5, 4, 6) + 1j * rng.randn(5, 4, 6)
    a[1, 2, 3] = 0.0
    x = R.cross_power(a, b, [0, 1, 4, 4, 5])
    assert x.shape == (4, 4, 6) and not x[2].any() and (x[:, 0, 0] == 0).all()
    assert np.abs(np.abs(x[0].reshape(-1)[1:]) - 1.0).max() <= 1e-12
    u = a[1:4] * np.conj(b[1:4])
    u[0, 2, 3] = 0.0
    want = (u / np.where(np.abs(u) > 0, np.abs(u), 1.0)).sum(0)
    want[0, 0] = 0.0
    assert np.abs(x[1] - want).max() <= 1e-12
    p = np.zeros((8, 8))
    p[0, 7] = p[5, 2] = 2.0           # a tie: the first in row-major order
    p[7, 0] = 1.5                     # inside the wrapped block of (0, 7)
    p[3, 3] = 1.0
    pk = R.peak(p)
    assert pk['index'] == (0, 7) and pk['peak'] == 2.0 and pk['second'] == 2.0 and pk['signed'][1] < 0
    p[5, 2] = 0.5
    assert R.peak(p)['second'] == 1.0
    q = np.zeros((3, 3))
    q[1, 1] = 1.0
    assert R.peak(q)['second'] == -np.inf and R.peak(q)['offset'] == (0.0, 0.0)
    # folding: index h / 2 stays, h / 2 + 1 becomes negative
    for idx, want in ((4, 4.0), (5, -3.0)):
        z = np.zeros((8, 8))
        z[idx, 0] = 1.0
        assert R.peak(z)['signed'][0] == want


# ---- estimate_initial_transform.py --method ----
def _write_pairs(directory, n):
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    for i in range(n):
        Image.fromarray(np.full((8, 10), i, np.uint8)).save(os.path.join(directory, '%d_optical.png' % i))
        Image.fromarray(np.full((8, 8), i, np.uint16)).save(os.path.join(directory, '%d_thermal.png' % i))


def _fake(H, peak1=0.5, second1=0.1, peak2=0.6, second2=0.2, branch=0, seen=None):
    def estimator(args, names):
        if seen is not None:
            seen.append((args.transform, list(names)))
        return np.asarray(H, np.float64), dict(peak1=peak1, second1=second1, peak2=peak2, second2=second2, branch=branch)
    return estimator


def _never(*a, **k):
    raise AssertionError('the other estimator must not run')


def test_method_flag_parsing():
    import estimate_initial_transform as E
    a = E.build_parser().parse_args(['-i', 'x'])
    assert a.method == 'matches' and a.transform == 'homography' and a.min_peak_ratio == 1.1
    a = E.build_parser().parse_args(['-i', 'x', '--method', 'fourier', '--min-peak-ratio', '1.5'])
    assert a.method == 'fourier' and a.min_peak_ratio == 1.5
    with pytest.raises(SystemExit):
        E.build_parser().parse_args(['-i', 'x', '--method', 'spectrum'])
    assert 'guess' in ' '.join(E.build_parser().format_help().split())


def test_fourier_report_yaml_and_refusals(tmp_path, capsys):
    import estimate_initial_transform as E
    import multipoint_amd.utils as U
    _write_pairs(tmp_path, 3)
    H = U.compose_similarity(-0.05, 0.8, 4.0, -2.5)
    seen = []
    base = ['-i', str(tmp_path), '--method', 'fourier', '-m', str(tmp_path / 'no_such_model_dir'), '-y', str(tmp_path / 'no_such.yaml')]
    # an explicit other model: exit status 2, nothing written, the estimator not called
    assert E.main(base + ['--transform', 'affine'], estimator=_never, fourier_estimator=_never) == 2
    assert E.main(base + ['--transform', 'homography'], estimator=_never, fourier_estimator=_never) == 2
    assert not (tmp_path / 'initial_transform.yaml').exists()
    # omitted or similarity: runs without a model directory or a config (no network is loaded)
    assert E.main(base, estimator=_never, fourier_estimator=_fake(H, seen=seen)) == 0
    assert seen == [('similarity', ['0', '1', '2'])]
    got = np.array(yaml.safe_load(open(tmp_path / 'initial_transform.yaml'))['perspective'], np.float64)
    assert np.allclose(got @ H, np.eye(3), atol=1e-12) and got[2].tolist() == [0.0, 0.0, 1.0]
    report = json.load(open(tmp_path / 'initial_transform_report.json'))
    assert report['method'] == 'fourier' and report['transform'] == 'similarity'
    assert report['pairs_read'] == report['pairs_used'] == 3 and report['branch_180'] is False
    assert [report['similarity'][k] for k in ('angle', 'scale', 'dx', 'dy')] == pytest.approx([-0.05, 0.8, 4.0, -2.5], abs=1e-12)
    assert report['stage1'] == {'peak': 0.5, 'second': 0.1, 'ratio': 5.0} and report['stage2']['ratio'] == pytest.approx(3.0)
    # an existing yaml is refused without --force
    written = (tmp_path / 'initial_transform.yaml').read_text()
    assert E.main(base, fourier_estimator=_never) == 2 and (tmp_path / 'initial_transform.yaml').read_text() == written
    assert E.main(base + ['--transform', 'similarity', '--force', '--max-pairs', '2'], fourier_estimator=_fake(H, branch=1)) == 0
    report = json.load(open(tmp_path / 'initial_transform_report.json'))
    assert report['pairs_used'] == 2 and report['branch_180'] is True
    # a ratio below the floor in either stage: exit status 1, nothing written
    for kw in (dict(second1=0.48), dict(second2=0.58), dict(peak1=0.0, second1=0.0)):
        out = tmp_path / 'low' / 'initial_transform.yaml'
        os.makedirs(tmp_path / 'low', exist_ok=True)
        assert E.main(base + ['-o', str(out)], fourier_estimator=_fake(H, **kw)) == 1
        assert os.listdir(tmp_path / 'low') == []
    assert E.main(base + ['-o', str(out), '--min-peak-ratio', '1.01'], fourier_estimator=_fake(H, second1=0.48)) == 0


def test_matches_method_is_untouched(tmp_path):
    """The default method: the report and the estimator's arguments as before (build_report keeps its signature)."""
    import inspect

    import estimate_initial_transform as E
    assert list(inspect.signature(E.build_report).parameters) == ['names_read', 'names_used', 'pair_offsets', 'mask', 'n_inliers',
                                                                    'cost', 'transform', 'H']
    _write_pairs(tmp_path, 2)
    seen = []

    def estimator(args, config, names):
        seen.append((args.method, args.transform))
        return np.eye(3), np.ones(12, np.uint8), np.array([0, 6, 12]), 12, (2.0, 1.0)
    argv = ['-y', os.path.join(ROOT, 'configs', 'config_image_pair_dataset_prediction.yaml'), '-m',
            os.path.join(ROOT, 'tests', 'golden', 'lghd'), '-v', 'none', '-i', str(tmp_path)]
    assert E.main(argv, estimator=estimator, fourier_estimator=_never) == 0
    assert seen == [('matches', 'homography')]
    report = json.load(open(tmp_path / 'initial_transform_report.json'))
    assert sorted(report) == ['cost_after_polish', 'cost_before_polish', 'inliers', 'inliers_per_pair', 'matches_pooled',
                              'pairs_read', 'pairs_used', 'pairs_with_4_inliers']
