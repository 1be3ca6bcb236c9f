"""CPU: the definition of the local residual field checked on its float64 restatement
(tests/residual_restatement.py) with planted pairs, the premises the GPU comparison rests on (the restatement's own float32
difference, the share of undetermined windows), and what of multipoint_amd.utils.residual needs no device: the summary, the
proposal and the argument checks."""
import ctypes
import math

import numpy as np
import pytest

import residual_cases as C
import residual_restatement as R
from multipoint_amd import _lib
from multipoint_amd.utils import residual as U


@pytest.fixture(scope='module')
def planted_fields():
    out = {}
    for kind in ('integer', 'fractional', 'two_region'):
        o, t, truth = C.planted(kind)
        out[kind] = (R.field(C.features(o, False), C.features(t, False), None, f32=False, **C.PARAMS), truth)
    return out


def test_vocabulary():
    assert (U.RES_OK, U.RES_FEW_VALID, U.RES_FLAT, U.RES_AT_EDGE) == (R.OK, R.FEW_VALID, R.FLAT, R.AT_EDGE)
    assert tuple(U.RESIDUAL_WINDOWS) == R.WINDOWS
    import multipoint_amd.utils as top
    assert top.residual_field is U.residual_field and top.propose_decision is U.propose_decision
    assert (U.RESIDUAL_THRESHOLDS['min_rho'], U.RESIDUAL_THRESHOLDS['min_margin']) == (C.MIN_RHO, C.MIN_MARGIN)
    assert U.VAR_FLOOR == C.PARAMS['var_floor'] == C.VAR_FLOOR


def test_integer_shift(planted_fields):
    f, truth = planted_fields['integer']
    conf = C.confident(f)
    assert conf.sum() >= C.MIN_CONFIDENT['integer']
    assert (np.rint(f['d'][conf]) == np.array([2.0, -3.0])).all()
    assert (np.abs(f['d'][conf] - np.array([2.0, -3.0])) < 0.5).all()
    assert (f['n'][conf] == 32 * 32).all()
    assert (f['rho'][conf] >= f['rho0'][conf]).all()


@pytest.mark.parametrize('kind', ['fractional', 'two_region'])
def test_fractional_shift(planted_fields, kind):
    f, truth = planted_fields[kind]
    errs, n, total = C.planted_errors(f, truth)
    print('%s: %d confident windows with a truth of %d, largest error %.4f px (recorded %.3f)' % (kind, n, total, errs.max(),
                                                                                                   C.REACHED[kind]))
    assert n >= C.MIN_CONFIDENT[kind]
    assert errs.max() <= C.PLANTED_MARGIN * C.REACHED[kind]


def test_two_regions_differ(planted_fields):
    f, _ = planted_fields['two_region']
    left, right = f['d'][:, 0], f['d'][:, -1]
    assert np.abs(left).max() < 0.25
    assert np.abs(right - np.array(C.TWO_REGION)).max() < 0.25


def test_flat_window():
    rng = np.random.RandomState(3)
    fo = rng.rand(40, 40).astype(np.float32)
    ft = rng.rand(40, 40).astype(np.float32)
    ft[:26, :26] = 0.5                                                 # the first window's template (origin 2, 2; w 24) is constant
    for f32 in (False, True):
        f = R.field(fo, ft, None, w=24, s=14, r=2, min_valid=0.5, var_floor=0.0, f32=f32)
        assert f['status'].shape == (1, 1)
        assert f['status'][0, 0] == R.FLAT and np.isnan(f['d'][0, 0]).all() and np.isnan(f['rho'][0, 0])
        assert f['n'][0, 0] == 24 * 24
    # a large variance floor declares every window flat
    f = R.field(fo, ft, None, w=8, s=8, r=2, min_valid=0.5, var_floor=10.0)
    assert (f['status'] == R.FLAT).all()


def test_few_valid():
    rng = np.random.RandomState(4)
    fo = rng.rand(24, 24).astype(np.float32)
    ft = rng.rand(24, 24).astype(np.float32)
    mask = np.ones((24, 24), np.uint8)
    mask[2:10, 2:7] = 0                                                # 40 of the first window's 64 pixels at d = 0: 24 stay, < 32
    f = R.field(fo, ft, mask, w=8, s=4, r=2, min_valid=0.5, var_floor=0.0)
    assert f['status'][0, 0] == R.FEW_VALID and f['n'][0, 0] == 24 and np.isnan(f['d'][0, 0]).all()
    mask[2:10, 6] = 1                                                  # 32 stay: exactly min_valid w^2 is enough
    f = R.field(fo, ft, mask, w=8, s=4, r=2, min_valid=0.5, var_floor=0.0)
    assert f['status'][0, 0] != R.FEW_VALID
    # a displacement whose own set is too small is undefined even when d = 0 is not: n is the count at the peak
    assert (f['n'][f['status'] != R.FEW_VALID] >= 32).all()


def test_shift_of_radius_is_at_edge():
    rng = np.random.RandomState(5)
    base = rng.rand(60, 60)
    fo = base[10:50, 10:50].astype(np.float32)
    ft = base[10 + 3:50 + 3, 10:50].astype(np.float32)                 # thermal[p] = optical[p + (3, 0)], r = 3
    f = R.field(fo, ft, None, w=16, s=8, r=3, min_valid=0.5, var_floor=0.0)
    assert (f['status'] == R.AT_EDGE).all()
    assert (f['d'][..., 0] == 3.0).all()                               # no refinement on the axis at the border
    assert (np.abs(f['d'][..., 1]) <= 0.5).all() and (f['rho'] > 0.999).all()


def test_tie_order():
    a = np.array([[0.1, 0.7], [0.4, 0.9]], np.float32)
    fo = np.tile(a, (12, 12))
    f = R.field(fo, fo.copy(), None, w=8, s=4, r=2, min_valid=0.5, var_floor=0.0)
    # period 2 in both axes: the nine even displacements tie at 1; the first in row-major order from -r wins
    assert (f['d'] == np.array([-2.0, -2.0])).all() and (f['status'] == R.AT_EDGE).all()
    assert (f['second'] == f['rho']).all() and (f['rho0'] == f['rho']).all()
    sc, cnt = R.scores(fo, fo, None, 2, 2, 8, 2, 0.5, 0.0, False)
    assert sc[0, 0] == sc[2, 2] == sc[4, 4] == sc[0, 4]


def test_restatement_float32_premises():
    """What the GPU comparison assumes of its reference: float32 products move no status or count, leave at most LEFT_OUT_CAP of a
    case's windows undetermined at DELTA, pick the same integer peak elsewhere, and move the sub-pixel terms by less than the
    recorded F32_DIFFERENCE."""
    worst_d = worst_s = 0.0
    seen = set()
    for shape in C.SHAPES:
        for kind in C.MASKS:
            a, b = C.restated(shape, kind, True), C.restated(shape, kind, False)
            assert (a['status'] == b['status']).all() and (a['n'] == b['n']).all(), (shape, kind)
            sel = C.decided(a)
            assert 1.0 - sel.mean() <= C.LEFT_OUT_CAP, (shape, kind)
            peak = sel & np.isin(a['status'], (R.OK, R.AT_EDGE))
            assert (np.rint(a['d'][peak]) == np.rint(b['d'][peak])).all(), (shape, kind)
            dd, ds = C.max_difference(a, b, sel)
            worst_d, worst_s = max(worst_d, dd), max(worst_s, ds)
            seen |= set(np.unique(a['status']).tolist())
    print('restatement f32 against float64: d %.3g px, scores %.3g' % (worst_d, worst_s))
    assert worst_d <= C.F32_DIFFERENCE['d'] and worst_s <= C.F32_DIFFERENCE['score']
    assert seen == {R.OK, R.FEW_VALID, R.FLAT, R.AT_EDGE}               # the cases reach every status


def _field(d, rho, second, status, rho0=None):
    d = np.asarray(d, np.float64)
    B, gy, gx = d.shape[:3]
    return {'d': d, 'rho': np.asarray(rho, np.float64), 'second': np.asarray(second, np.float64),
            'status': np.asarray(status), 'rho0': np.asarray(rho if rho0 is None else rho0, np.float64),
            'n': np.full((B, gy, gx), 64), 'origin': np.zeros((gy, gx, 2), np.int64), 'window': 8, 'stride': 8, 'radius': 2}


def test_summarize_hand_made():
    nan = float('nan')
    d = [[[[0.0, 0.0], [3.0, 4.0], [nan, nan], [0.0, 1.0]]],
         [[[nan, nan], [nan, nan], [nan, nan], [nan, nan]]]]
    rho = [[[0.9, 0.8, nan, 0.6]], [[nan, nan, nan, nan]]]
    second = [[[0.5, 0.2, nan, 0.58]], [[nan, nan, nan, nan]]]
    status = [[[0, 0, 2, 0]], [[1, 2, 2, 1]]]
    rho0 = [[[0.9, 0.1, nan, 0.5]], [[nan, nan, nan, nan]]]
    s = U.summarize_residual_field(_field(d, rho, second, status, rho0), min_rho=0.5, min_margin=0.05, tol_px=1.5)
    assert len(s) == 2
    a, b = s
    assert (a['windows'], a['confident'], a['at_edge']) == (4, 2, 0)    # window 3 misses the margin: 0.6 - 0.58 < 0.05
    assert a['coverage'] == 0.5 and a['median_d'] == [1.5, 2.0]
    assert a['median_mag'] == 2.5 and a['p90_mag'] == pytest.approx(4.5) and a['outlier_share'] == 0.5
    assert a['median_rho0'] == 0.5
    assert (b['windows'], b['confident'], b['coverage']) == (4, 0, 0.0)
    assert all(math.isnan(v) for v in (b['median_mag'], b['p90_mag'], b['outlier_share'], b['median_rho0'], *b['median_d']))
    # an AT_EDGE window counts in at_edge and is never confident
    e = U.summarize_residual_field(_field([[[[2.0, 0.0]]]], [[[0.99]]], [[[0.1]]], [[[3]]]))[0]
    assert (e['confident'], e['at_edge']) == (0, 1)
    assert not U.confident_windows(_field([[[[0.0, 0.0]]]], [[[0.99]]], [[[-np.inf]]], [[[1]]])).any()
    assert U.confident_windows(_field([[[[0.0, 0.0]]]], [[[0.99]]], [[[-np.inf]]], [[[0]]])).all()


def test_propose_decision():
    t = {'min_coverage': 0.25, 'accept_median_px': 1.0, 'accept_p90_px': 2.0, 'reject_median_px': 2.5}
    base = {'windows': 10, 'confident': 5, 'coverage': 0.5, 'median_mag': 0.3, 'p90_mag': 0.9}
    assert U.propose_decision(base, t) == 'a'
    assert U.propose_decision(dict(base, p90_mag=2.5), t) == '?'
    assert U.propose_decision(dict(base, median_mag=1.0, p90_mag=2.0), t) == 'a'
    assert U.propose_decision(dict(base, median_mag=2.5, p90_mag=3.0), t) == 'r'
    assert U.propose_decision(dict(base, median_mag=2.0, p90_mag=3.0), t) == '?'
    assert U.propose_decision(dict(base, coverage=0.2), t) == '?'       # featureless: never decided, whatever the residual
    assert U.propose_decision(dict(base, coverage=0.2, median_mag=9.0), t) == '?'
    nan = float('nan')
    assert U.propose_decision(dict(base, confident=0, coverage=0.0, median_mag=nan, p90_mag=nan), dict(t, min_coverage=0.0)) == '?'
    assert U.propose_decision(dict(base, median_mag=nan, p90_mag=nan), t) == '?'
    assert U.propose_decision(base) == 'a'                              # the defaults


def test_argument_refusals():
    lib = _lib.load_library()
    gy, gx = _lib.c_int(), _lib.c_int()

    def grid(H, W, w, s, r):
        return lib.mp_residual_grid(H, W, w, s, r, ctypes.byref(gy), ctypes.byref(gx))
    assert grid(96, 128, 32, 16, 8) == _lib.MP_OK and (gy.value, gx.value) == (4, 6)
    assert grid(33, 47, 8, 5, 3) == _lib.MP_OK and (gy.value, gx.value) == (4, 7)
    assert grid(48, 48, 32, 16, 8) == _lib.MP_OK and (gy.value, gx.value) == (1, 1)
    for args in ((47, 48, 32, 16, 8), (48, 47, 32, 16, 8), (96, 128, 20, 16, 8), (96, 128, 32, 0, 8), (96, 128, 32, 16, 9),
                 (96, 128, 32, 16, 0), (4097, 128, 32, 16, 8), (96, 4097, 32, 16, 8), (7, 7, 8, 1, 1)):
        assert grid(*args) == -1, args
        with pytest.raises(ValueError):
            R.grid(*args)
    for shape in C.SHAPES:
        assert grid(*shape) == _lib.MP_OK
        ys, xs = R.grid(*shape)
        assert (gy.value, gx.value) == (len(ys), len(xs)), shape
    for bad in (dict(window=20), dict(stride=0), dict(radius=9), dict(radius=0), dict(min_valid=0.0), dict(min_valid=1.5),
                dict(var_floor=-1.0), dict(var_floor=float('nan'))):
        kw = dict(window=32, stride=16, radius=8, min_valid=0.5, var_floor=0.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            U._check_parameters(**kw)
