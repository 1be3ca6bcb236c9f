"""CPU: the definition of the local alignment correction checked on its float64 restatement
(tests/field_restatement.py) -- the conjugate gradients against the dense solve, the robust rounds, the planted loop and the values
it reaches -- and what of multipoint_amd.utils.field needs no device: geometry, weights, the never-worse rule, the argument checks
and the binding."""
import ctypes
import os
import re

import numpy as np
import pytest

import field_cases as C
import field_restatement as F
from multipoint_amd import _lib
from multipoint_amd.utils import field as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('mp_field_fit_workspace', 'mp_field_fit', 'mp_field_warp')


def test_vocabulary():
    assert (U.FIELD_OK, U.FIELD_NO_DATA, U.FIELD_ALL_REJECTED, U.FIELD_MAX_ITER) == (F.OK, F.NO_DATA, F.ALL_REJECTED, F.MAX_ITER)
    import multipoint_amd.utils as top
    assert top.correct_locally is U.correct_locally and top.fit_displacement_field is U.fit_displacement_field
    assert top.warp_by_field is U.warp_by_field and top.field_geometry is U.field_geometry and top.field_weights is U.field_weights
    d = U.FIELD_DEFAULTS
    assert (d['smoothness'], d['min_initial_px'], d['keep_confident'], d['extrapolate']) == (C.SMOOTHNESS, C.MIN_INITIAL_PX,
                                                                                             C.KEEP_CONFIDENT, 'linear')
    assert d['rounds'] == C.ROUNDS


def test_header_and_signatures_agree():
    header = open(os.path.join(ROOT, 'include', 'multipoint_hip.h')).read()
    declared = set(re.findall(r'\b(mp_field_[a-z_0-9]+)\s*\(', header))
    assert declared == set(ENTRIES) == {k for k in _lib.SIGNATURES if k.startswith('mp_field_')}
    lib = _lib.load_library()
    for name in ENTRIES:
        assert hasattr(lib, name)
    for name, value in (('MP_FIELD_OK', F.OK), ('MP_FIELD_NO_DATA', F.NO_DATA), ('MP_FIELD_ALL_REJECTED', F.ALL_REJECTED),
                        ('MP_FIELD_MAX_ITER', F.MAX_ITER), ('MP_FIELD_INFO_INTS', 4)):
        assert re.search(r'#define %s %d\b' % (name, value), header), name


def test_workspace_entry_needs_no_device():
    lib = _lib.load_library()
    n = _lib.c_ll()
    assert lib.mp_field_fit_workspace(3, 4, 6, ctypes.byref(n)) == _lib.MP_OK and n.value == 3 * 24 * 7 * 8
    assert lib.mp_field_fit_workspace(1, 256, 256, ctypes.byref(n)) == _lib.MP_OK and n.value == 65536 * 7 * 8
    assert lib.mp_field_fit_workspace(65535, 256, 256, ctypes.byref(n)) == _lib.MP_OK and n.value == 65535 * 65536 * 56
    for args in ((0, 4, 6), (65536, 4, 6), (1, 0, 6), (1, 4, 257), (1, 257, 4), (1, 4, 0)):
        assert lib.mp_field_fit_workspace(*args, ctypes.byref(n)) == -1, args
    assert lib.mp_field_fit_workspace(1, 4, 6, None) == -1


@pytest.mark.parametrize('pattern', C.PATTERNS)
@pytest.mark.parametrize('lattice', C.LATTICES, ids=lambda l: '%dx%d' % l)
def test_pcg_against_dense(lattice, pattern):
    d, w, robust_px, rounds = C.lattice_case(lattice, pattern)
    refs = C.lattice_reference(lattice, pattern)
    for b in range(C.FRAMES):
        ref = refs[b]
        got = F.fit(d[b], w[b], C.SMOOTHNESS, robust_px, rounds, C.TOL, solver='pcg')
        assert got['status'] == ref['status'] and got['nonzero'] == ref['nonzero'] and got['nonfinite'] == ref['nonfinite']
        assert np.array_equal(got['weight'] > 0, ref['weight'] > 0)
        err = float(np.linalg.norm(got['u'] - ref['u']))
        assert err <= ref['bound'], (err, ref['bound'])
        assert np.isfinite(got['u']).all()
        if ref['status'] == F.NO_DATA:
            assert (got['u'] == 0).all() and got['iterations'] == 0
        else:
            assert got['residual'] <= C.TOL and got['iterations'] <= 4 * lattice[0] * lattice[1] + 64


def test_cases_reach_every_branch():
    seen = set()
    rejected = nonfinite = 0
    for lattice in C.LATTICES:
        for pattern in C.PATTERNS:
            d, w, robust_px, rounds = C.lattice_case(lattice, pattern)
            for ref in C.lattice_reference(lattice, pattern):
                seen.add(ref['status'])
                for wt, u, e in ref['solves']:
                    if e is not None:                                # no restated residual within 1e-9 of the threshold
                        assert (np.abs(e[ref['solves'][0][0] > 0] - robust_px) > 1e-9).all(), (lattice, pattern)
                if pattern == 'outlier' and lattice[0] * lattice[1] >= 12:
                    rejected += int(ref['nonzero'] < lattice[0] * lattice[1])
                if pattern == 'nan_under_zero':
                    nonfinite += ref['nonfinite']
    assert seen == {F.OK, F.NO_DATA, F.ALL_REJECTED}
    assert rejected >= 6 and nonfinite >= len(C.LATTICES)             # the outlier goes, the non-finite node is counted


def test_fit_properties():
    # a constant d comes back whatever the weights; a single weight spreads its value over the lattice
    w = np.zeros((3, 4))
    w[1, 2] = 0.3
    d = np.full((3, 4, 2), np.nan)
    d[1, 2] = (1.25, -0.5)
    r = F.fit(d, w, 0.25)
    assert np.allclose(r['u'], np.array([1.25, -0.5]), atol=1e-12) and r['nonzero'] == 1 and r['status'] == F.OK
    r = F.fit(d, np.zeros((3, 4)), 0.25)
    assert r['status'] == F.NO_DATA and (r['u'] == 0).all()
    # a larger smoothness flattens: the spread of u falls
    d2, w2, _, _ = C.lattice_case((4, 6), 'ones')
    assert np.ptp(F.fit(d2[0], w2[0], 4.0)['u'][..., 0]) < np.ptp(F.fit(d2[0], w2[0], 0.05)['u'][..., 0])
    # max_iter 1 cannot meet the rule on a real lattice
    assert F.fit(d2[0], w2[0], 0.25, solver='pcg', max_iter=1)['status'] == F.MAX_ITER
    A = F.system(np.ones((4, 6)), 0.25)
    print('condition number of the 4 x 6 system at smoothness 0.25: %.2f' % np.linalg.cond(A))
    assert np.allclose(A, A.T) and np.linalg.cond(A) < 4.0


def test_interpolation_and_extrapolation():
    u = np.zeros((2, 3, 2))
    u[..., 0] = [[0.0, 1.0, 2.0], [2.0, 3.0, 4.0]]                     # linear: 1 per node in x, 2 per node in y
    geo = (4.0, 8.0, 16.0)
    ys, xs = np.array([4.0, 12.0, 20.0, 36.0, -12.0]), np.array([8.0, 16.0, 40.0, 56.0, -8.0])
    lin, _ = F.interpolate(u, geo, ys, xs, 1)
    want = 2.0 * (ys[:, None] - 4.0) / 16.0 + (xs[None] - 8.0) / 16.0
    assert np.allclose(lin, want, atol=1e-12)                        # linear extrapolation continues a linear field
    cl, _ = F.interpolate(u, geo, ys, xs, 0)
    assert cl.max() == 4.0 and cl.min() == 0.0 and cl[4, 4] == 0.0 and cl[3, 3] == 4.0
    one, _ = F.interpolate(np.full((1, 1, 2), 0.75), geo, ys, xs, 1)
    assert (one == 0.75).all()                                       # a 1 x 1 lattice is a constant, whatever the mode


def test_warp_identity_and_validity():
    rng = np.random.RandomState(2)
    src = rng.uniform(0.1, 1.0, (12, 20)).astype(np.float32)
    dst, valid = F.warp(src, np.zeros((2, 2, 2)), (2.0, 3.0, 8.0))
    assert dst.tobytes() == src.tobytes() and (valid == 1).all()
    dst, valid = F.warp(src, np.full((1, 1, 2), 0.5), (0.0, 0.0, 4.0))
    assert (valid[-1] == 0).all() and (valid[:, -1] == 0).all() and (valid[:-1, :-1] == 1).all()
    h = np.float32(0.5)
    assert dst[3, 4] == (src[3, 4] * h + src[3, 5] * h) * h + (src[4, 4] * h + src[4, 5] * h) * h
    bad = np.eye(3)
    bad[2] = [0, 0, -1.0]
    dst, valid = F.warp(src, np.zeros((1, 1, 2)), (0.0, 0.0, 4.0), hom=bad)
    assert (dst == 0).all() and (valid == 0).all()
    dst, valid = F.warp(src, np.full((1, 1, 2), np.inf), (0.0, 0.0, 4.0))
    assert (dst == 0).all() and (valid == 0).all()


def _field(d, rho, second, status, window=32, stride=16, origin=(8, 8)):
    d = np.asarray(d, np.float64)
    B, gy, gx = d.shape[:3]
    ys, xs = origin[0] + stride * np.arange(gy), origin[1] + stride * np.arange(gx)
    return {'d': d, 'rho': np.asarray(rho, np.float64), 'second': np.asarray(second, np.float64), 'status': np.asarray(status),
            'rho0': np.asarray(rho, np.float64), 'n': np.full((B, gy, gx), 64),
            'origin': np.stack(np.meshgrid(ys, xs, indexing='ij'), -1), 'window': window, 'stride': stride, 'radius': 8}


def test_geometry_and_weights():
    f = _field(np.zeros((1, 1, 3, 2)), [[[0.9, 0.6, 0.9]]], [[[0.1, 0.58, 0.2]]], [[[0, 0, 3]]])
    assert U.field_geometry(f) == (8 + 15.5, 8 + 15.5, 16.0)
    assert U.field_geometry(_field(np.zeros((1, 2, 2, 2)), np.ones((1, 2, 2)), np.zeros((1, 2, 2)), np.zeros((1, 2, 2), int), 24, 7,
                                   (2, 5))) == (13.5, 16.5, 7.0)
    assert U.field_weights(f, 0.5, 0.05).tolist() == [[[1.0, 0.0, 0.0]]]      # margin missed; at the edge
    assert U.field_weights(f, 0.5, 0.05, 'rho').tolist() == [[[0.9, 0.0, 0.0]]]
    assert U.field_weights(f, 0.5, 0.01, 'rho').tolist() == [[[0.9, 0.6, 0.0]]]
    assert U.field_weights(f).dtype == np.float64
    with pytest.raises(ValueError):
        U.field_weights(f, mode='soft')
    assert C.geometry({'origin': np.array([[[8, 8]]])}) == (23.5, 23.5, 16.0)


def test_never_worse_every_branch():
    first = {'windows': 24, 'confident': 20, 'coverage': 20 / 24, 'median_mag': 1.4}
    final = {'windows': 24, 'confident': 20, 'coverage': 20 / 24, 'median_mag': 0.02}
    kw = dict(min_coverage=0.25, min_initial_px=0.25, keep_confident=0.8)
    nan = float('nan')
    assert U.never_worse(first, final, **kw) == (True, 'applied')
    assert U.never_worse(dict(first, coverage=0.2), final, **kw) == (False, 'coverage')
    assert U.never_worse(dict(first, confident=0, coverage=0.0, median_mag=nan), final, **kw) == (False, 'coverage')
    assert U.never_worse(dict(first, coverage=0.25), final, **kw) == (True, 'applied')          # reaching it is enough
    assert U.never_worse(dict(first, median_mag=0.2), final, **kw) == (False, 'aligned')
    assert U.never_worse(dict(first, median_mag=0.25), dict(final, median_mag=0.1), **kw) == (True, 'applied')
    assert U.never_worse(dict(first, median_mag=nan), final, **kw) == (False, 'aligned')
    assert U.never_worse(first, dict(final, median_mag=1.4), **kw) == (False, 'not_improved')   # equal is not smaller
    assert U.never_worse(first, dict(final, median_mag=1.6), **kw) == (False, 'not_improved')
    assert U.never_worse(first, dict(final, median_mag=nan, confident=0), **kw) == (False, 'not_improved')
    assert U.never_worse(first, dict(final, confident=15), **kw) == (False, 'lost_windows')
    assert U.never_worse(first, dict(final, confident=16), **kw) == (True, 'applied')           # exactly 0.8 of 20
    assert U.never_worse(first, final) == (True, 'applied')                                      # the defaults


def test_argument_checks():
    ok = dict(smoothness=0.25, robust_px=None, rounds=2, tol=1e-12, max_iter=None, nodes=24)
    assert U._check_fit(**ok) == (0.25, 0.0, 2, 1e-12, 4 * 24 + 64)
    assert U._check_fit(**dict(ok, nodes=1 << 20))[4] == 1 << 20
    for bad in (dict(smoothness=0.0), dict(smoothness=float('inf')), dict(smoothness=float('nan')), dict(robust_px=-1.0),
                dict(robust_px=float('nan')), dict(rounds=17), dict(rounds=-1), dict(tol=-1e-3), dict(tol=float('inf')),
                dict(max_iter=0), dict(max_iter=(1 << 20) + 1)):
        with pytest.raises(ValueError):
            U._check_fit(**dict(ok, **bad))


@pytest.mark.parametrize('kind', ['smooth', 'two_region'])
def test_planted_loop_on_the_restatement(kind):
    """Where the planted bounds are measured: the restated loop's first and final median residual and, for the smooth field, its
    error at the nodes, against the values recorded in field_cases.REACHED."""
    summaries, Uacc, geo = C.restated_loop(kind)
    first, final = summaries[0], summaries[-1]
    rec = C.REACHED[kind]
    print('%s: median residual by round %s px, confident %s (recorded first %.3f, final %.4f)' % (
        kind, ['%.4f' % s['median_mag'] for s in summaries], [s['confident'] for s in summaries], rec['first'], rec['final']))
    assert first['confident'] == final['confident'] == 24
    assert abs(first['median_mag'] - rec['first']) < 0.01
    assert final['median_mag'] <= C.PLANTED_MARGIN * rec['final']
    assert U.never_worse(first, final, C.MIN_COVERAGE, C.MIN_INITIAL_PX, C.KEEP_CONFIDENT) == (True, 'applied')
    truth = C.planted(kind)[2]
    if truth is not None:
        err = C.field_error(Uacc, geo, truth)
        print('%s: median field error at the nodes %.4f px (recorded %.4f)' % (kind, err, rec['error']))
        assert err <= C.PLANTED_MARGIN * rec['error']


def test_planted_loop_leaves_aligned_and_featureless_alone():
    s = C.restated_loop('aligned')[0]
    assert U.never_worse(s[0], s[-1], C.MIN_COVERAGE, C.MIN_INITIAL_PX, C.KEEP_CONFIDENT) == (False, 'aligned')
    s = C.restated_loop('featureless')[0]
    assert s[0]['confident'] == 0
    assert U.never_worse(s[0], s[-1], C.MIN_COVERAGE, C.MIN_INITIAL_PX, C.KEEP_CONFIDENT) == (False, 'coverage')
