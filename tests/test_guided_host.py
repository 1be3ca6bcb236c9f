"""CPU: the float64 yardstick of the guided matcher and its planted inputs (tests/guided_restatement.py), and the host-side
surface of the alignment refinement -- mode checks, configuration parsing and argument errors, all of which are decided
before anything is launched (no GPU is touched)."""
import numpy as np
import pytest
import torch

import guided_restatement as R
from multipoint_amd.pipeline import PairResults


@pytest.mark.parametrize('D', R.WIDTHS)
def test_infinite_radius_is_the_plain_mutual_matcher(D):
    for case in range(len(R.PAIRS)):
        pr = R.make_pair(D, case)
        got, _, _ = R.guided_mutual(pr['A'], pr['B'], pr['kpA'], pr['kpB'], pr['H'], np.inf, D)
        assert np.array_equal(got, R.plain_mutual(pr['A'], pr['B'])), (D, case)


@pytest.mark.parametrize('D', R.WIDTHS)
def test_input_conditions_hold_for_every_seed(D):
    """What the GPU tests rely on: no (i, j) distance within 5e-4 px of a radius (the fp32 gate decides like the float64
    one), at most 2 % ambiguous rows, and the construction makes its point -- the plain mutual matcher loses the partners
    that have a distractor, the gated one finds them."""
    for case, (N, M) in enumerate(R.PAIRS):
        pr = R.make_pair(D, case)
        assert len(np.unique(pr['kpA'], axis=0)) == N
        assert pr['kpA'].min(initial=10) >= 10 and (pr['kpA'] < np.array(R.FRAME) - 10 + 1).all()
        plain = R.plain_mutual(pr['A'], pr['B'])
        t = pr['true']
        assert len(t) == min(N, M) // 2
        for radius in R.RADII:
            margin, amb = R.input_conditions(pr, D, radius)
            print('D %d case %d radius %g: nearest distance to the radius %.3g px, %.2f %% ambiguous' % (D, case, radius, margin,
                                                                                                        100 * amb))
            assert margin >= R.MIN_RADIUS_MARGIN
            assert amb <= R.MAX_AMBIGUOUS
            got, _, _ = R.guided_mutual(pr['A'], pr['B'], pr['kpA'], pr['kpB'], pr['H'], radius, D)
            if len(t) >= 8:
                found = int((got[t[:, 0]] == t[:, 1]).sum()); found_plain = int((plain[t[:, 0]] == t[:, 1]).sum())
                assert found >= 0.9 * len(t) and found >= 1.5 * found_plain


def test_zero_homography_gates_everything_out():
    pr = R.make_pair(64, 0)
    got, _, _ = R.guided_mutual(pr['A'], pr['B'], pr['kpA'], pr['kpB'], np.zeros((3, 3)), 6.0, 64)
    assert (got == -1).all()


def _empty(mode):
    return PairResults(None, None, None, None, None, None, None, 0, 0, mode)


def test_pair_metrics_takes_guided_lists():
    import multipoint_amd.utils as U
    assert _empty('guided').match_mode == 'guided'
    with pytest.raises(Exception) as e:                # past the mode check: fails on the empty results' missing tensors
        U.pair_metrics(_empty('guided'), None, 4.0)
    assert not isinstance(e.value, ValueError) and 'mutual' not in str(e.value)
    for mode in ('nearest', 'ratio'):
        with pytest.raises(ValueError, match='mutual'):
            U.pair_metrics(_empty(mode), None, 4.0)


def test_refinement_config_parsing():
    from multipoint_amd.utils.evaluation import _refinement_config
    assert _refinement_config({}) is None
    assert _refinement_config({'alignment_refinement': None}) is None
    assert _refinement_config({'alignment_refinement': {'enable': False, 'radius': 5, 'rounds': 2, 'polish': False}}) is None
    assert _refinement_config({'alignment_refinement': {'radius': 5}}) is None                 # enable defaults to false
    assert _refinement_config({'alignment_refinement': {'enable': True}}) == {'radius': None, 'rounds': 1, 'polish': True}
    assert _refinement_config({'alignment_refinement': {'enable': True, 'radius': 5.5, 'rounds': 2, 'polish': False}}) == \
        {'radius': 5.5, 'rounds': 2, 'polish': False}
    with pytest.raises(ValueError, match='unknown'):
        _refinement_config({'alignment_refinement': {'enable': True, 'radious': 5}})


def test_driver_key_set_unchanged_without_refinement():
    """An empty loader runs the driver's bookkeeping without a GPU: absent and disabled give today's keys, enabled adds the
    four *_refined keys and nothing else."""
    import multipoint_amd.utils as U
    base = {'nms': 4, 'detection_threshold': 0.015, 'topk': 300, 'reprojection_threshold': 3}
    absent = U.compute_descriptor_metrics(None, [], 'cpu', base, 4, 3)
    off = U.compute_descriptor_metrics(None, [], 'cpu', dict(base, alignment_refinement={'enable': False, 'rounds': 3}), 4, 3)
    on = U.compute_descriptor_metrics(None, [], 'cpu', dict(base, alignment_refinement={'enable': True}), 4, 3)
    assert set(absent) == set(off)
    assert not any(k.endswith('_refined') for k in absent)
    assert set(on) - set(absent) == {'h_correctness_refined', 'average_h_error_refined', 'pts_dist_refined',
                                     'n_matches_refined'}
    assert set(absent) <= set(on)


def test_argument_errors_come_before_any_launch():
    import multipoint_amd.utils as U
    P, K, D = 2, 4, 64
    desc = torch.zeros((P, K, D)); cnt = torch.zeros((P,), dtype=torch.int32)
    kp = torch.zeros((P, K, 2), dtype=torch.int32)
    Hm = torch.eye(3, dtype=torch.float64).repeat(P, 1, 1)
    for radius in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='radius'):
            U.guided_pairs(desc, cnt, desc, cnt, kp, kp, Hm, radius)
    with pytest.raises(ValueError, match='multiple of D'):
        big = torch.zeros((P + 1, K, D))                  # (long enough for P pairs at the odd stride)
        U.guided_pairs(big, cnt, big, cnt, kp, kp, Hm, 6.0, pair_stride=K * D + 1)
    with pytest.raises(ValueError, match=r'\[P, K, 2\]'):
        U.guided_pairs(desc, cnt, desc, cnt, kp[:, :2], kp, Hm, 6.0)
    with pytest.raises(ValueError, match='int32'):
        U.guided_pairs(desc, cnt, desc, cnt, kp.to(torch.int64), kp, Hm, 6.0)
    with pytest.raises(ValueError, match='one 3x3 homography per pair'):
        U.guided_pairs(desc, cnt, desc, cnt, kp, kp, Hm[:1], 6.0)
    res = PairResults(torch.zeros((2 * P, K, 2), dtype=torch.int32), None, torch.zeros((2 * P,), dtype=torch.int32), None,
                      torch.full((P, K), -1, dtype=torch.int32), torch.zeros((P, K)), cnt, 8, 8)
    with pytest.raises(ValueError, match='threshold'):
        U.refine_homography(res, Hm, reproj_threshold=0.0)
    with pytest.raises(ValueError, match='iters'):
        U.refine_homography(res, Hm, iters=-1)
    with pytest.raises(ValueError, match='one 3x3 matrix per pair'):
        U.refine_homography(res, Hm[:1])
    res.match_mode = 'nearest'
    with pytest.raises(ValueError, match='mutual'):
        U.refine_alignment(res)
    res.match_mode = 'mutual'
    with pytest.raises(ValueError, match='rounds'):
        U.refine_alignment(res, rounds=-1)
    with pytest.raises(ValueError, match='radius'):
        U.refine_alignment(res, radius=0.0)
