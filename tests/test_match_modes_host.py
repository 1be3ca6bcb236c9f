"""CPU: which `prediction.matching` configurations PairPipeline accepts (reference
configs/config_image_pair_dataset_prediction.yaml, multipoint/utils/matching.py:4-33).  The pipeline batches every mode
that keeps one match per optical keypoint and raises what utils.get_matches raises for the configurations that function
rejects; no GPU is touched (construction only)."""
import pytest

from multipoint_amd.pipeline import PairPipeline, PairResults


def _pipe(method, kwargs, knn):
    return PairPipeline(None, {'matching': {'method': method, 'method_kwargs': kwargs, 'knn_matches': knn}})


def test_one_way_nearest_is_accepted():
    p = _pipe('bfmatcher', {}, False)
    assert p.match_mode == 'nearest' and p.match_ratio == 0.0
    assert _pipe('bfmatcher', {'crossCheck': False}, False).match_mode == 'nearest'


def test_ratio_test_is_accepted():
    p = _pipe('bfmatcher', {}, True)
    assert p.match_mode == 'ratio'
    assert p.match_ratio == 0.9                   # the double 0.9 get_matches multiplies by (matching.py:22), not 0.9f


def test_mutual_configurations_unchanged():
    p = _pipe('bfmatcher', {'crossCheck': True}, False)
    assert p.match_mode == 'mutual' and p.match_threshold == -1.0
    p = _pipe('nnmatcher', {'threshold': 0.8}, False)
    assert p.match_mode == 'mutual' and p.match_threshold == 0.8
    assert _pipe('nnmatcher', {}, False).match_threshold == 0.7
    assert PairPipeline(None, {}).match_mode == 'mutual'                # no matching block: the shipped default


def test_rejected_configurations_raise_what_get_matches_raises():
    with pytest.raises(ValueError):               # OpenCV: crossCheck supports k = 1 only
        _pipe('bfmatcher', {'crossCheck': True}, True)
    with pytest.raises(AttributeError):           # NNMatcher has no knnMatch (matching.py:21)
        _pipe('nnmatcher', {}, True)
    with pytest.raises(ValueError, match='non-negative'):
        _pipe('nnmatcher', {'threshold': -0.1}, False)
    with pytest.raises(ValueError, match='unknown matching method'):
        _pipe('nope', {}, False)


@pytest.mark.parametrize('method', ['thresholdmatcher', 'flann'])
@pytest.mark.parametrize('knn', [False, True])
def test_one_to_many_and_flann_stay_refused(method, knn):
    with pytest.raises(NotImplementedError):
        _pipe(method, {}, knn)


def test_pair_results_carry_the_match_mode():
    assert PairResults(None, None, None, None, None, None, None, 0, 0).match_mode == 'mutual'
    assert PairResults(None, None, None, None, None, None, None, 0, 0, 'ratio').match_mode == 'ratio'


def test_pair_metrics_refuses_one_way_matches():
    """tp[2p+1] of mp_pair_metrics reads a match from the thermal side: only a one-to-one list defines it."""
    import multipoint_amd.utils as U
    for mode in ('nearest', 'ratio'):
        with pytest.raises(ValueError, match='mutual'):
            U.pair_metrics(PairResults(None, None, None, None, None, None, None, 0, 0, mode), None, 4.0)
