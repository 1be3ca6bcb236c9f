"""Host side of the pooled homography estimate (no GPU): argument refusals before any launch, group ids, and the logic of
estimate_initial_transform.py -- the written matrix, the refusal to overwrite, --max-pairs, the report -- with a faked estimator."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

import pooled_cases as C
from multipoint_amd.utils import PooledMatches, pool_matches  # noqa: F401  (the feature under test: nothing here runs without it)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LGHD_DIR = os.path.join(ROOT, 'tests', 'golden', 'lghd')


def _host_results(P=3, K=16):
    from multipoint_amd.pipeline import PairResults
    return PairResults(torch.zeros((2 * P, K, 2), dtype=torch.int32), None, torch.zeros(2 * P, dtype=torch.int32), None,
                       -torch.ones((P, K), dtype=torch.int32), None, None, 64, 64)


def _host_pooled(n=10, G=1):
    import multipoint_amd.utils as U
    return U.PooledMatches(torch.zeros((n, 4)), None, None, torch.zeros(G + 1, dtype=torch.int32))


def test_exports():
    import multipoint_amd.utils as U
    for name in ('pool_matches', 'find_homography_pooled', 'refine_homography_pooled', 'estimate_shared_homography',
                 'find_homography_pooled_points', 'PooledMatches', 'pooled_chunk'):
        assert hasattr(U, name)
    chunk, splits = U.pooled_chunk()
    assert chunk >= 256 and chunk % 256 == 0 and splits >= 1
    assert U.MAX_RANSAC_MATCHES == 3200                                   # the per-pair limit is what it was


@pytest.mark.parametrize('groups', [[0, 1, 0], [2, 1, 1], [0, 0, -1], [0, 1], [0.0, 1.0, 2.0], [[0, 1, 2]], [0, 1, 70000]])
def test_pool_matches_refuses_bad_group_ids(groups):
    """Ids that decrease, negative ids, the wrong number or type of ids, more groups than a launch takes: ValueError before
    anything touches a device (the results here live on the host, so a launch would fail differently)."""
    import multipoint_amd.utils as U
    with pytest.raises(ValueError, match='group'):
        U.pool_matches(_host_results(), np.array(groups))


def test_group_ids_accepted():
    from multipoint_amd.utils.evaluation import _group_ids
    assert _group_ids(None, 5) == (None, 1)
    g, G = _group_ids([0, 0, 3, 3, 4], 5)
    assert g.dtype == np.int32 and g.tolist() == [0, 0, 3, 3, 4] and G == 5          # (ids 1 and 2: empty groups)
    g, G = _group_ids(torch.tensor([1, 1, 1]), 3)
    assert g.tolist() == [1, 1, 1] and G == 2


def test_estimators_refuse_bad_arguments():
    import multipoint_amd.utils as U
    pm = _host_pooled()
    for call in (lambda: U.find_homography_pooled(pm, 0.0),
                 lambda: U.find_homography_pooled(pm, float('nan')),
                 lambda: U.find_homography_pooled(pm, 3.0, max_iters=0),
                 lambda: U.find_homography_pooled(pm, 3.0, max_iters=(1 << 20) + 1),
                 lambda: U.find_homography_pooled(pm._replace(pts=torch.zeros((10, 3)))),
                 lambda: U.find_homography_pooled(pm._replace(pts=torch.zeros((10, 4), dtype=torch.float64))),
                 lambda: U.find_homography_pooled(pm._replace(group_offsets=torch.zeros(2, dtype=torch.int64))),
                 lambda: U.find_homography_pooled(pm._replace(group_offsets=torch.zeros(1, dtype=torch.int32))),
                 lambda: U.find_homography_pooled(pm._replace(group_offsets=torch.zeros(65537, dtype=torch.int32))),
                 lambda: U.refine_homography_pooled(pm, np.eye(3), reproj_threshold=-1.0),
                 lambda: U.refine_homography_pooled(pm, np.eye(3), iters=-1),
                 lambda: U.refine_homography_pooled(pm, np.eye(3), iters=1001),
                 lambda: U.refine_homography_pooled(pm, np.zeros((2, 3, 3))),
                 lambda: U.refine_homography_pooled(_host_pooled(G=2), np.eye(3)),
                 lambda: U.estimate_shared_homography(_host_results(), reproj_threshold=0.0),
                 lambda: U.estimate_shared_homography(_host_results(), max_iters=0),
                 lambda: U.estimate_shared_homography(_host_results(), iters=2000),
                 lambda: U.estimate_shared_homography(_host_results(), groups=[1, 0, 0]),
                 lambda: U.find_homography_pooled_points(np.zeros((5, 2)), np.zeros((4, 2))),
                 lambda: U.find_homography_pooled_points(np.zeros((5, 2)), np.zeros((5, 2)), reproj_threshold=0.0),
                 lambda: U.find_homography_pooled_points(np.zeros((5, 2)), np.zeros((5, 2)), max_iters=0)):
        with pytest.raises(ValueError):
            call()


def test_too_many_correspondences_refused():
    """N >= 2^24 (a zero-stride view: no memory behind it)."""
    import multipoint_amd.utils as U
    big = torch.zeros((1, 4)).expand(1 << 24, 4)
    with pytest.raises(ValueError, match='at most'):
        U.find_homography_pooled(_host_pooled()._replace(pts=big))


def test_fewer_than_four_points_need_no_device():
    import multipoint_amd.utils as U
    Hm, mask = U.find_homography_pooled_points(np.zeros((3, 2)), np.zeros((3, 2)))
    assert Hm is None and mask.shape == (3,) and mask.dtype == np.uint8 and not mask.any()


def test_pool_host_restatement():
    """The numpy restatement the GPU test compares against, on a case small enough to write down."""
    kp = np.zeros((4, 3, 2), np.int32)
    kp[0] = [[1, 2], [3, 4], [5, 6]]; kp[1] = [[7, 8], [9, 10], [0, 0]]
    kp[2] = [[11, 12], [13, 14], [0, 0]]; kp[3] = [[15, 16], [0, 0], [0, 0]]
    cnt = np.array([3, 2, 2, 1], np.int32)
    midx = np.array([[1, -1, 2], [0, 0, 0]], np.int32)                     # pair 0: row 2 names partner 2 >= nt = 2: dropped
    pts, qidx, po, go = C.pool_host(kp, cnt, midx, [0, 2])
    assert pts.tolist() == [[2, 1, 10, 9], [12, 11, 16, 15], [14, 13, 16, 15]] and qidx.tolist() == [0, 0, 1]
    assert po.tolist() == [0, 1, 3] and go.tolist() == [0, 1, 1, 3]
    assert C.scatter_mask(np.array([1, 0, 1], np.uint8), qidx, po, 2, 3).tolist() == [[1, 0, 0], [0, 1, 0]]


# ----------------------------------------------------------------------------------------------------------------------
# estimate_initial_transform.py
# ----------------------------------------------------------------------------------------------------------------------
def _cli():
    import estimate_initial_transform as E
    return E


def _write_pairs(directory, n):
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    for i in range(n):
        Image.fromarray(np.full((8, 10), i, np.uint8)).save(os.path.join(directory, '%d_optical.png' % i))
        Image.fromarray(np.full((8, 8), i, np.uint16)).save(os.path.join(directory, '%d_thermal.png' % i))


def _fake_estimator(H, inliers_per_pair, matches_per_pair=6, seen=None):
    def estimator(args, config, names):
        if seen is not None:
            seen.append(list(names))
        mask = np.concatenate([np.arange(matches_per_pair) < inliers_per_pair[i % len(inliers_per_pair)] for i in range(len(names))])
        po = np.arange(len(names) + 1) * matches_per_pair
        return np.asarray(H, np.float64), mask.astype(np.uint8), po, int(mask.sum()), (12.5, 3.25)
    return estimator


def _args(directory, *extra):
    return ['-y', os.path.join(ROOT, 'configs', 'config_image_pair_dataset_prediction.yaml'), '-m', LGHD_DIR, '-v', 'none',
            '-i', str(directory)] + list(extra)


def test_written_matrix_is_the_normalised_inverse(tmp_path):
    E = _cli()
    rng = np.random.default_rng(1)
    for _ in range(5):
        H = C.random_homography(rng, shift=30.0) * rng.uniform(0.5, 2.0)          # (any scale: a homography has none)
        T = E.perspective_from_estimate(H)
        ref = np.linalg.inv(H.astype(np.float64))
        assert T.dtype == np.float64 and T[2, 2] == 1.0
        assert np.abs(T - ref / ref[2, 2]).max() <= 1e-12 * np.abs(ref / ref[2, 2]).max()
        x = np.array([37.0, 11.0, 1.0])                                          # thermal pixel -> optical pixel -> back
        y = H @ (T @ x)
        assert np.abs(y[:2] / y[2] - x[:2]).max() < 1e-9
    with pytest.raises(ValueError):
        E.perspective_from_estimate(np.zeros((3, 3)))
    _write_pairs(tmp_path, 3)
    H = np.array([[1.0, 0, -9], [0, 1, -5], [0, 0, 1]])
    assert E.main(_args(tmp_path), estimator=_fake_estimator(H, [5])) == 0
    got = np.array(yaml.safe_load(open(tmp_path / 'initial_transform.yaml'))['perspective'], np.float64)
    assert got.shape == (3, 3) and np.array_equal(got, [[1, 0, 9], [0, 1, 5], [0, 0, 1]])


def test_existing_file_needs_force(tmp_path):
    E = _cli()
    _write_pairs(tmp_path, 2)
    hand = 'perspective:\n- [1.0, 0.0, 2.0]\n- [0.0, 1.0, 3.0]\n- [0.0, 0.0, 1.0]\n# measured by hand\n'
    (tmp_path / 'initial_transform.yaml').write_text(hand)
    seen = []
    est = _fake_estimator(np.eye(3), [6], seen=seen)
    assert E.main(_args(tmp_path), estimator=est) != 0
    assert (tmp_path / 'initial_transform.yaml').read_text() == hand and not seen      # refused before any estimate
    assert not (tmp_path / 'initial_transform_report.json').exists()
    assert E.main(_args(tmp_path, '--force'), estimator=est) == 0
    assert yaml.safe_load(open(tmp_path / 'initial_transform.yaml'))['perspective'] == np.eye(3).tolist()
    other = tmp_path / 'elsewhere' / 'guess.yaml'                                      # -o: the report goes next to it
    os.makedirs(other.parent)
    assert E.main(_args(tmp_path, '-o', str(other)), estimator=est) == 0
    assert other.exists() and (other.parent / 'initial_transform_report.json').exists()


def test_max_pairs_selection(tmp_path):
    E = _cli()
    names = [str(i) for i in range(10)]
    assert E.select_pairs(names, 0) == names and E.select_pairs(names, 10) == names and E.select_pairs(names, 99) == names
    assert E.select_pairs(names, 1) == ['0'] and E.select_pairs(names, 2) == ['0', '9']
    assert E.select_pairs(names, 4) == ['0', '3', '6', '9'] and E.select_pairs(names, 5) == ['0', '2', '4', '6', '9']
    for n in range(1, 40):
        for k in range(1, n + 1):
            got = E.select_pairs(list(range(n)), k)
            assert len(got) == len(set(got)) == k and got == sorted(got) and got[0] == 0 and (k == 1 or got[-1] == n - 1)
            assert max(np.diff(got), default=0) - min(np.diff(got), default=0) <= 1         # evenly spaced
    _write_pairs(tmp_path, 11)                                                             # numeric order: 0, 1, ..., 10
    seen = []
    assert E.main(_args(tmp_path, '--max-pairs', '3'), estimator=_fake_estimator(np.eye(3), [6], seen=seen)) == 0
    assert seen == [['0', '5', '10']]
    report = json.load(open(tmp_path / 'initial_transform_report.json'))
    assert report['pairs_read'] == 11 and report['pairs_used'] == 3


def test_report_fields(tmp_path):
    E = _cli()
    _write_pairs(tmp_path, 4)
    assert E.main(_args(tmp_path), estimator=_fake_estimator(np.eye(3), [5, 0, 4, 3])) == 0
    report = json.load(open(tmp_path / 'initial_transform_report.json'))
    assert report == {'pairs_read': 4, 'pairs_used': 4, 'matches_pooled': 24, 'inliers': 12, 'cost_before_polish': 12.5,
                      'cost_after_polish': 3.25, 'inliers_per_pair': {'0': 5, '1': 0, '2': 4, '3': 3}, 'pairs_with_4_inliers': 2}
    with pytest.raises(ValueError):
        E.build_report(['0'], ['0'], [0, 5], np.zeros(4), 0, None)


def test_too_few_inliers_write_nothing(tmp_path):
    E = _cli()
    _write_pairs(tmp_path, 3)
    assert E.main(_args(tmp_path), estimator=_fake_estimator(np.zeros((3, 3)), [1])) == 1          # 3 inliers in all
    assert not (tmp_path / 'initial_transform.yaml').exists() and not (tmp_path / 'initial_transform_report.json').exists()
    empty = tmp_path / 'empty'
    os.makedirs(empty)
    assert E.main(_args(empty), estimator=_fake_estimator(np.eye(3), [6])) == 1
