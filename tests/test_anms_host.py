"""CPU: the adaptive non-maximal suppression restatement (tests/anms_restatement.py) against a second, independent formulation,
its stated properties, the planted-map finding of DESIGN.md, and the host plumbing of the spread entries."""
import os
import re

import numpy as np
import pytest

import anms_restatement as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('mp_box_nms_spread', 'mp_detect_keypoints_spread', 'mp_suppression_radii')


def sweep(y, x, s, k, robust):
    """The other way round: visit the candidates by descending score and keep the running set of those that dominate the current
    one (it only grows: the threshold s_i falls); plain Python arithmetic on numpy fp32 scalars.  Returns (kept, R)."""
    n = len(s)
    c = np.float32(robust)
    by_score = sorted(range(n), key=lambda i: (-float(s[i]), i))
    by_product = sorted(range(n), key=lambda j: (-float(c * s[j]), j))
    R = [A.NONE] * n
    running, nxt = [], 0
    for i in by_score:
        while nxt < n and s[i] < c * s[by_product[nxt]]:
            running.append(by_product[nxt])
            nxt += 1
        for j in running:
            R[i] = min(R[i], (int(y[i]) - int(y[j])) ** 2 + (int(x[i]) - int(x[j])) ** 2)
    ranked = sorted(range(n), key=lambda i: (-R[i], -float(s[i]), i))
    return sorted(ranked[:min(k, n)]), R


def random_list(rng, n, H, W, levels=0):
    idx = np.sort(rng.choice(H * W, n, replace=False))
    s = rng.random(n, dtype=np.float32) * np.float32(0.9) + np.float32(0.05)
    if levels:
        s = (np.floor(s * levels) + 1).astype(np.float32) / np.float32(levels)
    return idx // W, idx % W, s


@pytest.mark.parametrize('robust', [1.0, 0.9, 0.5])
@pytest.mark.parametrize('levels', [0, 8])
def test_restatement_equals_the_sweep(robust, levels):
    rng = np.random.default_rng(11)
    for n in (0, 1, 2, 17, 150):
        y, x, s = random_list(rng, n, 24, 32, levels)
        for k in (1, 5, n, n + 3):
            kept, R = A.select(y, x, s, k, robust)
            kept2, R2 = sweep(y, x, s, k, robust)
            assert R.tolist() == R2 and kept.tolist() == kept2, (n, k)


@pytest.mark.parametrize('robust', [1.0, 0.9, 0.5])
def test_no_dominator_iff_at_least_the_scaled_maximum(robust):
    rng = np.random.default_rng(5)
    for levels in (0, 8):
        y, x, s = random_list(rng, 200, 24, 32, levels)
        R = A.radii(y, x, s, robust)
        bound = np.float32(robust) * s.max()
        assert np.array_equal(R == A.NONE, s >= bound) and (R == A.NONE).any()
        assert (R[R != A.NONE] > 0).all()                          # distinct pixels


def test_exact_product_does_not_dominate():
    # powers of two with c = 0.5: s_i == c * s_j exactly for neighbouring levels, which must not dominate
    y, x = np.arange(4), np.zeros(4, np.int64)
    s = np.array([0.125, 0.25, 0.5, 1.0], np.float32)
    assert A.radii(y, x, s, 0.5).tolist() == [4, 4, A.NONE, A.NONE]
    assert A.radii(y, x, s, 1.0).tolist() == [1, 1, 1, A.NONE]
    assert A.radii(y, x, np.full(4, 0.5, np.float32), 1.0).tolist() == [A.NONE] * 4          # equal scores never dominate


def test_short_lists_are_kept_whole():
    rng = np.random.default_rng(2)
    y, x, s = random_list(rng, 40, 24, 32)
    for k in (40, 41, 1000):
        assert A.select(y, x, s, k)[0].tolist() == list(range(40))
    assert len(A.select(y, x, s, 39)[0]) == 39


def test_ties_fall_back_on_score_then_index():
    # a lattice of equal scores: every R is NONE, every score equal -- the first k in row-major order stay
    y, x = np.divmod(np.arange(12), 4)
    assert A.select(y * 4, x * 4, np.full(12, 0.3, np.float32), 5)[0].tolist() == [0, 1, 2, 3, 4]
    # equal R, different scores: the higher score first
    s = np.array([1.0, 0.2, 0.3, 0.2], np.float32)
    kept, R = A.select([1, 1, 1, 2], [4, 3, 5, 4], s, 2)
    assert R.tolist() == [A.NONE, 1, 1, 1] and kept.tolist() == [0, 2]


@pytest.mark.parametrize('seed', range(5))
def test_planted_map_score_topk_clusters_and_anms_spreads(seed):
    m = A.planted_map(seed)
    yx = np.argwhere(m > 0)
    s = m[yx[:, 0], yx[:, 1]]
    assert 271 <= len(yx) <= 286
    by_score = np.lexsort((np.arange(len(s)), -s.view(np.uint32).astype(np.int64)))[:64]
    assert A.occupied_cells(yx[by_score]) == 4
    kept, _ = A.select(yx[:, 0], yx[:, 1], s, 64, 1.0)
    assert len(kept) == 64 and A.occupied_cells(yx[kept]) >= 15


def test_plumbing():
    from multipoint_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'multipoint_hip.h')).read()
    integration = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in ENTRIES:
        m = re.search(r'\bint %s\(([^;]*)\);' % name, header)
        assert m, '%s is not declared in the header' % name
        params = [p for p in m.group(1).replace('\n', ' ').split(',') if p.strip()]
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(params), name
        assert params[0].strip() == 'mp_handle* h' and params[-1].strip() == 'void* stream'
        assert '`%s`' % name in integration, '%s is missing from INTEGRATION.md' % name
    # the spread entries are the score entries' arguments plus robust (and the radii)
    for name, extra in (('mp_box_nms', 1), ('mp_detect_keypoints', 2)):
        assert len(_lib.SIGNATURES[name + '_spread'][1]) == len(_lib.SIGNATURES[name][1]) + extra
    assert 'keypoints_spread.hip' in build.SOURCES and build.SCRATCH_CAPS['keypoints_spread.hip'] == 0


def test_mode_arguments_are_checked_on_the_host():
    import multipoint_amd.utils as U
    from multipoint_amd.pipeline import PairPipeline
    assert U.topk_selection({'topk': 0}) == {} and U.topk_selection({'topk': 5, 'topk_mode': 'score', 'anms_robust': 0.5}) == {}
    assert U.topk_selection({'topk': 5, 'topk_mode': 'anms'}) == {'topk_mode': 'anms', 'anms_robust': 1.0}
    with pytest.raises(ValueError, match='topk_mode'):
        U.topk_selection({'topk': 5, 'topk_mode': 'grid'})
    with pytest.raises(ValueError, match='top-k above 0'):
        U.topk_selection({'topk': 0, 'topk_mode': 'anms'})
    assert PairPipeline(None, {'topk': 32, 'topk_mode': 'anms', 'anms_robust': 0.9}).anms_robust == 0.9
    assert PairPipeline(None, {'topk': 32}).topk_mode == 'score'
    with pytest.raises(ValueError):
        PairPipeline(None, {'topk': 32, 'topk_mode': 'ssc'})
    with pytest.raises(ValueError):
        PairPipeline(None, {'topk': 0, 'topk_mode': 'anms'})
    import torch
    with pytest.raises(ValueError, match='topk_mode'):              # (refused before the device is asked for)
        U.detect_keypoints(torch.rand(16, 16), 4, 0.015, keep_top_k=4, topk_mode='best')
    # the command lines share one pair of flags
    import estimate_initial_transform
    import export_keypoints
    import predict_align_image_pair
    import predict_keypoints
    for mod, base in ((predict_align_image_pair, []), (predict_keypoints, []), (export_keypoints, ['-o', 'x.npz']),
                      (estimate_initial_transform, ['-i', 'x'])):
        args = mod.build_parser().parse_args(base + ['--topk-mode', 'anms', '--anms-robust', '0.9'])
        assert args.topk_mode == 'anms' and args.anms_robust == 0.9
        args = mod.build_parser().parse_args(base)
        assert args.topk_mode is None and args.anms_robust is None
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(base + ['--topk-mode', 'grid'])
