"""GPU (MI355X): guided re-matching (mp_match_guided) and the Levenberg-Marquardt polish (mp_refine_homography) from the
kernels up to utils.refine_alignment, utils.compute_descriptor_metrics and predict_align_image_pair.py --refine.

The matcher's yardstick is the float64 restatement of tests/guided_restatement.py on its planted pairs (tolerance and
ambiguity as in tests/test_gpu_match_modes.py); the polish's is oracle/cv_homography.py::_lm_refine, the restatement of
OpenCV 4.2's solver, on the same inlier set."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import guided_restatement as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = R.K
MP_EINVAL = -1


@pytest.fixture(scope='module')
def cases():
    """Planted pairs and their float64 yardstick per radius, computed once per D and left unchanged."""
    out = {}
    for D in R.WIDTHS:
        prs = [R.make_pair(D, c) for c in range(len(R.PAIRS))]
        ref = {r: [R.guided_mutual(p['A'], p['B'], p['kpA'], p['kpB'], p['H'], r, D) for p in prs] for r in R.RADII}
        out[D] = (prs, ref)
    return out


def _interleaved(prs, D, homs=None):
    """The pairs in the interleaved layout of a PairResults (slot 2p optical, 2p+1 thermal): (desc [2P,K,D], kp [2P,K,2],
    count [2P], H [P,3,3]) on the device, and the strides."""
    P = len(prs)
    desc = np.zeros((2 * P, K, D), np.float32); kp = np.zeros((2 * P, K, 2), np.int32); cnt = np.zeros(2 * P, np.int32)
    for p, pr in enumerate(prs):
        n, m = len(pr['A']), len(pr['B'])
        desc[2 * p, :n] = pr['A']; desc[2 * p + 1, :m] = pr['B']
        kp[2 * p, :n] = pr['kpA']; kp[2 * p + 1, :m] = pr['kpB']
        cnt[2 * p], cnt[2 * p + 1] = n, m
    H = np.stack([pr['H'] for pr in prs]) if homs is None else np.asarray(homs, np.float64)
    return (torch.from_numpy(desc).to(DEV), torch.from_numpy(kp).to(DEV), torch.from_numpy(cnt).to(DEV),
            torch.from_numpy(H).to(DEV), dict(pair_stride=2 * K * D, count_stride=2))


def _guided(desc, kp, cnt, H, lay, radius, threshold=-1.0):
    from multipoint_amd.utils import guided_pairs
    out = guided_pairs(desc, cnt, desc[1:], cnt[1:], kp, kp[1:], H, radius, threshold, **lay)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize('radius', R.RADII)
@pytest.mark.parametrize('D', R.WIDTHS)
def test_kernel_against_float64(cases, D, radius):
    prs, ref = cases[D]
    for pr in prs:                                      # conditions on the INPUTS, before the GPU is touched
        margin, amb = R.input_conditions(pr, D, radius)
        assert margin >= R.MIN_RADIUS_MARGIN and amb <= R.MAX_AMBIGUOUS
    # all seven pairs in one launch, plus pair 0 once more under an all-zero H ("no estimate")
    homs = [pr['H'] for pr in prs] + [np.zeros((3, 3))]
    desc, kp, cnt, H, lay = _interleaved(prs + [prs[0]], D, homs)
    midx, mdist, mcnt = _guided(desc, kp, cnt, H, lay, radius)
    t2 = 2 * R.tau(D)
    for p, (pr, (want, amb, u)) in enumerate(zip(prs, ref[radius])):
        N, M = len(pr['A']), len(pr['B'])
        got = midx[p]
        assert (got[N:] == -1).all() and (mdist[p][N:] == 0).all()
        assert mcnt[p] == int((got >= 0).sum())
        ok = ~amb
        print('D %d radius %g pair %d (%d x %d): %d matched, %d ambiguous' % (D, radius, p, N, M, int((got >= 0).sum()),
                                                                             int(amb.sum())))
        assert np.array_equal(got[:N][ok], want[ok])
        assert (mdist[p][got < 0] == 0).all()
        rows = np.nonzero(got[:N] >= 0)[0]
        if len(rows):
            err = np.abs(mdist[p][rows].astype(np.float64) ** 2 - u[rows, got[rows]]).max()
            print('    max |d^2 - u64| = %.3g (2 tau = %.3g)' % (err, t2))
            assert err <= t2
    assert mcnt[len(prs)] == 0 and (midx[len(prs)] == -1).all() and (mdist[len(prs)] == 0).all()


@pytest.mark.parametrize('D', R.WIDTHS)
def test_wide_gate_is_the_mutual_matcher(cases, D):
    """H = identity and a radius beyond the frame admit every (i, j): indices, distance bits and counts equal
    mp_match_mutual_nn's, with and without a distance threshold."""
    from multipoint_amd.utils import match_pairs
    prs, _ = cases[D]
    desc, kp, cnt, H, lay = _interleaved(prs, D, [np.eye(3)] * len(prs))
    for thr in (-1.0, 0.7):
        got = _guided(desc, kp, cnt, H, lay, 1e6, thr)
        want = [o.cpu().numpy() for o in match_pairs(desc, cnt, desc[1:], cnt[1:], thr, **lay)]
        print('D %d threshold %g: %s matches per pair' % (D, thr, want[2].tolist()))
        assert np.array_equal(got[0], want[0])
        assert np.array_equal(got[1].view(np.int32), want[1].view(np.int32))
        assert np.array_equal(got[2], want[2])
        assert want[2].sum() > 0


@pytest.mark.parametrize('D', R.WIDTHS)
def test_guided_finds_the_partners_the_mutual_matcher_loses(cases, D):
    from multipoint_amd.utils import match_pairs
    prs, _ = cases[D]
    sub = prs[:2]                                       # (160, 130) and (37, 160)
    desc, kp, cnt, H, lay = _interleaved(sub, D)
    gidx = _guided(desc, kp, cnt, H, lay, 6.0)[0]
    pidx = match_pairs(desc, cnt, desc[1:], cnt[1:], **lay)[0].cpu().numpy()
    for p, pr in enumerate(sub):
        t = pr['true']
        found = int((gidx[p][t[:, 0]] == t[:, 1]).sum()); plain = int((pidx[p][t[:, 0]] == t[:, 1]).sum())
        print('D %d pair %d: guided finds %d of %d planted partners, mutual NN %d' % (D, p, found, len(t), plain))
        assert found >= 0.9 * len(t)
        assert found >= 1.5 * plain
        j = gidx[p][gidx[p] >= 0]
        assert len(np.unique(j)) == len(j)              # one-to-one


def test_two_launches_give_identical_bytes(cases):
    prs, _ = cases[256]
    desc, kp, cnt, H, lay = _interleaved(prs, 256)
    first = _guided(desc, kp, cnt, H, lay, 48.0)
    again = _guided(desc, kp, cnt, H, lay, 48.0)
    for x, y in zip(first, again):
        assert x.tobytes() == y.tobytes()


def test_refusals():
    """MP_EINVAL from the C entry itself (the Python wrapper has checks of its own in front of it)."""
    from multipoint_amd import _lib
    h = _lib.get_handle(torch.device(DEV))

    def call(P, Kc, D, radius, pair_stride=None):
        desc = torch.zeros((P, Kc, D + 1), dtype=torch.float32, device=DEV)       # (room for the odd stride)
        cnt = torch.zeros((P,), dtype=torch.int32, device=DEV)
        kp = torch.zeros((P, Kc, 2), dtype=torch.int32, device=DEV)
        hom = torch.zeros((P, 9), dtype=torch.float64, device=DEV)
        mi = torch.empty((P, Kc), dtype=torch.int32, device=DEV); md = torch.empty((P, Kc), dtype=torch.float32, device=DEV)
        mc = torch.empty((P,), dtype=torch.int32, device=DEV)
        return h.lib.mp_match_guided(h.ptr, _lib.ptr(desc), _lib.ptr(cnt), _lib.ptr(desc), _lib.ptr(cnt),
                                     Kc * D if pair_stride is None else pair_stride, 1, P, Kc, D, _lib.ptr(kp), _lib.ptr(kp),
                                     _lib.ptr(hom), radius, -1.0, _lib.ptr(mi), _lib.ptr(md), _lib.ptr(mc),
                                     _lib.stream_ptr(torch.device(DEV)))
    assert call(2, 4, 64, 6.0) == 0
    assert call(2, 4, 96, 6.0) == MP_EINVAL
    assert call(65536, 1, 64, 6.0) == MP_EINVAL
    assert call(2, 4, 64, 0.0) == MP_EINVAL
    assert call(2, 4, 64, -3.0) == MP_EINVAL
    assert call(2, 4, 64, float('nan')) == MP_EINVAL
    assert call(2, 4, 64, float('inf')) == MP_EINVAL
    assert call(2, 4, 64, 6.0, pair_stride=4 * 64 + 1) == MP_EINVAL
    assert b'multiple of D' in h.lib.mp_last_error(h.ptr)
    torch.cuda.synchronize()                           # nothing was launched by the refused calls: no error is pending


# ----------------------------------------------------------------------------------------------------------------------
# the polish
# ----------------------------------------------------------------------------------------------------------------------
PH, PW, NPTS = 480, 640, 200


def _planted(rng):
    a = rng.uniform(-0.15, 0.15); s = rng.uniform(0.9, 1.1)
    C = np.array([[1, 0, -PW / 2], [0, 1, -PH / 2], [0, 0, 1.0]]); Ci = np.array([[1, 0, PW / 2], [0, 1, PH / 2], [0, 0, 1.0]])
    M = np.array([[s * np.cos(a), -s * np.sin(a), rng.uniform(-20, 20)], [s * np.sin(a), s * np.cos(a), rng.uniform(-20, 20)],
                  [rng.uniform(-2e-4, 2e-4), rng.uniform(-2e-4, 2e-4), 1.0]])
    H = Ci @ M @ C
    return H / H[2, 2]


def _correspondences(seed, outliers, P=8):
    """P pairs of NPTS correspondences under planted homographies on 480 x 640, rounded to integers, a fraction replaced by
    uniformly random points.  Returns (PairResults with the identity match list, src [P,N,2] (x, y), dst [P,N,2])."""
    from multipoint_amd.pipeline import PairResults
    rng = np.random.default_rng(seed)
    kp = np.zeros((2 * P, NPTS, 2), np.int32)
    for p in range(P):
        H = _planted(rng)
        src = np.stack([rng.integers(0, PW, NPTS), rng.integers(0, PH, NPTS)], 1).astype(np.float64)
        q = np.concatenate([src, np.ones((NPTS, 1))], 1) @ H.T
        dst = np.round(q[:, :2] / q[:, 2:3])
        bad = rng.permutation(NPTS)[:int(outliers * NPTS)]
        dst[bad] = np.stack([rng.integers(0, PW, len(bad)), rng.integers(0, PH, len(bad))], 1)
        kp[2 * p] = src[:, ::-1]; kp[2 * p + 1] = dst[:, ::-1]
    res = PairResults(torch.from_numpy(kp).to(DEV), None, torch.full((2 * P,), NPTS, dtype=torch.int32, device=DEV), None,
                      torch.arange(NPTS, dtype=torch.int32, device=DEV).repeat(P, 1).contiguous(), None, None, PH, PW)
    return res, kp[0::2, :, ::-1].astype(np.float64), kp[1::2, :, ::-1].astype(np.float64)


def _project(H, pts):
    q = np.concatenate([pts, np.ones((len(pts), 1))], 1) @ np.asarray(H).reshape(3, 3).T
    return q[:, :2] / q[:, 2:3]


@pytest.mark.parametrize('outliers', [0.1, 0.3, 0.5])
def test_polish_against_the_oracle(outliers):
    """mp_refine_homography from mp_find_homography's estimate against _lm_refine on the same inlier set.  The corner bound
    of 1e-3 px comes from use -- three orders below the +-0.5 px quantisation of the keypoints --, not from a measurement;
    the observed maxima are printed."""
    from oracle import cv_homography as CV
    from multipoint_amd.utils import find_homography, refine_homography
    res, src, dst = _correspondences(int(outliers * 100), outliers)
    H0, _, n0 = find_homography(res, 3.0)
    H1, mask, nin, cost = refine_homography(res, H0, 3.0)
    H0 = H0.cpu().numpy(); H1 = H1.cpu().numpy(); mask = mask.cpu().numpy().astype(bool); nin = nin.cpu().numpy()
    cost = cost.cpu().numpy()
    corners = np.array([[0, 0], [PW, 0], [0, PH], [PW, PH]], np.float64)
    worst_corner = worst_cost = 0.0
    for p in range(len(H0)):
        assert n0[p] >= 4
        # the returned mask is the inlier set of the INPUT estimate
        err = np.linalg.norm(_project(H0[p], src[p]) - dst[p], axis=1)
        clear = np.abs(err - 3.0) > 1e-9
        assert np.array_equal(mask[p][clear], (err <= 3.0)[clear])
        assert nin[p] == int(mask[p].sum()) and nin[p] >= 0.9 * (1 - outliers) * NPTS
        s_in, d_in = src[p][mask[p]], dst[p][mask[p]]
        assert abs(H1[p][2, 2] - 1.0) == 0.0
        before = float(CV._reproj_err2(H0[p] / H0[p][2, 2], s_in, d_in).sum())
        after = float(CV._reproj_err2(H1[p], s_in, d_in).sum())
        assert abs(cost[p, 0] - before) <= 1e-9 * before and abs(cost[p, 1] - after) <= 1e-9 * after
        assert cost[p, 1] <= cost[p, 0]                                    # exact: only improving steps are accepted
        Ho = CV._lm_refine(H0[p], s_in, d_in, 10)
        want = float(CV._reproj_err2(Ho, s_in, d_in).sum())
        dc = np.linalg.norm(_project(H1[p], corners) - _project(Ho, corners), axis=1).max()
        worst_corner = max(worst_corner, dc); worst_cost = max(worst_cost, cost[p, 1] / want - 1.0)
        print('outliers %.0f %% pair %d: %d inliers, cost %.6f -> %.6f (oracle %.6f), corners differ by %.3g px'
              % (100 * outliers, p, nin[p], cost[p, 0], cost[p, 1], want, dc))
        assert cost[p, 1] <= want * (1 + 1e-6)
        assert dc <= 1e-3
    print('outliers %.0f %%: max corner difference %.3g px, max cost excess over the oracle %.3g' % (100 * outliers, worst_corner,
                                                                                                  worst_cost))


def test_polish_without_enough_inliers_returns_zeros():
    from multipoint_amd.utils import find_homography, refine_homography
    res, _, _ = _correspondences(7, 0.1, P=3)
    H0, _, _ = find_homography(res, 3.0)
    res.match_idx[1, 3:] = -1                           # pair 1: three matches
    H0[2] = 0.0                                         # pair 2: no estimate
    before = H0.clone()
    H1, mask, nin, cost = refine_homography(res, H0, 3.0)
    assert torch.equal(H0, before)                      # the caller's tensor is not polished in place
    assert int(nin[0]) >= 4 and float(H1[0].abs().sum()) > 0
    assert float(H1[1].abs().sum()) == 0 and int(nin[1]) <= 3 and int(mask[1].sum()) == int(nin[1])
    assert float(H1[2].abs().sum()) == 0 and int(nin[2]) == 0 and int(mask[2].sum()) == 0
    assert float(cost[1:].abs().sum()) == 0


# ----------------------------------------------------------------------------------------------------------------------
# composition, driver, command line
# ----------------------------------------------------------------------------------------------------------------------
def _results(prs, D):
    from multipoint_amd.pipeline import PairResults
    from multipoint_amd.utils import match_pairs
    desc, kp, cnt, _, lay = _interleaved(prs, D)
    mi, md, mc = match_pairs(desc, cnt, desc[1:], cnt[1:], **lay)
    return PairResults(kp, None, cnt, desc, mi, md, mc, *R.FRAME)


def test_refine_alignment_is_the_composition_of_its_steps(cases):
    from multipoint_amd.pipeline import PairResults
    from multipoint_amd.utils import find_homography, guided_pairs, refine_alignment, refine_homography
    prs, _ = cases[64]
    res = _results(prs, 64)
    keep = [t.clone() for t in (res.match_idx, res.match_dist, res.match_count, res.kp_yx, res.kp_count, res.desc)]
    res2, H, mask, nin = refine_alignment(res, 3.0)
    # by hand
    H0, _, n0 = find_homography(res, 3.0)
    mi, md, mc = guided_pairs(res.desc, res.kp_count, res.desc[1:], res.kp_count[1:], res.kp_yx, res.kp_yx[1:], H0, 6.0,
                              pair_stride=2 * K * 64, count_stride=2)
    none = n0 < 4                                       # pairs without a first estimate keep their matches
    assert bool(none.any()) and not bool(none.all())    # (the empty and two-row pairs / the large ones)
    mi = torch.where(none[:, None], res.match_idx, mi); md = torch.where(none[:, None], res.match_dist, md)
    mc = torch.where(none, res.match_count, mc)
    hand = PairResults(res.kp_yx, None, res.kp_count, res.desc, mi, md, mc, *R.FRAME, 'guided')
    H1, _, _ = find_homography(hand, 3.0)
    H2, mask2, nin2, _ = refine_homography(hand, H1, 3.0)
    assert res2.match_mode == 'guided' and res2 is not res
    assert res2.kp_yx is res.kp_yx and res2.desc is res.desc and res2.kp_count is res.kp_count
    assert torch.equal(res2.match_idx, mi) and torch.equal(res2.match_dist, md) and torch.equal(res2.match_count, mc)
    assert torch.equal(H, H2) and torch.equal(mask, mask2) and torch.equal(nin, nin2)
    assert float(H[none].abs().sum()) == 0
    print('matches per pair: first %s, guided %s; inliers %s' % (res.match_count.tolist(), mc.tolist(), nin.tolist()))
    assert int(mc[0]) > int(res.match_count[0]) or int(nin[0]) > int(n0[0])
    for was, now in zip(keep, (res.match_idx, res.match_dist, res.match_count, res.kp_yx, res.kp_count, res.desc)):
        assert torch.equal(was, now)
    assert res.match_mode == 'mutual'
    # nothing to do: the first estimate and the original matches
    res3, H3, mask3, nin3 = refine_alignment(res, 3.0, rounds=0, polish=False)
    H0b, mask0, n0b = find_homography(res, 3.0)
    assert torch.equal(H3, H0b) and torch.equal(mask3, mask0) and torch.equal(nin3, n0b)
    assert torch.equal(res3.match_idx, res.match_idx) and torch.equal(res3.match_count, res.match_count)
    assert res3.match_mode == 'guided'


@pytest.fixture(scope='module')
def net(oracle):
    import multipoint_amd.models as models
    cfg = dict(oracle.SHIPPED_MODEL_CONFIG)
    n = models.MultiPoint(cfg); n.load_state_dict(oracle.make_weights(0, cfg)); n.to(DEV); n.eval()
    return n


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(np.asarray(a), np.asarray(b))


def test_driver_reports_refined_keys_only_when_enabled(net):
    import multipoint_amd.utils as U
    import test_gpu_match_modes as MM                   # (its synthetic loader and prediction block)
    pred = MM._pred(MM.DEFAULT)
    plain = U.compute_descriptor_metrics(net, MM._loader(2), DEV, pred, 4, 3)
    off = U.compute_descriptor_metrics(net, MM._loader(2), DEV, dict(pred, alignment_refinement={'enable': False}), 4, 3)
    on = U.compute_descriptor_metrics(net, MM._loader(2), DEV, dict(pred, alignment_refinement={'enable': True}), 4, 3)
    new = {'h_correctness_refined', 'average_h_error_refined', 'pts_dist_refined', 'n_matches_refined'}
    assert set(off) == set(plain) and set(on) == set(plain) | new and not (set(plain) & new)
    for k in plain:
        assert _same(plain[k], off[k]) and _same(plain[k], on[k]), k
    assert len(on['pts_dist_refined']) == 4 and len(on['n_matches_refined']) == 4
    print('pts_dist %s refined %s, matches after re-matching %s' % (np.array2string(np.asarray(on['pts_dist']), precision=3),
                                                                    np.array2string(on['pts_dist_refined'], precision=3),
                                                                    on['n_matches_refined'].tolist()))
    assert on['average_h_error_refined'] == on['pts_dist_refined'].mean()
    assert on['h_correctness_refined'] == (on['pts_dist_refined'] < 3).sum() / 4


def test_cli_refine(tmp_path):
    d = tmp_path / 'multipoint'
    d.mkdir()
    with open(os.path.join(ROOT, 'model_weights', 'multipoint', 'params.yaml')) as f:
        (d / 'params.yaml').write_text(f.read())
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'config_image_pair_dataset_prediction.yaml')))
    cfg['dataset'].update({'num_samples': 2, 'height': 120, 'width': 160})
    cfg['dataset']['augmentation']['homographic']['enable'] = False
    cfg['prediction'].update({'topk': 300, 'batchsize': 1, 'num_worker': 0})
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    base = [sys.executable, os.path.join(ROOT, 'predict_align_image_pair.py'), '-y', str(tmp_path / 'cfg.yaml'), '-m', str(d),
            '-v', 'none']
    # two fresh child processes, side by side
    runs = [subprocess.Popen(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
            for extra in (['-p'], ['--refine'])]
    (plain, perr), (refined, rerr) = [r.communicate() for r in runs]
    assert runs[0].returncode == 0, perr[-2000:]
    assert runs[1].returncode == 0, rerr[-2000:]
    line = [l for l in refined.split('\n') if l.startswith('Refinement:')]
    print(line)
    assert len(line) == 1
    assert re.match(r'Refinement: \d+ inliers of \d+ matches -> (\d+ inliers of \d+ matches|no refined estimate|unchanged)',
                    line[0])
    # without the flag nothing of the refinement is printed, and what -p prints is what --refine prints in front of its own lines
    assert 'Refine' not in plain

    def stable(text):
        return [l for l in text.split('\n') if not re.search(r'took:|Box nms:', l)]
    head = stable(refined)[:stable(refined).index(line[0])]
    assert stable(plain)[:len(head)] == head
    assert 'RANSAC inliers:' in head[-1]
