"""GPU (MI355X): sub-pixel keypoints -- the refinement kernel (mp_refine_keypoints) against its float64 restatement and on
planted Gaussian blobs, descriptor sampling at fractional positions (mp_sample_descriptors_f) against the oracle and the
reference's fixture, the homography estimators on float keypoints (mp_find_homography_f, mp_refine_homography_f,
mp_pool_matches_f) against their int namesakes, a planted pair end to end, and the option in PairPipeline and on the command
line.  Every bound is derived where it is used; measured figures are printed before they are asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import subpixel_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
# the matrix of the issue's DLT experiment, optical (x, y, 1) -> thermal, on a 120 x 160 frame
PLANTED_H = np.array([[1.02, 0.03, 3.3], [-0.025, 0.98, -2.7], [1e-4, -5e-5, 1.0]])
FH, FW = 120, 160


def _project(H, pts_xy):
    q = np.concatenate([pts_xy, np.ones((len(pts_xy), 1))], 1) @ np.asarray(H, np.float64).reshape(3, 3).T
    return q[:, :2] / q[:, 2:3]


def _corner_error(H_est, H_true=PLANTED_H):
    corners = np.array([[0, 0], [FW, 0], [0, FH], [FW, FH]], np.float64)
    return float(np.linalg.norm(_project(H_est, corners) - _project(H_true, corners), axis=1).mean())


# ----------------------------------------------------------------------------------------------------------------------
# the refinement kernel against the restatement
# ----------------------------------------------------------------------------------------------------------------------
def _refinement_case(H, W, seed):
    """B = 3 maps and lists: image 0 a random positive map with EVERY pixel a keypoint (row 0, column W - 1, centres lower
    than a neighbour, refined and unrefined axes), image 1 without keypoints, image 2 a map of crafted neighbourhoods.
    Returns (prob [3,H,W] float32, kp [3,n,2] int32, counts)."""
    rng = np.random.default_rng(seed)
    prob = np.zeros((3, H, W), np.float32)
    prob[0] = rng.uniform(0.02, 1.0, (H, W))
    prob[1] = rng.uniform(0.02, 1.0, (H, W))
    m = np.full((H, W), 0.125, np.float32)
    pts = []
    # (y, x), then the values at (y-1,x), (y+1,x), (y,x-1), (y,x+1) and the centre
    crafted = [((1, 1), (0.0, 0.25, 0.25, 0.375, 0.5)),        # a zero neighbour on y
               ((1, 4), (0.25, 0.25, 0.375, 0.25, 0.5)),       # two equal neighbours on y
               ((1, 7), (0.5, 0.5, 0.25, 0.375, 0.5)),         # three equal values on y
               ((4, 1), (0.75, 0.25, 0.25, 0.375, 0.5)),       # a centre lower than a neighbour on y
               ((4, 4), (0.25, 0.375, 0.5, 0.5, 0.5)),         # three equal values on x
               ((4, 7), (0.25, 0.375, 0.25, 0.5, 0.5)),        # a neighbour equal to the centre on x: half a pixel
               ((6, 2), (0.25, 0.375, -0.5, 0.25, 0.5)),       # a negative neighbour on x
               ((6, 5), (np.inf, 0.25, 0.25, 0.375, 0.5)),     # an infinite neighbour on y
               ((6, 9), (0.25, np.nan, 0.25, 0.375, 0.5))]     # a NaN neighbour on y
    for (y, x), (up, down, left, right, c) in crafted:
        m[y - 1, x], m[y + 1, x], m[y, x - 1], m[y, x + 1], m[y, x] = up, down, left, right, c
        pts.append((y, x))
    pts += [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 5), (3, W - 1)]          # the frame's edge
    prob[2] = m
    n = H * W
    kp = np.zeros((3, n, 2), np.int32)
    kp[0] = np.stack(np.unravel_index(np.arange(n), (H, W)), 1)
    kp[2, :len(pts)] = pts
    kp[2, len(pts):] = (2, 2)                                   # (slots beyond the count hold an in-frame pixel)
    return prob, kp, [n, 0, len(pts)]


def _pick_refinement_case(H, W):
    """The first seed whose random map keeps the restatement's own left-out cases (bound > 0.05 px) within 2 %: chosen on the
    CPU from the float64 rule alone, before the kernel runs."""
    for seed in range(50):
        prob, kp, counts = _refinement_case(H, W, seed)
        sub, refined, bound = R.refine_keypoints(prob.astype(np.float64), kp, counts)
        live = np.zeros(bound.shape, bool)
        for b, c in enumerate(counts):
            live[b, :c] = True
        left_out = live & refined & (bound > 0.05)
        # (within 2 % of the whole lists and of their first 40 rows, the two list lengths the test runs)
        if left_out.sum() <= 0.02 * live.sum() and left_out[:, :40].sum() <= 0.02 * live[:, :40].sum():
            return prob, kp, counts, sub, refined, bound, left_out, live
    raise AssertionError('no seed keeps the ill-conditioned cases within 2 %')


@pytest.mark.parametrize('shape', [(9, 13), (8, 12)])
@pytest.mark.parametrize('where', ['K above the counts', 'K below the counts'])
def test_refinement_against_float64(shape, where):
    """Per axis |kernel - restatement| <= 8 * 2^-23 * (|l-| + 2 |l0| + |l+|) / |den| + 1e-6: <= 2 ulp for each logf plus the
    first-order sensitivity of the quotient to them (tests/subpixel_restatement.py computes it); the 1e-6 holds the rounding
    of the quotient and of y + delta at y < 16.  Axes the rule does not refine equal the integer exactly."""
    import multipoint_amd.utils as U
    H, W = shape
    prob, kp, counts, sub, refined, bound, left_out, live = _pick_refinement_case(H, W)
    n = kp.shape[1]
    K = n + 3 if where == 'K above the counts' else 40               # 40 < H * W (image 0), > 15 (image 2)
    kp_k = np.full((3, K, 2), 2, np.int32)
    kp_k[:, :min(K, n)] = kp[:, :K]
    got = U.refine_keypoints(torch.from_numpy(prob[:, None]).to(DEV), torch.from_numpy(kp_k).to(DEV),
                             torch.tensor(counts, dtype=torch.int32, device=DEV))
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, K, 2)
    got = got.cpu().numpy().astype(np.float64)
    worst = 0.0
    checked = unrefined = 0
    for b in range(3):
        c = min(counts[b], K)
        assert (got[b, c:] == 0).all()                                  # rows beyond the count
        for k in range(c):
            for a in range(2):
                if left_out[b, k, a]:
                    continue
                if not refined[b, k, a]:
                    assert got[b, k, a] == float(kp[b, k, a]), (b, k, a)
                    unrefined += 1
                    continue
                dev = abs(got[b, k, a] - sub[b, k, a])
                worst = max(worst, dev / bound[b, k, a])
                assert dev <= bound[b, k, a], (b, k, a, dev, bound[b, k, a])
                assert abs(got[b, k, a] - kp[b, k, a]) <= 0.5 + 1e-6
                checked += 1
    print('%dx%d %s: %d refined axes checked, %d unrefined exact, %d left out of %d; largest deviation / bound = %.3f'
          % (H, W, where, checked, unrefined, int(left_out.sum()), int(live.sum()), worst))
    assert checked >= 15 and unrefined >= 15


@pytest.mark.parametrize('sigma', [0.8, 1.2, 2.0])
def test_refinement_recovers_planted_blobs(sigma):
    """den = -1 / sigma^2 <= -0.25 and |l| <= 10 put the bound above below 4e-5 px; y + delta rounds by <= 8e-6 at y < 256."""
    import multipoint_amd.utils as U
    rng = np.random.default_rng(int(sigma * 10) + 1)
    centres, base = R.planted_centres(rng, FH, FW, 40)
    prob = R.render_blobs(FH, FW, centres, sigma, dtype=np.float32)
    got = U.refine_keypoints(torch.from_numpy(prob).to(DEV), torch.from_numpy(base.astype(np.int32))[None].to(DEV),
                             torch.tensor([40], dtype=torch.int32, device=DEV))[0].cpu().numpy().astype(np.float64)
    err = np.abs(got - centres).max()
    print('sigma %.1f: largest error %.3e px' % (sigma, err))
    assert err <= 1e-4


# ----------------------------------------------------------------------------------------------------------------------
# descriptor sampling at fractional positions
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [64, 128, 256, 384])
def test_fractional_sampling_against_the_oracle(oracle, D):
    import multipoint_amd.utils as U
    H, W, Hc, Wc = 24, 40, 3, 5
    rng = np.random.default_rng(D)
    desc = rng.standard_normal((D, Hc, Wc)).astype(np.float32)
    kp = np.concatenate([np.stack([rng.uniform(0, H - 1, 40), rng.uniform(0, W - 1, 40)], 1),
                         [[0, 0], [H, W], [H - 1, W - 1], [H / 2.0, W / 4.0], [-0.4, 3.3], [5.5, -0.3], [H + 0.4, 7.7],
                          [9.1, W + 0.45]]]).astype(np.float32)
    want = oracle.interpolate_descriptors(kp, desc, H, W)
    kp_t = torch.from_numpy(kp).to(DEV)
    before = kp_t.clone()
    got = U.interpolate_descriptors(kp_t, torch.from_numpy(desc).to(DEV), H, W)
    assert torch.equal(kp_t, before)                                    # the caller's keypoints are not normalised in place
    err = np.abs(got.cpu().numpy() - want).max()
    print('D %d: largest difference to the oracle %.3e' % (D, err))
    assert err <= 1e-5
    # fractions are used, not truncated
    trunc = U.interpolate_descriptors(torch.from_numpy(kp.astype(np.int64)).to(DEV), torch.from_numpy(desc).to(DEV), H, W)
    assert np.abs(trunc.cpu().numpy()[:40] - want[:40]).max() > 1e-3
    # a float tensor of whole numbers is the int entry bit for bit (batched, with rows beyond the counts)
    kpi = torch.from_numpy(np.stack([rng.integers(0, H, (2, 9)), rng.integers(0, W, (2, 9))], 2).astype(np.int32)).to(DEV)
    cnt = torch.tensor([9, 4], dtype=torch.int32, device=DEV)
    dmap = torch.from_numpy(rng.standard_normal((2, D, Hc, Wc)).astype(np.float32)).to(DEV)
    a = U.interpolate_descriptors_batched(kpi, cnt, dmap, H, W)
    b = U.interpolate_descriptors_batched(kpi.float(), cnt, dmap, H, W)
    c = U.interpolate_descriptors_batched(kpi.double(), cnt, dmap, H, W)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
    assert float(b[1, 4:].abs().sum()) == 0


def test_fractional_sampling_against_the_reference_fixture(golden_dir):
    import multipoint_amd.utils as U
    g = np.load(os.path.join(golden_dir, 'sampling_fractional.npz'))
    got = U.interpolate_descriptors(torch.from_numpy(g['kp']).to(DEV), torch.from_numpy(g['desc']).to(DEV), int(g['H']), int(g['W']))
    err = np.abs(got.cpu().numpy() - g['out']).max()
    print('largest difference to the reference rows %.3e' % err)
    assert err <= 1e-5


# ----------------------------------------------------------------------------------------------------------------------
# homography from float keypoints
# ----------------------------------------------------------------------------------------------------------------------
def _planted_lists(seed=3, P=3, K=40):
    """P pairs of K integer correspondences under PLANTED_H (a fifth replaced by random points); the last pair keeps three
    matches.  Returns (kp [2P,K,2] int32, counts [2P], match_idx [P,K])."""
    rng = np.random.default_rng(seed)
    kp = np.zeros((2 * P, K, 2), np.int32)
    midx = np.tile(np.arange(K, dtype=np.int32), (P, 1))
    for p in range(P):
        src = np.stack([rng.integers(0, FW, K), rng.integers(0, FH, K)], 1).astype(np.float64)
        dst = np.round(_project(PLANTED_H, src))
        bad = rng.permutation(K)[:K // 5]
        dst[bad] = np.stack([rng.integers(0, FW, len(bad)), rng.integers(0, FH, len(bad))], 1)
        perm = rng.permutation(K)                                        # the partner of optical i is thermal perm[i]
        kp[2 * p] = src[:, ::-1]
        kp[2 * p + 1, perm] = dst[:, ::-1]
        midx[p] = perm
    midx[P - 1, 3:] = -1
    midx[0, 5] = -1; midx[0, 17] = K + 2                                 # no partner; a partner beyond the thermal list
    cnt = np.full(2 * P, K, np.int32)
    cnt[1] = K - 2                                                       # (a thermal list shorter than K drops two partners)
    return kp, cnt, midx


def _pair_results(kp, cnt, midx, sub=None):
    from multipoint_amd.pipeline import PairResults
    return PairResults(torch.from_numpy(kp).to(DEV), None, torch.from_numpy(cnt).to(DEV), None, torch.from_numpy(midx).to(DEV),
                       None, None, FH, FW, kp_sub=None if sub is None else torch.from_numpy(sub).to(DEV))


def _bytes_equal(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
               for x, y in zip(a, b))


def test_float_homography_of_whole_numbers_is_the_int_entry():
    """One kernel template behind both entries: an integer-valued float list gives H, mask, n_inliers and cost byte for
    byte -- per pair (find, polish), pooled (the list, find, polish) -- and the same bytes from run to run."""
    import multipoint_amd.utils as U
    kp, cnt, midx = _planted_lists()
    ri = _pair_results(kp, cnt, midx)
    rf = _pair_results(kp, cnt, midx, kp.astype(np.float32))
    fi, ff, ff2 = U.find_homography(ri, 3.0, 500, seed=4), U.find_homography(rf, 3.0, 500, seed=4), U.find_homography(rf, 3.0, 500, seed=4)
    assert _bytes_equal(fi, ff) and _bytes_equal(ff, ff2)
    H, mask, nin = fi
    assert int(nin[0]) >= 20 and int(nin[1]) >= 20
    assert float(H[2].abs().sum()) == 0 and int(nin[2]) == 0 and int(mask[2].sum()) == 0        # three matches: no model
    assert _corner_error(H[0].cpu().numpy()) < 3.0
    pi, pf, pf2 = U.refine_homography(ri, H, 3.0), U.refine_homography(rf, H, 3.0), U.refine_homography(rf, H, 3.0)
    assert _bytes_equal(pi, pf) and _bytes_equal(pf, pf2)
    assert float(pf[0][2].abs().sum()) == 0 and float(pf[3][2].abs().sum()) == 0
    groups = np.array([0, 0, 1])
    li, lf = U.pool_matches(ri, groups), U.pool_matches(rf, groups)
    assert _bytes_equal(li, lf) and li.pts.shape[0] == int(li.pair_offsets[-1]) > 60
    si = U.estimate_shared_homography(ri, groups, 3.0, 500, seed=4)
    sf = U.estimate_shared_homography(rf, groups, 3.0, 500, seed=4)
    sf2 = U.estimate_shared_homography(rf, groups, 3.0, 500, seed=4)
    for a, b in ((si, sf), (sf, sf2)):
        assert _bytes_equal((a.H, a.mask, a.n_inliers, a.cost), (b.H, b.mask, b.n_inliers, b.cost))
    assert float(sf.H[1].abs().sum()) == 0 and int(sf.n_inliers[0]) >= 40                        # group 1: three matches
    # refine_alignment's estimates: without re-matching rounds it is find + polish on the list it was given
    ai, af = U.refine_alignment(ri, 3.0, rounds=0, max_iters=500, seed=4), U.refine_alignment(rf, 3.0, rounds=0, max_iters=500, seed=4)
    assert _bytes_equal(ai[1:], af[1:]) and _bytes_equal(af[1:], pf[:3]) and af[0].kp_sub is rf.kp_sub and ai[0].kp_sub is None


def test_float_homography_reads_the_fractions():
    """Exact projective correspondences: the float entries recover the planted matrix, the int entries see them truncated."""
    import multipoint_amd.utils as U
    rng = np.random.default_rng(11)
    K = 40
    src = np.stack([rng.uniform(5, FW - 5, K), rng.uniform(5, FH - 5, K)], 1)
    dst = _project(PLANTED_H, src)
    sub = np.stack([src[:, ::-1], dst[:, ::-1]]).astype(np.float32)
    kp = sub.astype(np.int32)
    cnt = np.full(2, K, np.int32)
    midx = np.arange(K, dtype=np.int32)[None]
    for name, res in (('int', _pair_results(kp, cnt, midx)), ('float', _pair_results(kp, cnt, midx, sub))):
        H0, _, n0 = U.find_homography(res, 3.0, 500)
        H1, _, n1, cost = U.refine_homography(res, H0, 3.0)
        shared = U.estimate_shared_homography(res, None, 3.0, 500)
        e1, e2 = _corner_error(H1[0].cpu().numpy()), _corner_error(shared.H[0].cpu().numpy())
        print('%s keypoints: corner error per pair %.3e px, pooled %.3e px, polished cost %.3e' % (name, e1, e2, float(cost[0, 1])))
        assert name == 'int' or (int(n0[0]) == K and int(n1[0]) == K)
        # float32 positions are exact to 2^-17 px at x < 256: three orders below the bound; truncation costs tenths of a pixel
        assert (e1 <= 1e-3 and e2 <= 1e-3) if name == 'float' else (e1 > 0.05 and e2 > 0.05)
    # find_homography_points: floating input is not truncated, integer input goes as before
    Hf, mf = U.find_homography_points(src, dst, 3.0, 500, device=DEV)
    Hi, mi = U.find_homography_points(kp[0][:, ::-1], kp[1][:, ::-1], 3.0, 500, device=DEV)
    Hk, _, _ = U.find_homography(_pair_results(kp, cnt, midx), 3.0, 500)
    assert _corner_error(Hf) <= 1e-3 and mf.sum() == K
    assert np.array_equal(Hi, Hk[0].cpu().numpy()) and _corner_error(Hi) > 0.05


def test_float_entries_refuse_what_the_int_entries_refuse():
    from multipoint_amd import _lib
    h = _lib.get_handle(torch.device(DEV))
    z = torch.zeros(64, dtype=torch.float32, device=DEV)
    i = torch.zeros(64, dtype=torch.int32, device=DEV)
    d = torch.zeros(64, dtype=torch.float64, device=DEV)
    s = _lib.stream_ptr(torch.device(DEV))
    assert h.lib.mp_find_homography_f(h.ptr, None, _lib.ptr(i), _lib.ptr(i), 1, 4, 3.0, 10, 0, _lib.ptr(d), _lib.ptr(i), _lib.ptr(i), s) != 0
    assert b'mp_find_homography_f' in h.lib.mp_last_error(h.ptr)
    assert h.lib.mp_find_homography_f(h.ptr, _lib.ptr(z), _lib.ptr(i), _lib.ptr(i), 1, 3201, 3.0, 10, 0, _lib.ptr(d), _lib.ptr(i), _lib.ptr(i), s) != 0
    assert h.lib.mp_refine_homography_f(h.ptr, _lib.ptr(z), _lib.ptr(i), _lib.ptr(i), 1, 4, -1.0, 10, _lib.ptr(d), _lib.ptr(i), _lib.ptr(i), None, s) != 0
    assert b'mp_refine_homography_f' in h.lib.mp_last_error(h.ptr)
    assert h.lib.mp_sample_descriptors_f(h.ptr, _lib.ptr(z), 1, 1, 1, 32, 8, 8, _lib.ptr(z), _lib.ptr(i), 1, _lib.ptr(z), s) != 0
    assert b'mp_sample_descriptors_f' in h.lib.mp_last_error(h.ptr)
    assert h.lib.mp_refine_keypoints(h.ptr, _lib.ptr(z), 1, 0, 8, _lib.ptr(i), _lib.ptr(i), 1, _lib.ptr(z), s) != 0
    assert h.lib.mp_refine_keypoints(h.ptr, None, 1, 8, 8, _lib.ptr(i), _lib.ptr(i), 1, _lib.ptr(z), s) != 0
    assert b'mp_refine_keypoints' in h.lib.mp_last_error(h.ptr)


# ----------------------------------------------------------------------------------------------------------------------
# a planted pair, end to end
# ----------------------------------------------------------------------------------------------------------------------
def test_planted_pair_end_to_end():
    """40 blobs of sigma 1.2 on 120 x 160, the thermal map rendered at the warped centres, matches by construction:
    box-NMS keypoints -> refine_keypoints -> find_homography + refine_homography.  With the sub-pixel lists the mean corner
    error is <= 0.01 px (localisation <= 1e-4 px, a conditioning factor below 10 for ~40 correspondences in this frame, a
    tenfold margin on top) and below a tenth of what the same calls give on the integer lists (0.29-0.54 px by the float64
    DLT on rounded points)."""
    import multipoint_amd.utils as U
    rng = np.random.default_rng(5)
    centres, base = R.planted_centres(rng, FH, FW, 165)
    warped = _project(PLANTED_H, centres[:, ::-1])[:, ::-1]
    inside = (warped[:, 0] >= 6) & (warped[:, 0] <= FH - 7) & (warped[:, 1] >= 6) & (warped[:, 1] <= FW - 7)
    keep = np.sort(rng.choice(np.nonzero(inside)[0], 40, replace=False))
    centres, warped = centres[keep], warped[keep]
    prob = np.stack([R.render_blobs(FH, FW, centres, 1.2, dtype=np.float32), R.render_blobs(FH, FW, warped, 1.2, dtype=np.float32)])
    prob_t = torch.from_numpy(prob[:, None]).to(DEV)
    K = 48
    kp, _, cnt = U.detect_keypoints(prob_t, 4, 0.1, capacity=K)
    assert cnt.tolist() == [40, 40]
    sub = U.refine_keypoints(prob_t, kp, cnt)
    kp_h, sub_h = kp.cpu().numpy(), sub.cpu().numpy().astype(np.float64)
    # matches by construction: the keypoint of blob i in either list
    blob = [np.abs(kp_h[s, :40, None, :] - c[None]).max(-1).argmin(1) for s, c in ((0, centres), (1, warped))]
    assert sorted(blob[0].tolist()) == list(range(40)) and sorted(blob[1].tolist()) == list(range(40))
    loc = max(np.abs(sub_h[0, :40] - centres[blob[0]]).max(), np.abs(sub_h[1, :40] - warped[blob[1]]).max())
    assert np.abs(sub_h[:, :40] - kp_h[:, :40]).max() <= 0.5
    where = np.empty(40, np.int64)
    where[blob[1]] = np.arange(40)                                       # thermal row of blob i
    midx = np.full((1, K), -1, np.int32)
    midx[0, :40] = where[blob[0]]
    errs = {}
    for name, s in (('integer', None), ('sub-pixel', sub.cpu().numpy())):
        res = _pair_results(kp_h, cnt.cpu().numpy(), midx, s)
        H0, _, n0 = U.find_homography(res, 3.0)
        H1, _, n1, _ = U.refine_homography(res, H0, 3.0)
        assert int(n0[0]) == 40 and int(n1[0]) == 40
        errs[name] = _corner_error(H1[0].cpu().numpy())
    print('localisation %.3e px; mean corner error: integer lists %.4f px, sub-pixel lists %.3e px' % (loc, errs['integer'], errs['sub-pixel']))
    assert loc <= 1e-4
    assert errs['sub-pixel'] <= 0.01
    assert errs['sub-pixel'] < 0.1 * errs['integer']


# ----------------------------------------------------------------------------------------------------------------------
# the pipeline, the driver, the command line
# ----------------------------------------------------------------------------------------------------------------------
PRED = {'nms': 4, 'detection_threshold': 0.015, 'topk': 120, 'cpu_nms': True, 'reprojection_threshold': 3,
        'matching': {'method': 'bfmatcher', 'method_kwargs': {'crossCheck': True}, 'knn_matches': False}}


@pytest.fixture(scope='module')
def net(oracle):
    import multipoint_amd.models as models
    cfg = dict(oracle.SHIPPED_MODEL_CONFIG)
    n = models.MultiPoint(cfg); n.load_state_dict(oracle.make_weights(0, cfg)); n.to(DEV); n.eval()
    return n


@pytest.fixture(scope='module')
def pair_images(oracle):
    opt = oracle.make_images(5, 2, 64, 96).to(DEV)
    th = torch.roll(opt, shifts=(2, 3), dims=(2, 3)).contiguous()
    return opt, th


def _check_subpixel_results(res, prob, desc_map, H, W):
    import multipoint_amd.utils as U
    res.wait()
    assert res.kp_sub is not None and res.kp_sub.dtype == torch.float32 and res.kp_sub.shape == res.kp_yx.shape
    assert torch.equal(res.kp_sub, U.refine_keypoints(prob, res.kp_yx, res.kp_count))
    assert torch.equal(res.desc, U.interpolate_descriptors_batched(res.kp_sub, res.kp_count, desc_map, H, W))
    K = res.kp_yx.shape[1]
    live = torch.arange(K, device=DEV)[None, :] < res.kp_count.clamp(max=K)[:, None]
    assert int(live.sum()) > 50
    d = (res.kp_sub - res.kp_yx.float()).abs()[live]
    assert float(d.max()) <= 0.5 and float(d.max()) > 0.01                 # refined, and never beyond half a pixel
    assert float(res.kp_sub[~live].abs().sum()) == 0
    host = res.to_host()
    assert len(host[0]['kp_optical_sub']) == len(host[0]['kp_optical']) and host[1]['kp_thermal_sub'].dtype == np.float32


def test_pipeline_with_subpixel(net, pair_images):
    from multipoint_amd.pipeline import PairPipeline
    opt, th = pair_images
    images = PairPipeline.interleave(opt, th)
    on = dict(PRED, subpixel={'enable': True})
    out = net({'image': images})
    pipe = PairPipeline(net, on)
    res = pipe.run_interleaved(images)
    pipe.check_converged(DEV)
    _check_subpixel_results(res, out['prob'], out['desc'], 64, 96)
    conv = PairPipeline(net, on, keep_maps=True).run_converged(images)
    _check_subpixel_results(conv, conv.prob, conv.desc_map, 64, 96)
    live = torch.arange(120, device=DEV)[None, :] < res.kp_count[:, None]         # (kp_yx rows beyond the count are not written)
    assert torch.equal(conv.kp_sub, res.kp_sub) and torch.equal(conv.kp_count, res.kp_count)
    assert torch.equal(conv.kp_yx[live], res.kp_yx[live])
    # two frame sizes: each camera's list is refined on its own map
    th2 = th[:, :, :, :80].contiguous()
    two = PairPipeline(net, on).run_two_sized(opt, th2)
    assert two.kp_sub.shape == two.kp_yx.shape and two.kp_sub.dtype == torch.float32
    import multipoint_amd.utils as U
    for side, img, w in ((0, opt, 96), (1, th2, 80)):
        o = net({'image': img, 'is_optical': torch.full((2, 1), side == 0, dtype=torch.bool)})
        assert torch.equal(two.kp_sub[side::2], U.refine_keypoints(o['prob'], two.kp_yx[side::2].contiguous(), two.kp_count[side::2].contiguous()))
        assert torch.equal(two.desc[side::2], U.interpolate_descriptors_batched(two.kp_sub[side::2].contiguous(), two.kp_count[side::2].contiguous(),
                                                                                o['desc'], 64, w))


def test_pipeline_without_the_key_is_unchanged(net, pair_images):
    """Key absent or disabled: kp_sub is None and every other field is what the stages give on the integer lists."""
    import multipoint_amd.utils as U
    from multipoint_amd.pipeline import PairPipeline
    opt, th = pair_images
    images = PairPipeline.interleave(opt, th)
    out = net({'image': images})
    runs = []
    for cfg in (PRED, dict(PRED, subpixel={'enable': False}), dict(PRED, subpixel=None)):
        pipe = PairPipeline(net, cfg)
        res = pipe.run_interleaved(images).wait()
        pipe.check_converged(DEV)
        assert res.kp_sub is None and 'kp_optical_sub' not in res.to_host()[0]
        runs.append(res)
    def lists(kp_yx, kp_score, kp_count):                 # (rows beyond a list's count are not written: compared as zeros)
        live = torch.arange(kp_yx.shape[1], device=DEV)[None, :] < kp_count[:, None]
        return (torch.where(live[..., None], kp_yx, torch.zeros_like(kp_yx)), torch.where(live, kp_score, torch.zeros_like(kp_score)),
                kp_count)
    fields = ('desc', 'match_idx', 'match_dist', 'match_count')
    for other in runs[1:]:
        assert _bytes_equal([getattr(runs[0], f) for f in fields], [getattr(other, f) for f in fields])
        assert _bytes_equal(lists(runs[0].kp_yx, runs[0].kp_score, runs[0].kp_count), lists(other.kp_yx, other.kp_score, other.kp_count))
    res = runs[0]
    kp, sc, cnt = U.detect_keypoints(out['prob'], 4, 0.015, keep_top_k=120, capacity=120, max_rounds=8)
    assert _bytes_equal(lists(res.kp_yx, res.kp_score, res.kp_count), lists(kp, sc, cnt))
    desc = U.interpolate_descriptors_batched(kp, cnt, out['desc'], 64, 96)
    assert _bytes_equal((res.desc,), (desc,))
    mi, md, mc = U.match_pairs(desc, cnt, desc[1:], cnt[1:], -1.0, pair_stride=2 * 120 * desc.shape[2], count_stride=2)
    assert _bytes_equal((res.match_idx, res.match_dist, res.match_count), (mi, md, mc))
    # the estimators read the integer lists of such results, as before
    Ha, _, _ = U.find_homography(res, 3.0, 300)
    from multipoint_amd.pipeline import PairResults
    bare = PairResults(res.kp_yx, None, res.kp_count, None, res.match_idx, None, None, 64, 96)
    Hb, _, _ = U.find_homography(bare, 3.0, 300)
    assert torch.equal(Ha, Hb)


def test_estimators_read_kp_sub_of_pipeline_results(net, pair_images):
    import multipoint_amd.utils as U
    from multipoint_amd.pipeline import PairPipeline, PairResults
    opt, th = pair_images
    res = PairPipeline(net, dict(PRED, subpixel={'enable': True})).run_converged(PairPipeline.interleave(opt, th))
    as_int = PairResults(res.kp_yx, res.kp_score, res.kp_count, res.desc, res.match_idx, res.match_dist, res.match_count, 64, 96)
    as_float = PairResults(res.kp_yx, res.kp_score, res.kp_count, res.desc, res.match_idx, res.match_dist, res.match_count, 64, 96,
                           kp_sub=res.kp_yx.float())
    Hs, _, ns = U.find_homography(res, 3.0, 300)
    Hi, _, ni = U.find_homography(as_int, 3.0, 300)
    Hf, _, nf = U.find_homography(as_float, 3.0, 300)
    assert torch.equal(Hi, Hf) and int(ns.min()) >= 4
    assert not torch.equal(Hs, Hi)                                       # the sub-pixel list is what the estimate read
    pooled = U.pool_matches(res)
    q = pooled.query_index.long()[: int(pooled.pair_offsets[1])]
    assert torch.equal(pooled.pts[: len(q), 0], res.kp_sub[0, q, 1]) and torch.equal(pooled.pts[: len(q), 1], res.kp_sub[0, q, 0])
    with pytest.raises(ValueError, match='kp_sub'):
        U.find_homography(PairResults(res.kp_yx, None, res.kp_count, None, res.match_idx, None, None, 64, 96,
                                      kp_sub=res.kp_sub.double()), 3.0, 300)


def test_driver_honours_the_subpixel_key(net):
    import multipoint_amd.utils as U
    import test_gpu_match_modes as MM                   # (its synthetic loader and prediction block)
    pred = MM._pred(MM.DEFAULT)
    off = U.compute_descriptor_metrics(net, MM._loader(2), DEV, dict(pred, subpixel={'enable': False}), 4, 3)
    on = U.compute_descriptor_metrics(net, MM._loader(2), DEV, dict(pred, subpixel={'enable': True}), 4, 3)
    assert set(on) == set(off) and len(on['pts_dist']) == len(off['pts_dist']) == 4
    print('pts_dist: integer %s, sub-pixel %s' % (np.array2string(np.asarray(off['pts_dist']), precision=3),
                                                 np.array2string(np.asarray(on['pts_dist']), precision=3)))
    assert not np.array_equal(on['pts_dist'], off['pts_dist'])            # the estimates read the refined lists


def test_cli_subpixel(tmp_path):
    d = tmp_path / 'multipoint'
    d.mkdir()
    with open(os.path.join(ROOT, 'model_weights', 'multipoint', 'params.yaml')) as f:
        (d / 'params.yaml').write_text(f.read())
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'config_image_pair_dataset_prediction.yaml')))
    cfg['dataset'].update({'num_samples': 2, 'height': 120, 'width': 160})
    cfg['dataset']['augmentation']['homographic']['enable'] = False
    cfg['prediction'].update({'topk': 300, 'batchsize': 1, 'num_worker': 0})
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    npz = tmp_path / 'out.npz'
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'predict_align_image_pair.py'), '-y', str(tmp_path / 'cfg.yaml'), '-m', str(d),
                          '-v', 'none', '--subpixel', '--save-npz', str(npz)], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert 'Estimated Homography:' in out.stdout
    g = np.load(npz)
    for side in ('optical', 'thermal'):
        kp, sub = g['kp_' + side], g['kp_%s_sub' % side]
        assert sub.dtype == np.float32 and sub.shape == kp.shape and len(kp) > 10
        d = np.abs(sub - kp)
        assert d.max() <= 0.5 and d.max() > 0.01
