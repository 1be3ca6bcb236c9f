"""Host-side mirror of the descriptor-metric driver of the reference (multipoint/utils/evaluation.py:209-439,
`compute_descriptor_metrics`, the `-e` mode of predict_align_image_pair.py:69-73): forward, NMS/top-k, descriptor
sampling and mutual-NN matching run through PairPipeline, and the per-sample arithmetic (keypoint warping by the
ground-truth homography, the N x M correctness test, true positives of the matches, matching score) runs on the GPU
behind mp_pair_metrics.  Only the final precision/recall bookkeeping over the concatenated match lists is numpy, as
in the reference (:360-419).

The RANSAC homography estimate (:330-349, cv2.findHomography) runs on the GPU as well (mp_find_homography: same
algorithm family, not OpenCV's RNG, so estimates agree with OpenCV's only to the reprojection tolerance); the
4-corner error derived from it (:351-356) is four points of numpy per pair."""
import collections
import ctypes

import numpy as np
import torch

from .. import _lib


def div0(a, b):
    # evaluation.py:202-207
    with np.errstate(divide='ignore', invalid='ignore'):
        c = np.true_divide(a, b)
        idx = ~np.isfinite(c)
        c[idx] = np.where(a[idx] == 0, 1, 0)
    return c


def compute_mAP(precision, recall):
    # evaluation.py:99-103
    return np.sum(precision[1:] * (recall[1:] - recall[:-1]))


def ground_truth_homographies(h_optical, h_thermal):
    """evaluation.py:259,288: gt = h_t @ inv(h_o) and its inverse, fp32 like the reference's torch ops.
    h_* : (P,3,3) tensors/arrays.  Returns a (2P,9) float64 tensor: slot 2p = gt, 2p+1 = inv(gt)."""
    ho = torch.as_tensor(h_optical, dtype=torch.float32).cpu()
    ht = torch.as_tensor(h_thermal, dtype=torch.float32).cpu()
    gt = torch.matmul(ht, torch.linalg.inv(ho))
    gti = torch.linalg.inv(gt)
    return torch.stack([gt, gti], dim=1).reshape(-1, 9).to(torch.float64)


def pair_metrics(res, homography, threshold_keypoints):
    """GPU arithmetic of evaluation.py:287-328 for the pairs of a PairResults.
    homography: (2P,9) float64 from ground_truth_homographies().
    Returns (metrics [P,8] int32 device tensor, tp [2P,K] uint8 device tensor); see include/multipoint_hip.h.
    The results must hold MUTUAL matches (match_mode 'mutual', or 'guided': mutual inside a gate): tp[2p+1] reads the same pair from the thermal side, which only a one-to-one
    match list defines (the reference hard-codes the cross-check matcher for these metrics, evaluation.py:273-282)."""
    if getattr(res, 'match_mode', 'mutual') not in ('mutual', 'guided'):
        raise ValueError("pair_metrics needs mutual matches (match_mode 'mutual' or 'guided': one-to-one lists); these "
                         "results were matched in '%s' mode" % res.match_mode)
    res.wait()
    dev = res.kp_yx.device
    P = res.num_pairs
    K = res.kp_yx.shape[1]
    hom = torch.as_tensor(homography, dtype=torch.float64).reshape(2 * P, 9).to(dev).contiguous()
    metrics = torch.empty((P, 8), dtype=torch.int32, device=dev)
    tp = torch.empty((2 * P, K), dtype=torch.uint8, device=dev)
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_pair_metrics(h.ptr, _lib.ptr(res.kp_yx.contiguous()), _lib.ptr(res.kp_count.contiguous()),
                                      _lib.ptr(res.match_idx.contiguous()), _lib.ptr(hom), P, K, int(res.H), int(res.W),
                                      float(threshold_keypoints), _lib.ptr(metrics), _lib.ptr(tp),
                                      _lib.stream_ptr(dev)))
    return metrics, tp


def _keypoints_for_estimate(res, h, entry):
    """The keypoint list a homography estimator reads and the C entry that takes it: the sub-pixel positions res.kp_sub
    through `entry`_f when the results carry them (prediction.subpixel), else the integer list through `entry`."""
    sub = getattr(res, 'kp_sub', None)
    if sub is not None:
        if sub.dtype != torch.float32 or tuple(sub.shape) != tuple(res.kp_yx.shape):
            raise ValueError('%s: kp_sub must be float32 of the shape of kp_yx %s; got %s %s'
                             % (entry, tuple(res.kp_yx.shape), sub.dtype, tuple(sub.shape)))
        return getattr(h.lib, entry + '_f'), sub.contiguous()
    return getattr(h.lib, entry), res.kp_yx.contiguous()


# ----------------------------------------------------------------------------------------------------------------------
# the motion models of the estimators (MP_MODEL_*)
# ----------------------------------------------------------------------------------------------------------------------
TRANSFORM_MODELS = {'homography': 0, 'similarity': 1, 'affine': 2}       # MP_MODEL_*
TRANSFORM_MIN_POINTS = {'homography': 4, 'similarity': 2, 'affine': 3}   # the minimal sample S of a model


def transform_model(model):
    """The MP_MODEL_* number of a model name ('homography', 'similarity', 'affine')."""
    if model not in TRANSFORM_MODELS:
        raise ValueError('unknown transform model %r: expected one of %s' % (model, sorted(TRANSFORM_MODELS)))
    return TRANSFORM_MODELS[model]


def transform_min_inliers(model):
    """The fewest inliers a model of this kind is reported with: 4 for a homography, S + 1 for the others (a model that explains
    only its own minimal sample is no model)."""
    transform_model(model)
    return 4 if model == 'homography' else TRANSFORM_MIN_POINTS[model] + 1


# Every estimator below is one private body that two public functions call: the *_homography* one with model None -- it goes
# through the mp_*_homography* entries, which take no model -- and the *_transform* one with the model's name, through the
# mp_*_transform* entries.  `fn` is the public function's name, for the messages of the bodies that have any.
def _entry(step, model, suffix=''):
    """The name of the C entry of `step` ('find', 'refine') and the model arguments it takes."""
    if model is None:
        return 'mp_%s_homography%s' % (step, suffix), ()
    return 'mp_%s_transform%s' % (step, suffix), (transform_model(model),)


def _pair_find(res, model, reproj_threshold, max_iters, seed):
    name, margs = _entry('find', model)
    res.wait()
    dev = res.kp_yx.device
    P, K = res.num_pairs, res.kp_yx.shape[1]
    Hm = torch.empty((P, 3, 3), dtype=torch.float64, device=dev)
    mask = torch.empty((P, K), dtype=torch.uint8, device=dev)
    nin = torch.empty((P,), dtype=torch.int32, device=dev)
    h = _lib.get_handle(dev)
    entry, kp = _keypoints_for_estimate(res, h, name)
    with torch.cuda.device(dev):
        h.check(entry(h.ptr, _lib.ptr(kp), _lib.ptr(res.kp_count.contiguous()), _lib.ptr(res.match_idx.contiguous()), P, K, *margs,
                      float(reproj_threshold), int(max_iters), int(seed), _lib.ptr(Hm), _lib.ptr(mask), _lib.ptr(nin),
                      _lib.stream_ptr(dev)))
    return Hm, mask, nin


def _pair_refine(fn, res, H, model, reproj_threshold, count, count_name):
    name, margs = _entry('refine', model)
    count = int(count)
    if not float(reproj_threshold) > 0.0:
        raise ValueError('%s: reproj_threshold must be positive' % fn)
    if not 0 <= count <= 1000:
        raise ValueError('%s: %s must be in [0, 1000]' % (fn, count_name))
    P, K = res.num_pairs, res.kp_yx.shape[1]
    Hm = torch.as_tensor(H, dtype=torch.float64)
    if Hm.numel() != P * 9:
        raise ValueError('%s: need one 3x3 matrix per pair (%d), got %d values' % (fn, P, Hm.numel()))
    res.wait()
    dev = res.kp_yx.device
    Hm = Hm.to(dev).reshape(P, 3, 3).clone().contiguous()                    # (refined in place: never the caller's tensor)
    mask = torch.empty((P, K), dtype=torch.uint8, device=dev)
    nin = torch.empty((P,), dtype=torch.int32, device=dev)
    cost = torch.empty((P, 2), dtype=torch.float64, device=dev)
    h = _lib.get_handle(dev)
    entry, kp = _keypoints_for_estimate(res, h, name)
    with torch.cuda.device(dev):
        h.check(entry(h.ptr, _lib.ptr(kp), _lib.ptr(res.kp_count.contiguous()), _lib.ptr(res.match_idx.contiguous()), P, K, *margs,
                      float(reproj_threshold), count, _lib.ptr(Hm), _lib.ptr(mask), _lib.ptr(nin), _lib.ptr(cost),
                      _lib.stream_ptr(dev)))
    return Hm, mask, nin, cost


def find_homography(res, reproj_threshold=3.0, max_iters=2000, seed=0):
    """Batched cv2.findHomography(optical_pts, thermal_pts, cv2.RANSAC, reproj_threshold) for the pairs of a PairResults
    (predict_align_image_pair.py:205-216).  NOT OpenCV's algorithm bit for bit: every pair evaluates `max_iters` 4-point
    hypotheses in parallel (no confidence-driven early stop) and refits the best consensus set by the normalised DLT
    (OpenCV: adaptive iteration bound at confidence 0.995, refit, then a Levenberg-Marquardt polish -- that polish exists
    as a step of its own, refine_homography / refine_alignment, and is opt-in: this function stops at the refit).  Measured against an
    independent restatement of OpenCV 4.2's published algorithm (test infrastructure,
    tests/test_gpu_metrics.py::test_find_homography_against_opencv_semantics; planted homographies, 10-75 % outliers):
    mean corner distance differs by <= 0.11 px, the h_correctness decision (< 3 px) agrees on every pair, the inlier
    masks overlap by IoU >= 0.99 up to 50 % outliers (0.84 at 75 %: OpenCV's mask is the consensus set of its best
    4-point sample).  Returns (H [P,3,3] float64 mapping optical (x,y,1) to thermal -- all zeros
    where the reference would get None --, inlier mask [P,K] uint8 per optical keypoint, n_inliers [P] int32).
    Results that carry sub-pixel keypoints (res.kp_sub, prediction.subpixel) are estimated from those (mp_find_homography_f);
    so are refine_homography, refine_alignment's estimates and polish, pool_matches and estimate_shared_homography."""
    return _pair_find(res, None, reproj_threshold, max_iters, seed)


def refine_homography(res, H, reproj_threshold=3.0, iters=10):
    """The Levenberg-Marquardt polish that closes cv2.findHomography(..., cv2.RANSAC, thr), batched (mp_refine_homography):
    `H` ([P,3,3] or [P,9] float64, find_homography's estimate) is polished over the matches of `res` whose forward
    reprojection error under H is <= reproj_threshold (recomputed, so `res` may hold any matcher's list).
    Returns (H [P,3,3] float64 (h22 = 1; all zeros where the input is all zeros or fewer than 4 matches are inliers),
    mask [P,K] uint8 and n_inliers [P] int32 of that inlier set, cost [P,2] float64: the sum of squared residuals over it
    before / after)."""
    return _pair_refine('refine_homography', res, H, None, reproj_threshold, iters, 'iters')


def refine_alignment(res, reproj_threshold=3.0, radius=None, rounds=1, polish=True, max_iters=2000, seed=0, threshold=-1.0,
                     model='homography'):
    """Guided re-matching and a polished homography for the pairs of a PairResults with mutual matches (an extension; the
    reference stops at cv2.findHomography on the first match list):
      1. find_homography on the matches of `res`;
      2. `rounds` times: guided_pairs under the current estimate (partners within `radius` pixels of where the estimate
         maps a keypoint; default 2 * reproj_threshold; `threshold` as for match_pairs), then find_homography on the new list;
      3. with `polish`, refine_homography.
    A pair without a first estimate keeps its original matches and a zero matrix.  `res` is not modified.  With sub-pixel
    keypoints on `res` (kp_sub) the estimates and the polish read them; the gate of the re-matching stays on the integer pixels
    (it is several pixels wide).  `model` 'similarity' or 'affine': steps 1 to 3 use find_transform and refine_transform (local
    optimisation in the place of the polish) with that model; the default is unchanged, bit for bit.
    Returns (res2, H [P,3,3] float64, mask [P,K] uint8, n_inliers [P] int32); res2 is a new PairResults that shares the
    keypoints and descriptors of `res`, holds the final match list and has match_mode 'guided'."""
    from ..pipeline import PairResults
    from .matching import guided_pairs
    if getattr(res, 'match_mode', 'mutual') != 'mutual':
        raise ValueError("refine_alignment starts from mutual matches; these results were matched in '%s' mode" % res.match_mode)
    rounds = int(rounds)
    if rounds < 0:
        raise ValueError('refine_alignment: rounds must be >= 0')
    radius = 2.0 * float(reproj_threshold) if radius is None else float(radius)
    if not (radius > 0.0 and np.isfinite(radius)):
        raise ValueError('refine_alignment: radius must be finite and positive, got %r' % radius)
    def find(r):
        return find_transform(r, model, reproj_threshold, max_iters, seed)
    H, mask, nin = find(res)
    cur = res
    if rounds > 0:
        K, D = res.desc.shape[1:]
        none = (nin < transform_min_inliers(model))          # no first estimate (zero matrix): the original matches stay
        for _ in range(rounds):
            mi, md, mc = guided_pairs(res.desc, res.kp_count, res.desc[1:], res.kp_count[1:], res.kp_yx, res.kp_yx[1:], H,
                                      radius, threshold, pair_stride=2 * K * D, count_stride=2)
            mi = torch.where(none[:, None], res.match_idx, mi)
            md = torch.where(none[:, None], res.match_dist, md)
            mc = torch.where(none, res.match_count, mc)
            cur = PairResults(res.kp_yx, res.kp_score, res.kp_count, res.desc, mi, md, mc, res.H, res.W, 'guided',
                              kp_sub=getattr(res, 'kp_sub', None))
            H, mask, nin = find(cur)
    if cur is res:
        cur = PairResults(res.kp_yx, res.kp_score, res.kp_count, res.desc, res.match_idx, res.match_dist, res.match_count,
                          res.H, res.W, 'guided', kp_sub=getattr(res, 'kp_sub', None))
    if polish:
        H, mask, nin, _ = refine_transform(cur, H, model, reproj_threshold)
    return cur, H, mask, nin


MAX_RANSAC_MATCHES = 3200        # mp_find_homography keeps a pair's correspondences in LDS


def _points_find(fn, optical_pts, thermal_pts, model, reproj_threshold, max_iters, seed, device):
    from ..pipeline import PairResults
    kind = 'homography' if model is None else model
    min_inliers = transform_min_inliers(kind)
    a = np.asarray(optical_pts).reshape(-1, 2); b = np.asarray(thermal_pts).reshape(-1, 2)
    n = len(a)
    if len(b) != n:
        raise ValueError('%s: %d optical and %d thermal points' % (fn, n, len(b)))
    if n < TRANSFORM_MIN_POINTS[kind]:
        return None, np.zeros(n, np.uint8)
    if n > MAX_RANSAC_MATCHES:
        raise ValueError('%s: at most %d correspondences per call (the pair\'s matches live in LDS); '
                         'got %d -- keep the closest ones' % (fn, MAX_RANSAC_MATCHES, n))
    dev = _lib.require_cuda(device)
    kp = torch.zeros((2, n, 2), dtype=torch.int32)
    kp[0] = torch.from_numpy(np.ascontiguousarray(a[:, ::-1]).astype(np.int32)); kp[1] = torch.from_numpy(np.ascontiguousarray(b[:, ::-1]).astype(np.int32))
    sub = None
    if a.dtype.kind == 'f' or b.dtype.kind == 'f':
        sub = torch.from_numpy(np.stack([a[:, ::-1], b[:, ::-1]]).astype(np.float32)).to(dev)
    res = PairResults(kp.to(dev), None, torch.tensor([n, n], dtype=torch.int32, device=dev), None,
                      torch.arange(n, dtype=torch.int32, device=dev).reshape(1, n), None, None, 0, 0, kp_sub=sub)
    Hm, mask, nin = _pair_find(res, model, reproj_threshold, max_iters, seed)
    if int(nin[0]) < min_inliers:
        return None, np.zeros(n, np.uint8)
    return Hm[0].cpu().numpy(), mask[0].cpu().numpy()


def find_homography_points(optical_pts, thermal_pts, reproj_threshold=3.0, max_iters=2000, seed=0, device=None):
    """cv2.findHomography(optical_pts, thermal_pts, cv2.RANSAC, reproj_threshold) for ONE set of corresponding (x, y)
    points.  Integer input (pixel positions, as torch.nonzero's keypoints are) goes through mp_find_homography; floating
    input (sub-pixel positions) is kept as float32 and goes through mp_find_homography_f, as cv2.findHomography takes float
    points.  Returns (H 3x3 float64 numpy or None, mask (N,) uint8)."""
    return _points_find('find_homography_points', optical_pts, thermal_pts, None, reproj_threshold, max_iters, seed, device)


# ----------------------------------------------------------------------------------------------------------------------
# pooled homography: one model per GROUP of pairs (mp_pool_matches, mp_find_homography_pooled, mp_refine_homography_pooled)
# ----------------------------------------------------------------------------------------------------------------------
PooledMatches = collections.namedtuple('PooledMatches', 'pts query_index pair_offsets group_offsets')
PooledMatches.__doc__ = """The usable matches of P pairs as one compact device list (pool_matches):
pts [N,4] float32 (x, y optical, u, v thermal), pair-major and in query order inside a pair; query_index [N] int32, the optical
keypoint of each row; pair_offsets [P+1] int32 and group_offsets [G+1] int32, the rows a pair / a group owns."""
SharedHomography = collections.namedtuple('SharedHomography', 'H mask n_inliers cost pooled')

MAX_POOLED_MATCHES = (1 << 24) - 1    # rows of one pooled call
MAX_POOLED_GROUPS = 65535
MAX_POOLED_ITERS = 1 << 20


def pooled_chunk():
    """(points per staged LDS chunk of the pooled scoring kernel, most point splits of a launch): the group sizes at which the
    kernel changes path."""
    c, s = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load_library().mp_pooled_chunk(ctypes.byref(c), ctypes.byref(s)))
    return c.value, s.value


def _pooled_workspace(h, P, G, T, dev):
    n = ctypes.c_longlong()
    h.check(h.lib.mp_pooled_workspace_bytes(int(P), int(G), int(T), ctypes.byref(n)))
    return torch.empty((max(n.value, 16),), dtype=torch.uint8, device=dev)


def _group_ids(groups, P):
    """The group id of every pair as a host int32 array and the number of groups; None, 1 for one group."""
    if groups is None:
        return None, 1
    g = groups.detach().cpu().numpy() if isinstance(groups, torch.Tensor) else np.asarray(groups)
    if g.shape != (P,) or g.dtype.kind not in 'iu':
        raise ValueError('pool_matches: groups must be %d integers, one per pair; got shape %s, dtype %s' % (P, g.shape, g.dtype))
    if P and int(g.min()) < 0:
        raise ValueError('pool_matches: group ids must be non-negative')
    if (np.diff(g.astype(np.int64)) < 0).any():
        raise ValueError('pool_matches: group ids must be non-decreasing (a group is a contiguous run of pairs)')
    G = int(g.max()) + 1 if P else 1
    if G > MAX_POOLED_GROUPS:
        raise ValueError('pool_matches: at most %d groups, got %d' % (MAX_POOLED_GROUPS, G))
    return np.ascontiguousarray(g, dtype=np.int32), G


def pool_matches(res, groups=None):
    """The matches of the pairs of a PairResults as one compact list (mp_pool_matches), for estimating ONE homography per group
    of pairs.  `groups`: the group id of every pair, non-decreasing (a group is a contiguous run of pairs; ids without a pair
    are empty groups), default: all pairs in one group.  A match is dropped as the per-pair estimate drops it (no partner, or
    a partner index beyond the thermal list).  Returns a PooledMatches; synchronises once to learn the number of matches."""
    P, K = res.num_pairs, res.kp_yx.shape[1]
    gid, G = _group_ids(groups, P)
    if P <= 0 or K <= 0 or P * K > 0x7fffffff:
        raise ValueError('pool_matches: need P > 0, K > 0 and P * K < 2^31; got P = %d, K = %d' % (P, K))
    res.wait()
    dev = res.kp_yx.device
    pts = torch.empty((P * K, 4), dtype=torch.float32, device=dev)
    qidx = torch.empty((P * K,), dtype=torch.int32, device=dev)
    po = torch.empty((P + 1,), dtype=torch.int32, device=dev)
    go = torch.empty((G + 1,), dtype=torch.int32, device=dev)
    gdev = torch.from_numpy(gid).to(dev) if gid is not None else None
    h = _lib.get_handle(dev)
    entry, kp = _keypoints_for_estimate(res, h, 'mp_pool_matches')
    with torch.cuda.device(dev):
        ws = _pooled_workspace(h, P, G, 1, dev)
        h.check(entry(h.ptr, _lib.ptr(kp), _lib.ptr(res.kp_count.contiguous()),
                      _lib.ptr(res.match_idx.contiguous()), _lib.ptr(gdev), P, K, G, _lib.ptr(pts), _lib.ptr(qidx),
                      P * K, _lib.ptr(po), _lib.ptr(go), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    n = int(po[P])
    return PooledMatches(pts[:n], qidx[:n], po, go)


def _check_pooled(fn, pooled, reproj_threshold):
    if not float(reproj_threshold) > 0.0:
        raise ValueError('%s: reproj_threshold must be positive' % fn)
    pts, go = pooled.pts, pooled.group_offsets
    if pts.dim() != 2 or pts.shape[1] != 4 or pts.dtype != torch.float32:
        raise ValueError('%s: pts must be [N,4] float32, got %s %s' % (fn, tuple(pts.shape), pts.dtype))
    if pts.shape[0] > MAX_POOLED_MATCHES:
        raise ValueError('%s: at most %d correspondences per call, got %d' % (fn, MAX_POOLED_MATCHES, pts.shape[0]))
    if go.dim() != 1 or go.dtype != torch.int32 or not 2 <= go.numel() <= MAX_POOLED_GROUPS + 1:
        raise ValueError('%s: group_offsets must be [G+1] int32 with 1 <= G <= %d' % (fn, MAX_POOLED_GROUPS))
    return pts.shape[0], go.numel() - 1


def _pooled_find(fn, pooled, model, reproj_threshold, max_iters, seed):
    name, margs = _entry('find', model, '_pooled')
    max_iters = int(max_iters)
    N, G = _check_pooled(fn, pooled, reproj_threshold)
    if not 0 < max_iters <= MAX_POOLED_ITERS:
        raise ValueError('%s: max_iters must be in [1, %d]' % (fn, MAX_POOLED_ITERS))
    dev = pooled.pts.device
    pts = pooled.pts.contiguous()
    Hm = torch.empty((G, 3, 3), dtype=torch.float64, device=dev)
    mask = torch.empty((N,), dtype=torch.uint8, device=dev)
    nin = torch.empty((G,), dtype=torch.int32, device=dev)
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        ws = _pooled_workspace(h, 0, G, max_iters, dev)
        h.check(getattr(h.lib, name)(h.ptr, _lib.ptr(pts), _lib.ptr(pooled.group_offsets.contiguous()), N, G, *margs,
                                     float(reproj_threshold), max_iters, int(seed), _lib.ptr(Hm), _lib.ptr(mask), _lib.ptr(nin),
                                     _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
    return Hm, mask, nin


def _pooled_refine(fn, pooled, H, model, reproj_threshold, count, count_name):
    name, margs = _entry('refine', model, '_pooled')
    count = int(count)
    N, G = _check_pooled(fn, pooled, reproj_threshold)
    if not 0 <= count <= 1000:
        raise ValueError('%s: %s must be in [0, 1000]' % (fn, count_name))
    Hm = torch.as_tensor(H, dtype=torch.float64)
    if Hm.numel() != G * 9:
        raise ValueError('%s: need one 3x3 matrix per group (%d), got %d values' % (fn, G, Hm.numel()))
    dev = pooled.pts.device
    pts = pooled.pts.contiguous()
    Hm = Hm.to(dev).reshape(G, 3, 3).clone().contiguous()                    # (refined in place: never the caller's tensor)
    mask = torch.empty((N,), dtype=torch.uint8, device=dev)
    nin = torch.empty((G,), dtype=torch.int32, device=dev)
    cost = torch.empty((G, 2), dtype=torch.float64, device=dev)
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(getattr(h.lib, name)(h.ptr, _lib.ptr(pts), _lib.ptr(pooled.group_offsets.contiguous()), N, G, *margs,
                                     float(reproj_threshold), count, _lib.ptr(Hm), _lib.ptr(mask), _lib.ptr(nin), _lib.ptr(cost),
                                     _lib.stream_ptr(dev)))
    return Hm, mask, nin, cost


def _shared_estimate(fn, res, groups, model, reproj_threshold, max_iters, seed, polish, count, count_name):
    _entry('find', model)                                                    # (an unknown model is refused first)
    if not float(reproj_threshold) > 0.0:
        raise ValueError('%s: reproj_threshold must be positive' % fn)
    if not 0 < int(max_iters) <= MAX_POOLED_ITERS:
        raise ValueError('%s: max_iters must be in [1, %d]' % (fn, MAX_POOLED_ITERS))
    if not 0 <= int(count) <= 1000:
        raise ValueError('%s: %s must be in [0, 1000]' % (fn, count_name))
    pooled = pool_matches(res, groups)
    H, mask, nin = _pooled_find(fn, pooled, model, reproj_threshold, max_iters, seed)
    cost = None
    if polish:
        H, mask, nin, cost = _pooled_refine(fn, pooled, H, model, reproj_threshold, count, count_name)
    return SharedHomography(H, mask, nin, cost, pooled)


def find_homography_pooled(pooled, reproj_threshold=3.0, max_iters=2000, seed=0):
    """One RANSAC homography per group of a PooledMatches (mp_find_homography_pooled): find_homography's algorithm with the
    group in the place of the pair -- `max_iters` hypotheses per group from 4 of its correspondences, the most inliers win, the
    winner's inliers are refitted by the normalised DLT -- on lists of any length.  Returns (H [G,3,3] float64 optical (x,y,1)
    -> thermal, all zeros for a group with fewer than 4 correspondences or without a model; mask [N] uint8, one per row of
    pooled.pts; n_inliers [G] int32).  The same input gives the same bits on every run."""
    return _pooled_find('find_homography_pooled', pooled, None, reproj_threshold, max_iters, seed)


def refine_homography_pooled(pooled, H, reproj_threshold=3.0, iters=10):
    """refine_homography on the groups of a PooledMatches (mp_refine_homography_pooled): `H` ([G,3,3] or [G,9] float64) is
    polished over the group's correspondences within reproj_threshold of it.  Returns (H [G,3,3] float64 with h22 = 1, all zeros
    where the input is all zeros or has fewer than 4 inliers; mask [N] uint8 and n_inliers [G] int32 of the INPUT estimate's
    inlier set; cost [G,2] float64: the sum of squared residuals over it before / after)."""
    return _pooled_refine('refine_homography_pooled', pooled, H, None, reproj_threshold, iters, 'iters')


def estimate_shared_homography(res, groups=None, reproj_threshold=3.0, max_iters=2000, seed=0, polish=True, iters=10):
    """One homography per group of pairs that share a transform (a fixed rig: one group for the whole recording): pool_matches,
    find_homography_pooled and, with `polish`, refine_homography_pooled.  Returns a SharedHomography: H [G,3,3] float64, mask [N]
    uint8 per pooled match, n_inliers [G] int32, cost [G,2] float64 before / after the polish (None without it) and the
    PooledMatches (its pair_offsets / query_index lead from a mask byte back to the pair and the optical keypoint)."""
    return _shared_estimate('estimate_shared_homography', res, groups, None, reproj_threshold, max_iters, seed, polish, iters, 'iters')


def find_homography_pooled_points(optical_xy, thermal_xy, reproj_threshold=3.0, max_iters=2000, seed=0, device=None):
    """find_homography_pooled for ONE set of corresponding (x, y) points of any length, taken as float32 (sub-pixel positions
    are kept; find_homography_points, with its 3200 limit and integer positions, stays what the per-pair drivers use).
    Returns (H 3x3 float64 numpy or None, mask (N,) uint8)."""
    a = np.asarray(optical_xy, dtype=np.float32).reshape(-1, 2); b = np.asarray(thermal_xy, dtype=np.float32).reshape(-1, 2)
    n = len(a)
    if len(b) != n:
        raise ValueError('find_homography_pooled_points: %d optical and %d thermal points' % (n, len(b)))
    if n > MAX_POOLED_MATCHES:
        raise ValueError('find_homography_pooled_points: at most %d correspondences per call, got %d' % (MAX_POOLED_MATCHES, n))
    if not float(reproj_threshold) > 0.0:
        raise ValueError('find_homography_pooled_points: reproj_threshold must be positive')
    if not 0 < int(max_iters) <= MAX_POOLED_ITERS:
        raise ValueError('find_homography_pooled_points: max_iters must be in [1, %d]' % MAX_POOLED_ITERS)
    if n < 4:
        return None, np.zeros(n, np.uint8)
    dev = _lib.require_cuda(device)
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate([a, b], 1))).to(dev)
    pooled = PooledMatches(pts, None, None, torch.tensor([0, n], dtype=torch.int32, device=dev))
    Hm, mask, nin = find_homography_pooled(pooled, reproj_threshold, max_iters, seed)
    if int(nin[0]) < 4:
        return None, np.zeros(n, np.uint8)
    return Hm[0].cpu().numpy(), mask.cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------------
# the same routes with a choice of motion model (mp_find_transform*, mp_refine_transform*)
# ----------------------------------------------------------------------------------------------------------------------
def find_transform(res, model, reproj_threshold=3.0, max_iters=2000, seed=0):
    """find_homography with a choice of motion model (mp_find_transform): 'homography' (find_homography itself, the same bits),
    'similarity' [[a, -b, tx], [b, a, ty], [0, 0, 1]] (rotation, scale, two translations: what the reference's manual
    alignment gets from cv2.estimateRigidTransform(ir, opt, False)) or 'affine' [[a, b, tx], [c, d, ty], [0, 0, 1]].  The two
    new models draw `max_iters` hypotheses from 2 / 3 matches each, keep the one with the most inliers and refit it by exact
    least squares over them; a rig's few correct cross-spectral matches determine 4 or 6 parameters where they do not
    determine 8.  NOT cv2.estimateAffinePartial2D / estimateAffine2D bit for bit, and without their adaptive iteration bound.
    Returns what find_homography returns: (H [P,3,3] float64 optical (x,y,1) -> thermal, all zeros where there is no model
    (fewer than transform_min_inliers(model) inliers); mask [P,K] uint8 per optical keypoint; n_inliers [P] int32).  Sub-pixel
    keypoints on `res` (kp_sub) are read as find_homography reads them."""
    return _pair_find(res, model, reproj_threshold, max_iters, seed)


def refine_transform(res, H, model, reproj_threshold=3.0, rounds=10):
    """refine_homography with a choice of motion model (mp_refine_transform).  'homography': the Levenberg-Marquardt polish,
    `rounds` as its iterations (the same bits).  'similarity' / 'affine': local optimisation -- at most `rounds` times, mark the
    matches within reproj_threshold of the current model and refit it by exact least squares over them; a marking that changes
    nothing ends it.  Returns (H [P,3,3] float64, mask [P,K] uint8 and n_inliers [P] int32 of the last set marked -- the one
    the returned model was fitted to, the input's own with rounds = 0 --, cost [P,2] float64: the summed squared error over
    that set before / after the last refit).  All zeros where the input is all zeros or a set has fewer than
    transform_min_inliers(model) members."""
    return _pair_refine('refine_transform', res, H, model, reproj_threshold, rounds, 'rounds')


def find_transform_points(optical_pts, thermal_pts, model, reproj_threshold=3.0, max_iters=2000, seed=0, device=None):
    """find_homography_points with a choice of motion model: ONE set of corresponding (x, y) points, integer input through
    mp_find_transform and floating input, kept as float32, through mp_find_transform_f.  Returns (H 3x3 float64 numpy or None,
    mask (N,) uint8); None with fewer points than the model's minimal sample or without a model."""
    return _points_find('find_transform_points', optical_pts, thermal_pts, model, reproj_threshold, max_iters, seed, device)


def find_transform_pooled(pooled, model, reproj_threshold=3.0, max_iters=2000, seed=0):
    """find_homography_pooled with a choice of motion model (mp_find_transform_pooled): one model per group of a PooledMatches.
    Returns (H [G,3,3] float64, mask [N] uint8 per row of pooled.pts, n_inliers [G] int32)."""
    return _pooled_find('find_transform_pooled', pooled, model, reproj_threshold, max_iters, seed)


def refine_transform_pooled(pooled, H, model, reproj_threshold=3.0, rounds=10):
    """refine_transform on the groups of a PooledMatches (mp_refine_transform_pooled).  Returns (H [G,3,3] float64, mask [N]
    uint8, n_inliers [G] int32, cost [G,2] float64), as refine_transform describes them."""
    return _pooled_refine('refine_transform_pooled', pooled, H, model, reproj_threshold, rounds, 'rounds')


def estimate_shared_transform(res, groups=None, model='similarity', reproj_threshold=3.0, max_iters=2000, seed=0, polish=True,
                              rounds=10):
    """estimate_shared_homography with a choice of motion model: pool_matches, find_transform_pooled and, with `polish`,
    refine_transform_pooled (`rounds` of local optimisation; the polish's iterations for 'homography').  Returns a
    SharedHomography, as estimate_shared_homography does."""
    return _shared_estimate('estimate_shared_transform', res, groups, model, reproj_threshold, max_iters, seed, polish, rounds,
                            'rounds')


def decompose_similarity(H):
    """(angle, scale, dx, dy) of a similarity [[a, -b, tx], [b, a, ty], [0, 0, 1]] in the convention of the reference's
    optimiser (create_dataset/helper_functions/align.py:196-200, :210-211): angle = arctan2(H[0,1], H[0,0]), scale =
    H[0,0] / cos(angle) -- computed as hypot(H[0,0], H[0,1]), the same number without the division by a cosine near zero --,
    dx = H[0,2], dy = H[1,2]; the matrix is [[s cos, s sin, dx], [-s sin, s cos, dy]] again.  H is divided by H[2,2] first."""
    m = np.asarray(H.detach().cpu() if isinstance(H, torch.Tensor) else H, dtype=np.float64).reshape(3, 3)
    if not (np.isfinite(m).all() and m[2, 2] != 0.0):
        raise ValueError('decompose_similarity: need a finite 3x3 matrix with H[2,2] != 0')
    m = m / m[2, 2]
    return float(np.arctan2(m[0, 1], m[0, 0])), float(np.hypot(m[0, 0], m[0, 1])), float(m[0, 2]), float(m[1, 2])


def compose_similarity(angle, scale, dx, dy):
    """The 3x3 matrix decompose_similarity takes apart."""
    c, s = scale * np.cos(angle), scale * np.sin(angle)
    return np.array([[c, s, dx], [-s, c, dy], [0.0, 0.0, 1.0]])


def _warp_yx(pts_yx, hmat):
    """warp_keypoints(..., np.float) for a handful of points (homographies.py:331-346)."""
    p = np.asarray(pts_yx, dtype=np.float64)
    m = np.asarray(hmat, dtype=np.float64).reshape(3, 3)
    xy1 = np.concatenate([p[:, ::-1], np.ones((len(p), 1))], 1) @ m.T
    return (xy1[:, :2] / xy1[:, 2:3])[:, ::-1]


def _refinement_config(config):
    """refine_alignment's keyword arguments from prediction.alignment_refinement, or None when it is absent or disabled."""
    cfg = config.get('alignment_refinement') or {}
    unknown = set(cfg) - {'enable', 'radius', 'rounds', 'polish'}
    if unknown:
        raise ValueError('alignment_refinement: unknown key(s) %s' % sorted(unknown))
    if not cfg.get('enable', False):
        return None
    return {'radius': cfg.get('radius'), 'rounds': int(cfg.get('rounds', 1)), 'polish': bool(cfg.get('polish', True))}


def compute_descriptor_metrics(net, dataloader, device, config, threshold_keypoints, threshold_warp=None):
    """Same signature and result keys as the reference function (evaluation.py:209).
    Extension: config['alignment_refinement'] = {enable: false, radius: null, rounds: 1, polish: true}.  With enable: true
    every batch's mutual matches additionally go through refine_alignment (guided re-matching under the first estimate,
    then the Levenberg-Marquardt polish) and the result gains pts_dist_refined / average_h_error_refined /
    h_correctness_refined (as their unrefined namesakes, from the refined estimate) and n_matches_refined (matches per
    pair after re-matching).  Every other key keeps its value; without enable there is no new key.
    Extension: config['subpixel'] = {enable: false}.  With enable: true the pipeline refines its keypoint lists and samples the
    descriptors at the refined positions, and every homography estimate here reads the sub-pixel positions; the keypoint
    metrics (mp_pair_metrics) stay on the integer pixels, the reference's definitions.
    Extension: config['transform_model'] = 'homography' | 'similarity' | 'affine' (default, and when absent: 'homography',
    nothing changes).  With another model every estimate here, the refinement's included, is find_transform's."""
    from ..pipeline import PairPipeline, PairResults
    from .utils import data_to_device
    from .matching import get_matches, match_pairs, nearest_pairs
    # The metrics are ALWAYS computed on cv2.BFMatcher(crossCheck=True) matches, whatever the config says -- the
    # reference hard-codes that matcher for matches_optical / matches_thermal (evaluation.py:273-282) and uses
    # config['matching'] only for the matches the homography is estimated from (:332-336).
    metric_matching = {'method': 'bfmatcher', 'method_kwargs': {'crossCheck': True}, 'knn_matches': False}
    mcfg = config.get('matching', metric_matching)
    same_matcher = (mcfg.get('method', 'bfmatcher') == 'bfmatcher' and not mcfg.get('knn_matches', False)
                    and dict(mcfg.get('method_kwargs', {})) == {'crossCheck': True})
    pipe = PairPipeline(net, dict(config, matching=metric_matching))
    # another ONE-match-per-keypoint matcher for the homography estimate (nnmatcher, bfmatcher without crossCheck, the ratio
    # test) is batched like the default one; PairPipeline reads the configuration and raises what get_matches raises
    sel = None
    if not same_matcher and mcfg.get('method') in ('bfmatcher', 'nnmatcher'):
        sel = PairPipeline(None, dict(config, matching=mcfg))
    refine = _refinement_config(config)
    model = config.get('transform_model', 'homography')
    min_in, min_pts = transform_min_inliers(model), TRANSFORM_MIN_POINTS[model]
    if refine is not None and model != 'homography':
        refine = dict(refine, model=model)
    pts_dist_ref, n_matches_ref = [], []
    tp_o, tp_t, dist_o, dist_t, ms_o, ms_t, pts_dist = [], [], [], [], [], [], []
    n_gt_o = n_gt_t = 0
    for data in dataloader:
        data = data_to_device(data, device)
        opt, th = data['optical'], data['thermal']
        B = opt['image'].shape[0]
        eye = torch.eye(3, dtype=torch.float32).repeat(B, 1, 1)
        ho = opt.get('homography', eye)
        ht = th.get('homography', eye)
        res = pipe(opt['image'], th['image'], opt.get('valid_mask'), th.get('valid_mask'))
        gth = ground_truth_homographies(ho, ht)
        metrics, tp = pair_metrics(res, gth, threshold_keypoints)
        pipe.check_converged()
        est = res if same_matcher else None
        if sel is not None and res.kp_yx.shape[1] <= MAX_RANSAC_MATCHES:
            # all pairs in one launch, on the result's own descriptor lists in place, then one batched RANSAC call
            Kc, Dc = res.desc.shape[1:]
            lay = dict(pair_stride=2 * Kc * Dc, count_stride=2)
            if sel.match_mode == 'mutual':
                mm = match_pairs(res.desc, res.kp_count, res.desc[1:], res.kp_count[1:], sel.match_threshold, **lay)
            else:
                mm = nearest_pairs(res.desc, res.kp_count, res.desc[1:], res.kp_count[1:], sel.match_ratio or None, **lay)
            est = PairResults(res.kp_yx, res.kp_score, res.kp_count, res.desc, mm[0], mm[1], mm[2], res.H, res.W,
                              sel.match_mode, kp_sub=res.kp_sub)
        if est is not None:
            h_est, _, n_in = find_transform(est, model, config.get('reprojection_threshold', 3))
            h_est = h_est.cpu().numpy(); n_in = n_in.cpu().numpy()
        else:
            # one-to-many matchers (thresholdmatcher) and lists longer than one RANSAC launch holds: per pair through
            # get_matches (GPU), like the reference
            h_est = np.zeros((B, 3, 3)); n_in = np.zeros(B, dtype=np.int64)
            kp_all = (res.kp_yx if res.kp_sub is None else res.kp_sub).cpu().numpy(); cnt_all = res.kp_count.cpu().numpy()
            Kc = kp_all.shape[1]
            for p in range(B):
                no, nt = min(int(cnt_all[2 * p]), Kc), min(int(cnt_all[2 * p + 1]), Kc)
                if no == 0 or nt == 0:
                    continue
                matches = get_matches(res.desc[2 * p, :no], res.desc[2 * p + 1, :nt], mcfg['method'],
                                      mcfg.get('knn_matches', False), **mcfg.get('method_kwargs', {}))
                if len(matches) < min_pts:
                    continue
                if len(matches) > MAX_RANSAC_MATCHES:           # one-to-many matchers (thresholdmatcher): closest first
                    matches = sorted(matches, key=lambda mm: mm.distance)[:MAX_RANSAC_MATCHES]
                opts = np.array([kp_all[2 * p, mm.queryIdx][::-1] for mm in matches])
                tpts = np.array([kp_all[2 * p + 1, mm.trainIdx][::-1] for mm in matches])
                hp, mask = find_transform_points(opts, tpts, model, config.get('reprojection_threshold', 3), device=device)
                if hp is not None:
                    h_est[p] = hp; n_in[p] = int(mask.sum())
        if refine is not None:
            if res.kp_yx.shape[1] > MAX_RANSAC_MATCHES:
                raise ValueError('alignment_refinement: at most %d keypoints per image (the RANSAC launch keeps a pair\'s '
                                 'matches in LDS)' % MAX_RANSAC_MATCHES)
            res_r, h_ref, _, n_in_ref = refine_alignment(res, config.get('reprojection_threshold', 3), **refine)
            h_ref = h_ref.cpu().numpy(); n_in_ref = n_in_ref.cpu().numpy()
            n_matches_ref.extend(int(c) for c in res_r.match_count.cpu().numpy())
        H_o, W_o = opt['image'].shape[2:]
        m = metrics.cpu().numpy(); tp = tp.cpu().numpy()
        midx = res.match_idx.cpu().numpy(); mdist = res.match_dist.cpu().numpy()
        cnt = res.kp_count.cpu().numpy()
        K = midx.shape[1]
        for p in range(B):
            no = min(int(cnt[2 * p]), K)
            q = np.nonzero(midx[p, :no] >= 0)[0]
            # matches_optical (query = optical) and matches_thermal (query = thermal) are the same mutual pairs
            # (evaluation.py:273-282); their order does not matter, everything is re-sorted by distance below
            tp_o.append(tp[2 * p, q].astype(bool)); dist_o.append(mdist[p, q])
            tp_t.append(tp[2 * p + 1, midx[p, q]].astype(bool)); dist_t.append(mdist[p, q])
            n_gt_o += int(m[p, 0]); n_gt_t += int(m[p, 1])
            ms_o.append(float(m[p, 2]) / m[p, 4] if m[p, 4] > 0 else 0.0)
            ms_t.append(float(m[p, 3]) / m[p, 5] if m[p, 5] > 0 else 0.0)
            # homography correctness (:351-356; the reference's corner list, including its (H_o, H_o) last point)
            if n_in[p] >= min_in:
                pts = np.array([[0, 0], [H_o, 0], [0, W_o], [H_o, H_o]])
                gt = gth[2 * p].numpy().reshape(3, 3)
                pts_dist.append(np.linalg.norm(_warp_yx(pts, h_est[p]) - _warp_yx(pts, gt), axis=1).sum() / 4)
            else:
                pts_dist.append(999.0)
            if refine is not None:
                if n_in_ref[p] >= min_in:
                    pts = np.array([[0, 0], [H_o, 0], [0, W_o], [H_o, H_o]])
                    gt = gth[2 * p].numpy().reshape(3, 3)
                    pts_dist_ref.append(np.linalg.norm(_warp_yx(pts, h_ref[p]) - _warp_yx(pts, gt), axis=1).sum() / 4)
                else:
                    pts_dist_ref.append(999.0)
    out = summarize_descriptor_metrics(np.concatenate(tp_o) if tp_o else np.zeros(0, bool),
                                        np.concatenate(dist_o) if dist_o else np.zeros(0, np.float32),
                                        np.concatenate(tp_t) if tp_t else np.zeros(0, bool),
                                        np.concatenate(dist_t) if dist_t else np.zeros(0, np.float32),
                                        n_gt_o, n_gt_t, np.array(ms_o), np.array(ms_t))
    pts_dist = np.array(pts_dist)
    out['pts_dist'] = pts_dist
    out['average_h_error'] = pts_dist.mean() if len(pts_dist) else None
    out['h_correctness'] = (pts_dist < threshold_warp).sum() / len(pts_dist) if len(pts_dist) and threshold_warp is not None else None
    if refine is not None:
        pts_dist_ref = np.array(pts_dist_ref)
        out['pts_dist_refined'] = pts_dist_ref
        out['average_h_error_refined'] = pts_dist_ref.mean() if len(pts_dist_ref) else None
        out['h_correctness_refined'] = ((pts_dist_ref < threshold_warp).sum() / len(pts_dist_ref)
                                        if len(pts_dist_ref) and threshold_warp is not None else None)
        out['n_matches_refined'] = np.array(n_matches_ref, dtype=np.int64)
    return out


def summarize_descriptor_metrics(tp_optical, distance_optical, tp_thermal, distance_thermal, n_gt_optical,
                                 n_gt_thermal, m_score_optical, m_score_thermal):
    """evaluation.py:360-439 (precision / recall / NN-mAP / M-score bookkeeping), verbatim arithmetic."""
    sort_o = np.argsort(distance_optical, kind='stable')
    tp_optical = tp_optical[sort_o]; fp_optical = np.logical_not(tp_optical); distance_optical = distance_optical[sort_o]
    sort_t = np.argsort(distance_thermal, kind='stable')
    tp_thermal = tp_thermal[sort_t]; fp_thermal = np.logical_not(tp_thermal); distance_thermal = distance_thermal[sort_t]
    tpo, tpt = np.cumsum(tp_optical), np.cumsum(tp_thermal)
    fpo, fpt = np.cumsum(fp_optical), np.cumsum(fp_thermal)
    recall_optical = div0(tpo, n_gt_optical); recall_thermal = div0(tpt, n_gt_thermal)
    precision_optical = div0(tpo, tpo + fpo); precision_thermal = div0(tpt, tpt + fpt)
    recall_optical = np.concatenate([[0], recall_optical, [1]])
    precision_optical = np.concatenate([[0], precision_optical, [0]])
    precision_optical = np.maximum.accumulate(precision_optical[::-1])[::-1]
    recall_thermal = np.concatenate([[0], recall_thermal, [1]])
    precision_thermal = np.concatenate([[0], precision_thermal, [0]])
    precision_thermal = np.maximum.accumulate(precision_thermal[::-1])[::-1]
    nn_map_optical = compute_mAP(precision_optical, recall_optical)
    nn_map_thermal = compute_mAP(precision_thermal, recall_thermal)
    m_score = (m_score_optical.mean() + m_score_thermal.mean()) * 0.5 if len(m_score_optical) else 0.0
    return {
        'tp_optical': tp_optical, 'tp_thermal': tp_thermal, 'fp_optical': fp_optical, 'fp_thermal': fp_thermal,
        'distance_optical': distance_optical, 'distance_thermal': distance_thermal,
        'recall_optical': recall_optical, 'recall_thermal': recall_thermal,
        'precision_optical': precision_optical, 'precision_thermal': precision_thermal,
        'nn_map_optical': nn_map_optical, 'nn_map_thermal': nn_map_thermal,
        'nn_map': (nn_map_optical + nn_map_thermal) * 0.5,
        'm_score_optical': m_score_optical, 'm_score_thermal': m_score_thermal, 'm_score': m_score,
        'pts_dist': None, 'average_h_error': None, 'h_correctness': None,
    }


def repeatability_counts(kp_yx, kp_count, h_optical, h_thermal, H, W, distance_thresh):
    """GPU arithmetic of evaluation.py:156-199 on interleaved keypoint lists (slot 2p optical, 2p+1 thermal).
    Returns a [P,4] int32 device tensor: count1, count2, N_thermal, N_optical."""
    dev = kp_yx.device
    P = kp_yx.shape[0] // 2
    K = kp_yx.shape[1]
    ho = torch.as_tensor(h_optical, dtype=torch.float32).cpu().reshape(P, 3, 3)
    ht = torch.as_tensor(h_thermal, dtype=torch.float32).cpu().reshape(P, 3, 3)
    hoi, hti = torch.linalg.inv(ho), torch.linalg.inv(ht)          # fp32 like h.squeeze().inverse() (:168,173)
    hom = torch.stack([torch.stack([hoi, ht], 1), torch.stack([hti, ho], 1)], 1)       # [P][slot][warp][3][3]
    hom = hom.reshape(2 * P, 18).to(torch.float64).to(dev).contiguous()
    counts = torch.empty((P, 4), dtype=torch.int32, device=dev)
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_repeatability(h.ptr, _lib.ptr(kp_yx.contiguous()), _lib.ptr(kp_count.contiguous()), _lib.ptr(hom),
                                       P, K, int(H), int(W), float(distance_thresh), _lib.ptr(counts),
                                       _lib.stream_ptr(dev)))
    return counts


def compute_repeatability_multispectral(net, dataloader, device, config, distance_thresh=3, verbose=False):
    """Same signature and return value as the reference (evaluation.py:105-200):
    (mean repeatability, per-sample list, n_kp_optical, n_kp_thermal).  `config` is the whole yaml dict."""
    from .utils import box_nms_tie_robust, data_to_device, extract_keypoints, topk_selection
    pred = config['prediction']
    thr = pred['detection_threshold']
    select = topk_selection(pred)        # prediction.topk_mode / anms_robust (none in the score mode)
    cap = pred['topk'] if pred.get('topk', 0) > 0 else 4096
    repeatability, n_kp_optical, n_kp_thermal = [], [], []
    for data in dataloader:
        B = data['optical']['image'].shape[0]
        eye = torch.eye(3).repeat(B, 1, 1)
        ho = data['optical'].get('homography', eye)
        ht = data['thermal'].get('homography', eye)
        data = data_to_device(data, device)
        img = torch.stack([data['optical']['image'], data['thermal']['image']], 1).flatten(0, 1)     # interleaved
        mask = torch.stack([data['optical']['valid_mask'], data['thermal']['valid_mask']], 1).flatten(0, 1)
        flags = (torch.arange(2 * B) % 2 == 0).reshape(-1, 1)
        fwd_in = {'image': img, 'is_optical': flags}
        fwd = net(fwd_in)
        prob = fwd['prob']
        if pred['nms'] > 0:      # (top-k tie guard: flagged images are re-evaluated with the tie-exact algorithm)
            prob = box_nms_tie_robust(net, fwd_in, fwd, pred['nms'], thr, keep_top_k=pred['topk'], on_cpu=pred.get('cpu_nms', False),
                                      **select)
        # keypoints: nonzero((prob > thr) * mask)  (:156-157) -- the mask is applied AFTER the NMS here
        kp, _, cnt = extract_keypoints(prob, thr, cap, valid_mask=mask)
        H, W = prob.shape[2:]
        c = repeatability_counts(kp, cnt, ho, ht, H, W, distance_thresh).cpu().numpy()
        cnt = cnt.cpu().numpy()
        if (cnt > cap).any():
            raise RuntimeError('more than %d keypoints in an image: set prediction.topk' % cap)
        for p in range(B):
            n_kp_optical.append(int(cnt[2 * p])); n_kp_thermal.append(int(cnt[2 * p + 1]))
            if c[p, 2] + c[p, 3] > 0:
                repeatability.append((c[p, 0] + c[p, 1]) / (c[p, 2] + c[p, 3]))
                if verbose:
                    print('repeatability: %f' % repeatability[-1])
    return np.mean(repeatability), repeatability, n_kp_optical, n_kp_thermal


# ----------------------------------------------------------------------------------------------------------------------
# single-image detector metrics (evaluation.py:10-103; predict_keypoints.py:88-104)
# ----------------------------------------------------------------------------------------------------------------------
_WINDOW_DIST = np.sqrt(np.add.outer((np.arange(5) - 2) ** 2, (np.arange(5) - 2) ** 2).astype(np.float32)).reshape(-1)


def detector_records(prob, keypoint_map, zero_threshold=1e-4, distance_thresh=2.0):
    """GPU arithmetic of compute_tp_fp_dist for a batch: prob (B,H,W) / (B,1,H,W) fp32, keypoint_map (B,H,W) bool.
    Returns per image the tuple of the reference (tp, fp, prob, n_gt, dist) with the predictions ranked by
    (prob descending, row-major index ascending)."""
    if prob.dim() == 4:
        prob = prob[:, 0]
    if prob.dim() != 3 or tuple(keypoint_map.shape) != tuple(prob.shape):
        raise ValueError('detector_records: prob and keypoint_map must both be (B,H,W); got {} and {}'.format(
            tuple(prob.shape), tuple(keypoint_map.shape)))
    dev = _lib.require_cuda(prob.device if prob.device.type == 'cuda' else None)
    p = prob.to(dev, torch.float32).contiguous()
    g = keypoint_map.to(dev).ne(0).to(torch.uint8).contiguous()
    B, H, W = p.shape
    work = torch.empty((B, H * W), dtype=torch.int64, device=dev)
    rec_index = torch.empty((B, H * W), dtype=torch.int32, device=dev)
    rec_prob = torch.empty((B, H * W), dtype=torch.float32, device=dev)
    rec_bits = torch.empty((B, H * W), dtype=torch.int32, device=dev)
    rec_count = torch.empty((B,), dtype=torch.int32, device=dev)
    n_gt = torch.empty((B,), dtype=torch.int32, device=dev)
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_detector_metrics(h.ptr, _lib.ptr(p), _lib.ptr(g), B, H, W, float(zero_threshold),
                                          float(distance_thresh), _lib.ptr(work), _lib.ptr(rec_index),
                                          _lib.ptr(rec_prob), _lib.ptr(rec_bits), _lib.ptr(rec_count), _lib.ptr(n_gt),
                                          _lib.stream_ptr(dev)))
    cnt = rec_count.cpu().numpy()
    ngt = n_gt.cpu().numpy()
    nmax = int(cnt.max()) if B else 0
    idx = rec_index[:, :nmax].cpu().numpy()
    prb = rec_prob[:, :nmax].cpu().numpy()
    bits = rec_bits[:, :nmax].cpu().numpy().view(np.uint32)
    out = []
    for b in range(B):
        n = int(cnt[b])
        order = np.lexsort((idx[b, :n], -prb[b, :n].astype(np.float64)))        # prob desc, then index asc
        bb = bits[b, :n][order]
        tp = (bb >> np.uint32(31)).astype(bool)
        m = ((bb[:, None] >> np.arange(25, dtype=np.uint32)[None]) & np.uint32(1)).astype(bool)
        dist = np.broadcast_to(_WINDOW_DIST[None], m.shape)[m]                   # (prediction, window row-major) order
        out.append((tp, np.logical_not(tp), prb[b, :n][order], int(ngt[b]), dist.astype(np.float32)))
    return out


def compute_tp_fp_dist(prob, keypoints, zero_threshold=1e-4, distance_thresh=2.0):
    """evaluation.py:56-97 for one (H,W) heat map; `keypoints` is the (H,W) label map or an (N,2) (y,x) list."""
    prob = torch.as_tensor(prob)
    keypoints = torch.as_tensor(keypoints)
    if prob.shape != keypoints.shape:
        kk = keypoints.to(torch.int64).cpu()
        km = torch.zeros(tuple(prob.shape), dtype=torch.bool)
        km[kk[:, 0], kk[:, 1]] = True
        keypoints = km
    return detector_records(prob[None], keypoints[None], zero_threshold, distance_thresh)[0]


def compute_detector_metrics(net, dataloader, device, config):
    """Precision, recall and localisation error of the detector on a single-image loader with 'keypoints' labels;
    same signature and return value as the reference (evaluation.py:10-54): (precision, recall, prob, dist)."""
    from .utils import box_nms, data_to_device
    tp, fp, prob, n_gt, dist = [], [], [], 0, []
    for data in dataloader:
        data = data_to_device(data, device)
        out = net(data)
        if config['nms'] > 0:
            pred = box_nms(out['prob'], config['nms'], config['detection_threshold'], valid_mask=data['valid_mask'])
        else:
            pred = out['prob'] * data['valid_mask'].to(out['prob'].dtype)
        for item in detector_records(pred, data['keypoints']):
            tp.append(item[0]); fp.append(item[1]); prob.append(item[2]); n_gt += item[3]; dist.append(item[4])
    tp, fp = np.concatenate(tp), np.concatenate(fp)
    prob, dist = np.concatenate(prob), np.concatenate(dist)
    # evaluation.py:38-54
    sort_idx = np.argsort(prob)[::-1]
    tp, fp, prob = tp[sort_idx], fp[sort_idx], prob[sort_idx]
    tp_cum, fp_cum = np.cumsum(tp), np.cumsum(fp)
    recall = div0(tp_cum, n_gt)
    precision = div0(tp_cum, tp_cum + fp_cum)
    recall = np.concatenate([[0], recall, [1]])
    precision = np.concatenate([[0], precision, [0]])
    precision = np.maximum.accumulate(precision[::-1])[::-1]
    return precision, recall, prob, dist
