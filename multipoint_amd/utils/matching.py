"""Host-side mirror of multipoint/utils/matching.py: get_matches with the mutual-nearest-neighbour methods of the hot
path ('bfmatcher' with crossCheck=True, 'nnmatcher') and the remaining modes ('bfmatcher' without crossCheck, the
knn_matches ratio test, 'thresholdmatcher'); every distance matrix is evaluated on the GPU and never materialised.
match_pairs / nearest_pairs are the batched entries (all pairs of a batch in one launch, unit rows); get_matches is the
per-pair function of the reference and accepts arbitrary rows.  guided_pairs is match_pairs inside a geometric gate (an
extension: re-matching under a first homography estimate)."""
import ctypes

import numpy as np
import torch

from .. import _lib

__all__ = ['get_matches', 'NNMatcher', 'ThresholdMatcher', 'DMatch', 'match_pairs', 'knn2_pairs', 'nearest_pairs',
           'guided_pairs']


class DMatch:
    """Stand-in for cv2.DMatch (queryIdx, trainIdx, distance) -- cv2 is not a dependency here."""
    __slots__ = ('queryIdx', 'trainIdx', 'distance', 'imgIdx')

    def __init__(self, queryIdx, trainIdx, distance):
        self.queryIdx, self.trainIdx, self.distance, self.imgIdx = int(queryIdx), int(trainIdx), float(distance), 0

    def __repr__(self):
        return 'DMatch(queryIdx=%d, trainIdx=%d, distance=%.6f)' % (self.queryIdx, self.trainIdx, self.distance)


def _pair_layout(descA, countA, descB, countB, pair_stride, count_stride):
    """Addressing of P pairs for the batched matchers.  Default: descA / descB [P,K,D] contiguous, countA / countB [P].
    With `pair_stride` (floats between consecutive pairs) and `count_stride`, descA / descB / countA / countB are
    contiguous views that BEGIN at the first pair's rows / counts and are read in place -- the interleaved lists of
    PairResults: (desc, kp_count, desc[1:], kp_count[1:], pair_stride=2 * K * D, count_stride=2)."""
    K, D = descA.shape[-2:]
    if pair_stride is None:
        P = descA.shape[0]
        return (descA.contiguous(), countA.contiguous(), descB.contiguous(), countB.contiguous(), P, K, D, K * D,
                int(count_stride))
    count_stride = int(count_stride)
    P = (countA.numel() + count_stride - 1) // count_stride
    for d, c in ((descA, countA), (descB, countB)):
        if not (d.is_contiguous() and c.is_contiguous()):
            raise ValueError('strided matching reads contiguous views in place')
        if P < 1 or d.numel() < (P - 1) * pair_stride + K * D or c.numel() < (P - 1) * count_stride + 1:
            raise ValueError('descriptor / count views are shorter than %d pairs at these strides' % P)
    return descA, countA, descB, countB, P, K, D, int(pair_stride), count_stride


def _batched_match(entry, layout, mode, second=None):
    """One call of a batched MFMA matcher on the current stream: `entry` (mp_match_mutual_nn / mp_match_nearest) on the
    pairs `layout` (_pair_layout) addresses, with its mode argument (threshold / ratio).  `second`: None for the entry
    without second-neighbour outputs, else whether to allocate them.
    Returns [match_idx [P,K] int32, match_dist [P,K] f32, match_count [P] int32] (+ [second_idx, second_dist] or Nones)."""
    descA, countA, descB, countB, P, K, D, pair_stride, count_stride = layout
    dev = descA.device
    out = [torch.empty((P, K), dtype=torch.int32, device=dev), torch.empty((P, K), dtype=torch.float32, device=dev),
           torch.empty((P,), dtype=torch.int32, device=dev)]
    if second is not None:
        out += [torch.empty((P, K), dtype=torch.int32, device=dev) if second else None,
                torch.empty((P, K), dtype=torch.float32, device=dev) if second else None]
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(getattr(h.lib, entry)(h.ptr, _lib.ptr(descA), _lib.ptr(countA), _lib.ptr(descB), _lib.ptr(countB),
                                      pair_stride, count_stride, P, K, D, mode, *[_lib.ptr(o) for o in out],
                                      _lib.stream_ptr(dev)))
    return out


def match_pairs(descA, countA, descB, countB, threshold=-1.0, pair_stride=None, count_stride=1):
    """Mutual NN for P independent pairs on the GPU.
    descA/descB [P,K,D] fp32 unit rows, countA/countB [P] int32 (or strided views, see _pair_layout).
    Returns (match_idx [P,K] int32 (-1 = none), match_dist [P,K] f32, match_count [P] int32)."""
    layout = _pair_layout(descA, countA, descB, countB, pair_stride, count_stride)
    return tuple(_batched_match('mp_match_mutual_nn', layout, float(threshold)))


def nearest_pairs(descA, countA, descB, countB, ratio=None, return_second=False, pair_stride=None, count_stride=1):
    """One-directional matching for P independent pairs on the GPU (mp_match_nearest; unit rows, D in {64, 128, 256, 384}).
    `ratio=None`: every query row is matched to its nearest train row (BFMatcher.match without crossCheck);
    `ratio=r`: kept iff distance < r * second distance (knnMatch(.., 2) + Lowe's ratio test; get_matches uses 0.9).
    Returns (match_idx [P,K] int32 (-1 = none), match_dist [P,K] f32, match_count [P] int32), with `return_second`
    followed by (second_idx [P,K] int32, second_dist [P,K] f32): the second-nearest train row of every query."""
    layout = _pair_layout(descA, countA, descB, countB, pair_stride, count_stride)
    out = _batched_match('mp_match_nearest', layout, 0.0 if ratio is None else float(ratio), bool(return_second))
    return tuple(out if return_second else out[:3])


def guided_pairs(descA, countA, descB, countB, kpA, kpB, homography, radius, threshold=-1.0, pair_stride=None,
                 count_stride=1):
    """Mutual NN inside a geometric gate for P independent pairs on the GPU (mp_match_guided): optical row i and thermal
    row j are candidates for each other only if `homography[p]` maps keypoint i within `radius` pixels of keypoint j.
    descA / descB / countA / countB / pair_stride / count_stride as for match_pairs; kpA / kpB: int32 (y, x) keypoints
    laid out like the descriptors ([P,K,2], or with pair_stride contiguous views that begin at the first pair's rows --
    res.kp_yx and res.kp_yx[1:] for a PairResults); homography: [P,3,3] or [P,9] float64, optical (x, y, 1) -> thermal
    (find_homography's; an all-zero matrix yields no matches for its pair).
    Returns (match_idx [P,K] int32 (-1 = none), match_dist [P,K] f32, match_count [P] int32): a one-to-one list."""
    radius = float(radius)
    if not (radius > 0.0 and np.isfinite(radius)):
        raise ValueError('guided_pairs: radius must be finite and positive, got %r' % radius)
    descA, countA, descB, countB, P, K, D, stride, count_stride = _pair_layout(descA, countA, descB, countB, pair_stride,
                                                                              count_stride)
    if stride % D != 0:
        raise ValueError('guided_pairs: pair_stride must be a multiple of D = %d (keypoint rows are addressed like '
                         'descriptor rows)' % D)
    rows = stride // D
    for kp in (kpA, kpB):
        if kp.dtype != torch.int32 or kp.device != descA.device:
            raise ValueError('guided_pairs: keypoints must be int32 tensors on the descriptors\' device')
    if pair_stride is None:
        if tuple(kpA.shape) != (P, K, 2) or tuple(kpB.shape) != (P, K, 2):
            raise ValueError('guided_pairs: keypoints must be [P, K, 2] = [%d, %d, 2]' % (P, K))
        kpA, kpB = kpA.contiguous(), kpB.contiguous()
    else:
        for kp in (kpA, kpB):
            if not kp.is_contiguous() or kp.numel() < ((P - 1) * rows + K) * 2:
                raise ValueError('guided_pairs: keypoint views are shorter than %d pairs at this stride (or not contiguous)' % P)
    dev = descA.device
    hom = torch.as_tensor(homography, dtype=torch.float64)
    if hom.numel() != P * 9:
        raise ValueError('guided_pairs: need one 3x3 homography per pair (%d), got %d values' % (P, hom.numel()))
    hom = hom.reshape(P, 9).to(dev).contiguous()
    out = [torch.empty((P, K), dtype=torch.int32, device=dev), torch.empty((P, K), dtype=torch.float32, device=dev),
           torch.empty((P,), dtype=torch.int32, device=dev)]
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_match_guided(h.ptr, _lib.ptr(descA), _lib.ptr(countA), _lib.ptr(descB), _lib.ptr(countB), stride,
                                      count_stride, P, K, D, _lib.ptr(kpA), _lib.ptr(kpB), _lib.ptr(hom), radius,
                                      float(threshold), *[_lib.ptr(o) for o in out], _lib.stream_ptr(dev)))
    return tuple(out)


def _mutual_nn(desc_1, desc_2, threshold):
    if len(desc_1) == 0 or len(desc_2) == 0:              # matching.py:46-47
        return []
    A, nA, Bm, nB, N, M, K, D, dev = _pad_pair(desc_1, desc_2)         # (raises for differing sizes, matching.py:45)
    midx, mdist, _ = match_pairs(A, nA, Bm, nB, threshold)
    midx = midx[0, :N].cpu().numpy(); mdist = mdist[0, :N].cpu().numpy()
    q = np.nonzero(midx >= 0)[0]
    return [DMatch(i, midx[i], mdist[i]) for i in q]


class NNMatcher():
    """multipoint/utils/matching.py:35-72 (mutual nearest neighbour + distance threshold)."""

    def __init__(self, threshold=0.7):
        self.nn_thresh = threshold
        if threshold < 0.0:
            raise ValueError('\'threshold\' should be non-negative')

    def match(self, desc1, desc2):
        return _mutual_nn(desc1, desc2, float(self.nn_thresh))


def _pad_pair(desc_1, desc_2):
    d1 = torch.as_tensor(desc_1); d2 = torch.as_tensor(desc_2)
    if d1.dim() != 2 or d2.dim() != 2 or d1.shape[1] != d2.shape[1]:
        raise AssertionError('descriptor sizes differ')
    dev = d1.device if d1.device.type == 'cuda' else _lib.require_cuda(None)
    N, M, D = d1.shape[0], d2.shape[0], d1.shape[1]
    K = max(N, M, 1)
    A = torch.zeros((1, K, D), dtype=torch.float32, device=dev); A[0, :N] = d1.to(dev, torch.float32)
    Bm = torch.zeros((1, K, D), dtype=torch.float32, device=dev); Bm[0, :M] = d2.to(dev, torch.float32)
    nA = torch.tensor([N], dtype=torch.int32, device=dev); nB = torch.tensor([M], dtype=torch.int32, device=dev)
    return A, nA, Bm, nB, N, M, K, D, dev


def knn2_pairs(descA, countA, descB, countB):
    """The two nearest rows of descB for every row of descA (L2), P independent pairs on the GPU.
    Returns (nn_idx [P,K,2] int32 (-1 = none), nn_dist [P,K,2] f32)."""
    dev = descA.device
    P, K, D = descA.shape
    idx = torch.full((P, K, 2), -1, dtype=torch.int32, device=dev)
    dist = torch.zeros((P, K, 2), dtype=torch.float32, device=dev)
    h = _lib.get_handle(dev)
    with torch.cuda.device(dev):
        h.check(h.lib.mp_match_knn2(h.ptr, _lib.ptr(descA.contiguous()), _lib.ptr(countA.contiguous()),
                                    _lib.ptr(descB.contiguous()), _lib.ptr(countB.contiguous()), K * D, 1, P, K, D,
                                    _lib.ptr(idx), _lib.ptr(dist), _lib.stream_ptr(dev)))
    return idx, dist


class _BFMatcher():
    """cv2.BFMatcher(cv2.NORM_L2, crossCheck=...) as get_matches builds it (matching.py:7): `match` with crossCheck is
    the symmetric mutual nearest neighbour (the shipped configuration, mp_match_mutual_nn), without it the nearest
    train row of every query; `knnMatch(d1, d2, k <= 2)` the k nearest (mp_match_knn2)."""

    def __init__(self, crossCheck=False, **kwargs):
        if kwargs:
            raise TypeError('unsupported BFMatcher arguments: %s' % sorted(kwargs))
        self.cross_check = bool(crossCheck)

    def _knn2(self, desc1, desc2):
        if len(desc1) == 0 or len(desc2) == 0:
            return np.zeros((len(desc1), 2), np.int32) - 1, np.zeros((len(desc1), 2), np.float32)
        A, nA, Bm, nB, N, M, K, D, dev = _pad_pair(desc1, desc2)
        idx, dist = knn2_pairs(A, nA, Bm, nB)
        return idx[0, :N].cpu().numpy(), dist[0, :N].cpu().numpy()

    def match(self, desc1, desc2):
        if self.cross_check:
            return _mutual_nn(desc1, desc2, -1.0)
        idx, dist = self._knn2(desc1, desc2)
        return [DMatch(i, idx[i, 0], dist[i, 0]) for i in range(len(idx)) if idx[i, 0] >= 0]

    def knnMatch(self, desc1, desc2, k):
        if self.cross_check and k != 1:
            raise ValueError('BFMatcher: crossCheck=True supports knnMatch with k=1 only (as OpenCV)')
        if k not in (1, 2):
            raise NotImplementedError('knnMatch is implemented for k <= 2 (get_matches uses k = 2)')
        if self.cross_check:
            return [[m] for m in self.match(desc1, desc2)]
        idx, dist = self._knn2(desc1, desc2)
        return [[DMatch(i, idx[i, c], dist[i, c]) for c in range(k) if idx[i, c] >= 0] for i in range(len(idx))]


class ThresholdMatcher():
    """multipoint/utils/matching.py:74-99: every (i, j) closer than the threshold, in row-major order."""

    def __init__(self, threshold=0.4):
        self.threshold = threshold
        if threshold < 0.0:
            raise ValueError('\'threshold\' should be non-negative')

    def match(self, desc1, desc2):
        if len(desc1) == 0 or len(desc2) == 0:        # matching.py:86-87
            return []
        A, nA, Bm, nB, N, M, K, D, dev = _pad_pair(desc1, desc2)
        h = _lib.get_handle(dev)
        cap = max(4 * K, 1024)
        while True:
            ij = torch.empty((1, cap, 2), dtype=torch.int32, device=dev)
            dd = torch.empty((1, cap), dtype=torch.float32, device=dev)
            cnt = torch.empty((1,), dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                h.check(h.lib.mp_match_threshold(h.ptr, _lib.ptr(A), _lib.ptr(nA), _lib.ptr(Bm), _lib.ptr(nB), K * D, 1,
                                                 1, K, D, float(self.threshold), cap, _lib.ptr(ij), _lib.ptr(dd),
                                                 _lib.ptr(cnt), _lib.stream_ptr(dev)))
            n = int(cnt.item())
            if n <= cap:
                break
            cap = n                                   # the list overflowed: one retry with the exact size
        ij = ij[0, :n].cpu().numpy(); dd = dd[0, :n].cpu().numpy()
        order = np.lexsort((ij[:, 1], ij[:, 0]))      # np.argwhere order (:92)
        return [DMatch(ij[o, 0], ij[o, 1], dd[o]) for o in order]


def get_matches(desc_1, desc_2, method='bfmatcher', knn_matches=False, **kwargs):
    """multipoint/utils/matching.py:4-33.  desc_1 (N,D), desc_2 (M,D): numpy arrays or tensors.
    Returns a list of DMatch ordered by queryIdx."""
    if method == 'bfmatcher':
        matcher = _BFMatcher(**kwargs)
    elif method == 'nnmatcher':
        matcher = NNMatcher(**kwargs)
    elif method == 'thresholdmatcher':
        matcher = ThresholdMatcher(**kwargs)
    elif method == 'flann':
        raise NotImplementedError("matching method 'flann' (cv2.FlannBasedMatcher: an approximate randomised kd-tree "
                                  "index) has no exact GPU counterpart; use 'bfmatcher', which returns the exact "
                                  "neighbours flann approximates")
    else:
        raise ValueError('unknown matching method')
    if knn_matches:
        all_matches = matcher.knnMatch(desc_1, desc_2, 2)       # AttributeError for nnmatcher / thresholdmatcher, as in the reference
        ratio_thresh = 0.9                                      # Lowe's ratio test (:22-27)
        matches = []
        for m, n in all_matches:
            if m.distance < ratio_thresh * n.distance:
                matches.append(m)
        return matches
    return matcher.match(desc_1, desc_2)
