"""Shared generators of the pooled-homography tests (tests/test_pooled_host.py, tests/test_gpu_pooled_homography.py,
tests/test_gpu_initial_transform_cli.py): planted pairs (the `_planted` idea of tests/test_gpu_metrics.py: thermal = H(optical)
plus sub-pixel noise, rounded, a share of the matches replaced by random points), planted point sets, and a numpy restatement
of the pooling.  Everything here is host code."""
import numpy as np


def random_homography(rng, shift=8.0):
    hm = np.eye(3)
    hm[:2, :2] += rng.normal(0, 0.03, (2, 2)); hm[:2, 2] += rng.normal(0, shift, 2); hm[2, :2] += rng.normal(0, 5e-5, 2)
    return hm


def apply_h(hm, xy):
    xy1 = np.concatenate([np.asarray(xy, np.float64), np.ones((len(xy), 1))], 1) @ np.asarray(hm, np.float64).reshape(3, 3).T
    return xy1[:, :2] / xy1[:, 2:3]


def corner_error(h_est, h_true, H, W):
    c = np.array([[0, 0], [W, 0], [0, H], [W, H]], np.float64)
    return np.linalg.norm(apply_h(h_est, c) - apply_h(h_true, c), axis=1).max()


def planted_points(rng, n, H, W, outlier_frac, hm=None, noise=0.3, integer=True):
    """n correspondences (optical xy, thermal xy, outlier flags) under the planted model `hm` (default: a random one)."""
    hm = random_homography(rng) if hm is None else hm
    if integer:
        a = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1).astype(np.float64)
    else:
        a = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1)
    b = apply_h(hm, a) + rng.normal(0, noise, (n, 2))
    bad = rng.random(n) < outlier_frac
    if integer:
        b = np.round(b)
        b[bad] = np.stack([rng.integers(0, W, bad.sum()), rng.integers(0, H, bad.sum())], 1)
    else:
        b[bad] = np.stack([rng.uniform(0, W, bad.sum()), rng.uniform(0, H, bad.sum())], 1)
    return a, b, bad, hm


def planted_pairs(rng, P, K, H, W, outlier_frac, sizes=None, shared=None, matched_frac=0.9):
    """Interleaved keypoint lists of P pairs with a planted homography per pair (`shared`: one for all of them).  sizes[p]
    keypoints in pair p (default: K and 0.6 K in turn), the thermal list in another order, `matched_frac` of them matched.
    Returns kp [2P,K,2] (y, x), cnt [2P], midx [P,K], planted [(hm, bad flags per optical keypoint)]."""
    kp = np.zeros((2 * P, K, 2), np.int32); cnt = np.zeros(2 * P, np.int32); midx = -np.ones((P, K), np.int32)
    planted = []
    for p in range(P):
        n = (K if p % 2 == 0 else int(K * 0.6)) if sizes is None else int(sizes[p])
        a, b, bad, hm = planted_points(rng, n, H, W, outlier_frac, hm=shared)
        perm = rng.permutation(n)
        kp[2 * p, :n] = a[:, ::-1]; kp[2 * p + 1, perm] = b[:, ::-1]
        cnt[2 * p] = cnt[2 * p + 1] = n
        matched = rng.random(n) < matched_frac
        midx[p, :n][matched] = perm[matched]
        planted.append((hm, bad))
    return kp, cnt, midx, planted


def to_results(kp, cnt, midx, H, W, device='cuda'):
    import torch
    from multipoint_amd.pipeline import PairResults
    P, K = midx.shape
    return PairResults(torch.from_numpy(np.ascontiguousarray(kp)).to(device), None, torch.from_numpy(np.ascontiguousarray(cnt)).to(device),
                       None, torch.from_numpy(np.ascontiguousarray(midx)).to(device), torch.zeros((P, K), device=device), None, H, W)


def pool_host(kp, cnt, midx, groups=None):
    """numpy restatement of pool_matches: (pts [N,4] float32, query_index [N], pair_offsets [P+1], group_offsets [G+1])."""
    P, K = midx.shape
    pts, qidx, po = [], [], [0]
    for p in range(P):
        no, nt = min(int(cnt[2 * p]), K), min(int(cnt[2 * p + 1]), K)
        for i in range(max(no, 0)):
            j = int(midx[p, i])
            if 0 <= j < nt:
                pts.append([kp[2 * p, i, 1], kp[2 * p, i, 0], kp[2 * p + 1, j, 1], kp[2 * p + 1, j, 0]]); qidx.append(i)
        po.append(len(pts))
    po = np.array(po, np.int32)
    if groups is None:
        go = np.array([0, po[-1]], np.int32)
    else:
        g = np.asarray(groups)
        G = int(g.max()) + 1
        go = np.array([po[np.searchsorted(g, k, side='left')] if np.searchsorted(g, k, side='left') < P else po[-1]
                       for k in range(G + 1)], np.int32)
    return np.array(pts, np.float32).reshape(-1, 4), np.array(qidx, np.int32), po, go


def scatter_mask(mask, query_index, pair_offsets, P, K):
    """The pooled mask [N] as the per-pair layout [P,K] (one byte per optical keypoint)."""
    out = np.zeros((P, K), np.uint8)
    for p in range(P):
        s, e = int(pair_offsets[p]), int(pair_offsets[p + 1])
        out[p, query_index[s:e]] = mask[s:e]
    return out


def dlt_gap(a, b, inl):
    """How well the normalised-DLT refit over the inliers `inl` is conditioned: the second-smallest eigenvalue of A^T A over the
    largest.  The device solves the eigenproblem by Jacobi sweeps and the oracle by LAPACK; their eigenvectors agree to about
    2^-52 / gap, so a gap above 1e-6 keeps that three orders of magnitude below the 1e-6 bound the tests hold H to."""
    pa, pb = np.asarray(a, np.float64)[inl], np.asarray(b, np.float64)[inl]
    ca, cb = pa.mean(0), pb.mean(0)
    sa = np.sqrt(2.0) / max(np.sqrt(((pa - ca) ** 2).sum(1)).mean(), 1e-12)
    sb = np.sqrt(2.0) / max(np.sqrt(((pb - cb) ** 2).sum(1)).mean(), 1e-12)
    x, y = ((pa - ca) * sa).T; u, v = ((pb - cb) * sb).T
    o, z = np.ones_like(x), np.zeros_like(x)
    A = np.concatenate([np.stack([x, y, o, z, z, z, -u * x, -u * y, -u], 1), np.stack([z, z, z, x, y, o, -v * x, -v * y, -v], 1)])
    w = np.linalg.eigvalsh(A.T @ A)
    return w[1] / w[-1]


def _errors2(h, a, b):
    """Squared forward reprojection errors with the oracle's own expressions (inf where it refuses w = 0)."""
    h = np.asarray(h, np.float64).reshape(9)
    w = h[6] * a[:, 0] + h[7] * a[:, 1] + h[8]
    ok = np.abs(w) >= 1e-12
    iw = 1.0 / np.where(ok, w, 1.0)
    du = (h[0] * a[:, 0] + h[1] * a[:, 1] + h[2]) * iw - b[:, 0]
    dv = (h[3] * a[:, 0] + h[4] * a[:, 1] + h[5]) * iw - b[:, 1]
    return np.where(ok, du * du + dv * dv, np.inf)


def threshold_margin(h4, a, b, thr):
    """|reprojection error - thr| in pixels of every correspondence under the 3x3 model h4 (float32 inputs, fp64 arithmetic)."""
    a = np.asarray(a, np.float32).astype(np.float64); b = np.asarray(b, np.float32).astype(np.float64)
    return np.abs(np.sqrt(_errors2(h4, a, b)) - thr)


def winning_model(oracle, a, b, thr, T, seed, g):
    """The 4-point model of the oracle's winning hypothesis, from the oracle alone: oracle.ransac_homography returns the
    winner's consensus set but not its model, so the hypotheses are drawn again with the oracle's sampling (its _mix64) and
    the first one whose inlier set is the returned mask is the winner (most inliers, lowest index).  Returns a 3x3 matrix."""
    a32 = np.asarray(a, np.float32).astype(np.float64); b32 = np.asarray(b, np.float32).astype(np.float64)
    n = len(a32)
    _, mask = oracle.ransac_homography(a, b, thr, T, seed, g)
    for t in range(T):
        ctr = oracle._mix64((seed ^ (g << 32) ^ t) & oracle._M64)
        idx = []
        while len(idx) < 4:
            ctr = oracle._mix64(ctr); c = ctr % n
            if c not in idx:
                idx.append(c)
        m = np.zeros((8, 8)); r = np.zeros(8)
        for k, i in enumerate(idx):
            x, y = a32[i]; u, v = b32[i]
            m[2 * k] = [x, y, 1, 0, 0, 0, -u * x, -u * y]; r[2 * k] = u
            m[2 * k + 1] = [0, 0, 0, x, y, 1, -v * x, -v * y]; r[2 * k + 1] = v
        if abs(np.linalg.det(m)) < 1e-300 or np.linalg.cond(m) > 1e13:
            continue
        h = np.append(np.linalg.solve(m, r), 1.0)
        if np.array_equal(_errors2(h, a32, b32) <= float(thr) ** 2, mask):
            return h.reshape(3, 3)
    raise AssertionError('no hypothesis reproduces the oracle mask')


def well_posed(oracle, a, b, thr, T, seed, g=0, min_inliers=8):
    """What the (N, T) cases ask of their data, decided with the oracle alone: a model exists, its consensus set has at least
    min(N, min_inliers) members and its refit is conditioned as dlt_gap describes."""
    Ho, mo = oracle.ransac_homography(a, b, thr, T, seed, g)
    return Ho is not None and mo.sum() >= min(len(a), min_inliers) and dlt_gap(np.asarray(a, np.float32), np.asarray(b, np.float32), mo) >= 1e-6
