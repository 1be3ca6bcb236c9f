"""numpy restatement of the RIFT baseline as DESIGN.md 3.26 specifies it (Li, Hu, Ai, IEEE TIP 2020, restated from the paper; NOT
verified against the authors' MATLAB code), the model the HIP kernels of multipoint_amd/csrc/fft.hip, rift.hip and lghd.hip are
tested against:

  phase_congruency      M, m, the maximum index map, the noise thresholds and the sums they come from, in float64 (np.fft) or,
                        single=True, in complex64 / float32 throughout: the float32 error scale of the tolerances
  noise_threshold       T from the exact median of one scale-0 amplitude plane, in float64
  moment_u8             the 8-bit image of M that FAST runs on, float32 arithmetic in the specified order
  detect                FAST-9/16 on it (lghd_restatement's, with the threshold as an argument), the patch border, prob
  descriptors           6 x 6 cells x 6 bins of the maximum index map, [cell row][cell col][bin]
  mutual_nn             float64 brute-force mutual nearest neighbours
  fit_similarity        float64 least-squares similarity of point pairs

FAST, the filter bank and the test images are lghd_restatement's."""
import math

import numpy as np

import lghd_restatement as L

EPS = 1e-4
N_SCALES, N_ANGLES = L.N_SCALES, L.N_ANGLES
MULT = 1.6
DESCRIPTOR_SIZE, WIDTH = 216, 256


def noise_threshold(plane, k=1.0):
    """float64 T of one amplitude plane A[0][o]: its exact median (the mean of the two middle order statistics for an even
    count), tau = median / sqrt(ln 4), tot = tau (1 - q^4) / (1 - q) with q = 1 / 1.6 and q^4 = ((q q) q) q,
    T = tot sqrt(pi / 2) + (k tot) sqrt((4 - pi) / 2); every operation a float64 operation of its own."""
    v = np.sort(np.asarray(plane).ravel()).astype(np.float64)
    n = v.size
    median = float((v[(n - 1) // 2] + v[n // 2]) * 0.5)
    q = 1.0 / 1.6
    tau = median / math.sqrt(math.log(4.0))
    tot = tau * (1.0 - q * q * q * q) / (1.0 - q)
    return tot * math.sqrt(math.pi / 2.0) + (float(k) * tot) * math.sqrt((4.0 - math.pi) / 2.0)


def phase_congruency(u8, bank=None, k=1.0, g=3.0, cutoff=0.5, single=False):
    """dict of M, m [H][W], mim uint8 [H][W], T [6], sumA [6][H][W], amp0 [6][H][W] (= A[0][o]); float64 arrays whichever the
    precision of the run."""
    img = np.asarray(u8)
    H, W = img.shape
    bank = L.filter_bank(H, W) if bank is None else bank
    f = np.float32 if single else np.float64
    if single:
        spec = np.fft.fft2(img.astype(np.complex64))
        R = np.fft.ifft2(spec[None] * np.asarray(bank, np.float32))         # (np.fft.ifft2 divides by H W)
        assert R.dtype == np.complex64, 'numpy >= 2 is needed for a float32 FFT'
    else:
        spec = np.fft.fft2(img.astype(np.float64))
        R = np.fft.ifft2(spec[None] * np.asarray(bank, np.float64))
    R = R.reshape(N_SCALES, N_ANGLES, H, W)
    E, O = R.real.astype(f), R.imag.astype(f)
    A = np.sqrt(E * E + O * O)
    eps = f(EPS)
    cx2, cy2, cxy = np.zeros((H, W), f), np.zeros((H, W), f), np.zeros((H, W), f)
    T = np.zeros(N_ANGLES, f)
    sumA_all = np.zeros((N_ANGLES, H, W), f)
    for o in range(N_ANGLES):
        sumE, sumO, sumA, maxA = E[0, o].copy(), O[0, o].copy(), A[0, o].copy(), A[0, o].copy()
        for s in range(1, N_SCALES):
            sumE = sumE + E[s, o]; sumO = sumO + O[s, o]; sumA = sumA + A[s, o]; maxA = np.maximum(maxA, A[s, o])
        X = np.sqrt(sumE * sumE + sumO * sumO) + eps
        mE, mO = sumE / X, sumO / X
        En = np.zeros((H, W), f)
        for s in range(N_SCALES):
            En = En + (E[s, o] * mE + O[s, o] * mO - np.abs(E[s, o] * mO - O[s, o] * mE))
        T[o] = f(noise_threshold(A[0, o], k))
        En = np.maximum(En - T[o], f(0))
        width = (sumA / (maxA + eps) - f(1)) / f(3)
        weight = f(1) / (f(1) + np.exp((f(cutoff) - width) * f(g)))
        pc = weight * En / (sumA + eps)
        cx, cy = pc * f(math.cos(o * math.pi / 6)), pc * f(math.sin(o * math.pi / 6))
        cx2 = cx2 + cx * cx; cy2 = cy2 + cy * cy; cxy = cxy + cx * cy
        sumA_all[o] = sumA
    cx2, cy2, cxy = cx2 / f(3), cy2 / f(3), cxy * (f(4) / f(6))
    d = np.sqrt(cxy * cxy + (cx2 - cy2) * (cx2 - cy2)) + eps
    out = {'M': (cy2 + cx2 + d) / f(2), 'm': (cy2 + cx2 - d) / f(2), 'T': T, 'sumA': sumA_all, 'amp0': A[0]}
    assert all(v.dtype == f for v in out.values())
    out = {key: v.astype(np.float64) for key, v in out.items()}
    out['mim'] = np.argmax(sumA_all, axis=0).astype(np.uint8)           # the first maximum
    return out


def top_two_gap(sumA):
    """float64 [H][W]: largest minus second-largest summed amplitude among the 6 orientations"""
    s = np.sort(np.asarray(sumA, np.float64), axis=0)
    return s[-1] - s[-2]


def moment_u8(M):
    """(uint8) floor(255 ((M - min) / (max - min))) in float32, each operation rounded on its own; zeros when max == min"""
    M = np.asarray(M, np.float32)
    mn, mx = M.min(), M.max()
    span = np.float32(mx - mn)
    if not span > 0:
        return np.zeros(M.shape, np.uint8)
    return (np.float32(255.0) * ((M - mn) / span)).astype(np.uint8)


def fast_scores(u8, threshold):
    """lghd_restatement.fast_scores with `threshold` in place of its module constant"""
    keep = L.THRESHOLD
    L.THRESHOLD = int(threshold)
    try:
        return L.fast_scores(u8)
    finally:
        L.THRESHOLD = keep


def detect(M, fast_threshold=13, patch_size=96):
    """-> (u8m, score int32 [H][W], corners bool [H][W], prob float32 [H][W]): prob = score / 255 at corners with
    b <= y <= H - b and b <= x <= W - b, b = patch_size / 2"""
    u8m = moment_u8(M)
    H, W = u8m.shape
    score = fast_scores(u8m, fast_threshold)
    corners = L.fast_corners(score)
    b = patch_size // 2
    yy, xx = np.mgrid[0:H, 0:W]
    valid = corners & (yy >= b) & (yy <= H - b) & (xx >= b) & (xx <= W - b)
    prob = np.where(valid, score.astype(np.float32) / np.float32(255.0), np.float32(0)).astype(np.float32)
    return u8m, score, corners, prob


def keypoints(prob):
    return np.argwhere(prob > 0)                # row-major (y, x)


def descriptors(mim, kp, patch_size=96):
    """mim uint8 [H][W], kp (y, x) rows whose patches lie inside the frame -> float64 [n][216] counts"""
    kp = np.asarray(kp).reshape(-1, 2)
    b, c = patch_size // 2, patch_size // 6
    out = np.zeros((len(kp), 6, 6, N_ANGLES))
    for i, (y, x) in enumerate(kp):
        patch = mim[y - b:y + b, x - b:x + b]
        for j in range(6):
            for l in range(6):
                out[i, j, l] = np.bincount(patch[j * c:(j + 1) * c, l * c:(l + 1) * c].ravel(), minlength=N_ANGLES)[:N_ANGLES]
    return out.reshape(len(kp), DESCRIPTOR_SIZE)


def mutual_nn(a, b):
    """unit rows a [n][D], b [m][D] -> (query, train) index arrays of the mutual nearest neighbours (first minimum)"""
    if len(a) == 0 or len(b) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    d = 2.0 - 2.0 * (np.asarray(a, np.float64) @ np.asarray(b, np.float64).T)
    best, back = d.argmin(1), d.argmin(0)
    q = np.nonzero(back[best] == np.arange(len(a)))[0]
    return q, best[q]


def fit_similarity(src, dst):
    """least-squares x' = a x - b y + tx, y' = b x + a y + ty from (x, y) rows, as a 3 x 3 matrix, in float64"""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    n = len(src)
    A = np.zeros((2 * n, 4))
    A[0::2] = np.stack([src[:, 0], -src[:, 1], np.ones(n), np.zeros(n)], 1)
    A[1::2] = np.stack([src[:, 1], src[:, 0], np.zeros(n), np.ones(n)], 1)
    a, b, tx, ty = np.linalg.lstsq(A, dst.reshape(-1), rcond=None)[0]
    return np.array([[a, -b, tx], [b, a, ty], [0, 0, 1.0]])


def restated_side(image, fast_threshold, patch_size):
    """(keypoints (y, x), unit descriptor rows float64 [n][216], the float64 maps) of one float32 image in [0, 1]"""
    pc = phase_congruency(L.quantize(image))
    _, _, _, prob = detect(pc['M'].astype(np.float32), fast_threshold, patch_size)
    kp = keypoints(prob)
    return kp, L.unit_rows(descriptors(pc['mim'], kp, patch_size)), pc
