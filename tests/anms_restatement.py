"""Adaptive non-maximal suppression restated in plain numpy (include/multipoint_hip.h: mp_detect_keypoints_spread): the
dominance test with ONE fp32 multiply, integer squared distances, and the three-key order.  Shared by the host and GPU tests;
not a test module itself."""
import numpy as np

NONE = 0xFFFFFFFF


def radii(y, x, s, robust=1.0):
    """R [n] uint32 of the candidates (y_i, x_i, s_i): min over { j : s_i < fl(c * s_j) } of the squared distance, NONE without
    a dominator."""
    y, x = np.asarray(y, np.int64).reshape(-1), np.asarray(x, np.int64).reshape(-1)
    s = np.asarray(s, np.float32).reshape(-1)
    n = len(s)
    if n == 0:
        return np.zeros(0, np.uint32)
    cs = np.float32(robust) * s                                  # float32 * float32 array: one fp32 multiply each
    assert cs.dtype == np.float32
    dominated = s[:, None] < cs[None, :]                         # [i, j]: j dominates i
    d2 = (y[:, None] - y[None, :]) ** 2 + (x[:, None] - x[None, :]) ** 2
    return np.where(dominated, d2, NONE).min(axis=1).astype(np.uint32)


def select(y, x, s, k, robust=1.0):
    """(kept, R): the indices of the min(k, n) candidates first by (R descending, score bits descending, index ascending), listed
    in ascending (row-major) order, and every candidate's R.  The candidates are given in row-major order."""
    s = np.asarray(s, np.float32).reshape(-1)
    R = radii(y, x, s, robust)
    n = len(s)
    bits = s.view(np.uint32).astype(np.int64)                    # scores are positive: their bits order like the floats
    order = np.lexsort((np.arange(n), -bits, -R.astype(np.int64)))          # (the last key is the primary one)
    return np.sort(order[:min(int(k), n)]), R


def select_map(nms_map, k, robust=1.0):
    """select() on the survivors of a dense NMS output (zeros except the kept pixels).  Returns (kp [m, 2], score [m], R [m],
    dense map with the kept scores)."""
    nms_map = np.asarray(nms_map, np.float32)
    yx = np.argwhere(nms_map > 0)                                # row-major
    s = nms_map[yx[:, 0], yx[:, 1]]
    kept, R = select(yx[:, 0], yx[:, 1], s, k, robust)
    dense = np.zeros_like(nms_map)
    dense[yx[kept, 0], yx[kept, 1]] = s[kept]
    return yx[kept], s[kept], R[kept], dense


def planted_map(seed):
    """96 x 128: a dense block of strong peaks in the top-left quarter and sparse weak peaks over the whole frame; the order of
    the draws fixes the numbers."""
    rng = np.random.default_rng(seed)
    m = np.zeros((96, 128), np.float32)
    for y in range(2, 48, 4):
        for x in range(2, 64, 4):
            m[y, x] = 0.5 + 0.4 * rng.random()
    for y in range(2, 96, 8):
        for x in range(2, 128, 8):
            if m[y, x] == 0 and rng.random() < 0.6:
                m[y, x] = 0.05 + 0.25 * rng.random()
    return m


def occupied_cells(kp, H=96, W=128, grid=4):
    """number of cells of a grid x grid partition of the frame that hold a keypoint"""
    kp = np.asarray(kp).reshape(-1, 2)
    return len({(int(y) // (H // grid), int(x) // (W // grid)) for y, x in kp})
