"""The planted pair of the motion-model tests: a thermal frame that is a non-monotone map of the optical
frame under a known SIMILARITY, and a start 3.5 px off in mean four-corner error.  Pure numpy, over tests/mi_restatement.py."""
import numpy as np

import mi_restatement as R

H, W = 96, 128
P_TRUE = np.array([np.radians(1.5), 0.95, 6.0, 5.0])
P_INIT = P_TRUE + np.array([np.radians(0.6), 0.012, 1.8, -1.5])


def similarity_matrix(p):
    """(angle, scale, dx, dy) -> [[s cos a, s sin a, dx], [-s sin a, s cos a, dy], [0, 0, 1]] in float64"""
    a, s, dx, dy = (float(v) for v in p)
    return np.array([[s * np.cos(a), s * np.sin(a), dx], [-(s * np.sin(a)), s * np.cos(a), dy], [0.0, 0.0, 1.0]])


def model_matrix(p, model):
    """numpy float64 statement of the parameter map of the three models"""
    p = np.asarray(p, np.float64)
    if model == 'similarity':
        return similarity_matrix(p)
    if model == 'affine':
        return np.concatenate([p, [0.0, 0.0, 1.0]]).reshape(3, 3)
    assert model == 'homography'
    return p.reshape(3, 3).copy()


_CASE = []


def recovery_case():
    """optical (112, 144), thermal (96, 128) fp32, T_true, T_init; built once and shared (do not write into the arrays)"""
    if not _CASE:
        optical = R.blob_image(11, 112, 144, 300, 1.2, 4.0)
        T_true = similarity_matrix(P_TRUE)
        w = R.warp_image(optical, T_true, H, W)
        assert w.min() >= 0
        thermal = (4.0 * (w.astype(np.float64) - 0.45) ** 2).astype(np.float32)
        _CASE.append((optical, thermal, T_true, similarity_matrix(P_INIT)))
    return _CASE[0]


def error(T):
    """mean four-corner error against T_true on the 96 x 128 frame"""
    return R.corner_error(T, recovery_case()[2], H, W)
