"""Not GPU: the premises of the RIFT cases (tests/rift_cases.py), checked with the numpy restatement (tests/rift_restatement.py)
alone -- what tests/test_gpu_rift.py and tests/test_gpu_rift_e2e.py take for granted about their inputs."""
import numpy as np
import pytest

import lghd_restatement as L
import rift_cases as C
import rift_restatement as R


@pytest.mark.parametrize('name', [im[0] for im in C.MAP_FRAMES])
def test_ambiguous_share_is_small(name):
    """rule 3: at most 1 % of a frame's pixels have a float64 top-two gap of sumA below 16 float32 errors, and the float32 run
    agrees with the float64 arg-max at every other pixel"""
    f64, f32 = C.restated_maps(name)
    amb = C.ambiguous(name)
    print(name, 'ambiguous %.4f %%' % (100 * amb.mean()))
    assert amb.mean() <= C.AMBIGUOUS_CAP
    assert np.array_equal(f64['mim'][~amb], f32['mim'][~amb])
    # the error scale of the 8x rules is not degenerate
    assert 0 < np.abs(f32['M'] - f64['M']).max() < 1e-5 * max(np.ptp(f64['M']), 1e-3)


def test_even_and_odd_pixel_counts_are_covered():
    counts = [im[3] * im[4] for im in C.MAP_FRAMES]
    assert any(n % 2 for n in counts) and any(n % 2 == 0 for n in counts)
    # the median of an even count is the mean of two DIFFERENT elements on at least one frame: the upper middle one is looked for
    differs = []
    for name, _, _, H, W in C.MAP_FRAMES:
        if (H * W) % 2 == 0:
            v = np.sort(C.restated_maps(name)[1]['amp0'][0].astype(np.float32).ravel())
            differs.append(v[H * W // 2 - 1] != v[H * W // 2])
    assert any(differs)


def test_noise_threshold_formula():
    assert R.noise_threshold(np.zeros((4, 6), np.float32)) == 0.0
    # median 2.5 of 1 .. 4: tau = 2.5 / sqrt(ln 4), tot = tau (1 - 1.6^-4) / (1 - 1 / 1.6), T = tot (sqrt(pi / 2) + sqrt((4 - pi) / 2))
    want = 2.5 / np.sqrt(np.log(4)) * (1 - 1.6 ** -4) / (1 - 1 / 1.6) * (np.sqrt(np.pi / 2) + np.sqrt((4 - np.pi) / 2))
    assert abs(R.noise_threshold(np.array([4, 1, 3, 2], np.float32)) - want) <= 1e-12
    assert abs(R.noise_threshold(np.array([4, 1, 3], np.float32), k=0.0) - 3 / 2.5 * want * np.sqrt(np.pi / 2) /
               (np.sqrt(np.pi / 2) + np.sqrt((4 - np.pi) / 2))) <= 1e-12


@pytest.mark.parametrize('name,patch', [('smooth_48x80', 24), ('noise_64x64', 24), ('smooth_64x64', 48), ('noise_45x75', 24),
                                        ('smooth_96x128', 48), ('smooth_96x128', 96), ('smooth_160x192', 96)])
def test_frames_hold_keypoints(name, patch):
    """at least one valid keypoint at both thresholds, so that detect and describe have something to be compared on"""
    M = C.restated_maps(name)[0]['M'].astype(np.float32)
    for thr in (6, 13):
        assert (R.detect(M, thr, patch)[3] > 0).sum() >= 1


def test_constant_frames_in_exact_arithmetic():
    """every PC is 0 on a constant frame: M = eps / 2, m = -eps / 2 (step 5 with cx2 = cy2 = cxy = 0 and d = eps), MIM = 0, T = 0"""
    for name, _, _, _ in C.CONSTANT_FRAMES:
        pc = R.phase_congruency(C.constant_frame(name))
        assert np.abs(pc['M'] - R.EPS / 2).max() <= 1e-12 and np.abs(pc['m'] + R.EPS / 2).max() <= 1e-12
    pc = R.phase_congruency(C.constant_frame('zero_48x80'), single=True)
    assert np.all(pc['M'] == np.float32(R.EPS) / 2) and np.all(pc['m'] == -np.float32(R.EPS) / 2) and not pc['mim'].any()
    assert not pc['T'].any()


def test_contrast_inversion_leaves_the_float64_maps_alone():
    u8 = C.map_frame('smooth_96x128')
    a, b = C.restated_maps('smooth_96x128')[0], R.phase_congruency(255 - u8)
    for key in ('M', 'm', 'sumA', 'T'):
        assert np.abs(a[key] - b[key]).max() <= 1e-9 * max(1.0, np.abs(a[key]).max()), key
    amb = C.ambiguous('smooth_96x128')
    assert np.array_equal(a['mim'][~amb], b['mim'][~amb])


@pytest.mark.parametrize('i', range(3))
def test_planted_pairs(i):
    """the restatement's own chain on a planted pair: the stored counts are what it gets, and a float64 least-squares similarity
    through its correct matches is within 0.5 px of the planted map at the frame corners"""
    (ko, do), (kt, dt) = C.restated_pair(i)
    q, t = R.mutual_nn(do, dt)
    good = C.planted_error(i, ko[q], kt[t]) <= 3.0
    print('pair %d: %d / %d keypoints, %d mutual, %d within 3 px' % (i, len(ko), len(kt), len(q), good.sum()))
    assert (len(q), int(good.sum())) == (C.RESTATED_MUTUAL[i], C.RESTATED_CORRECT[i])
    assert good.sum() >= 60
    A = R.fit_similarity(ko[q][good][:, ::-1], kt[t][good][:, ::-1])
    err = C.corner_error(i, A)
    print('corner error %.3f px' % err)
    assert err < 0.5


def test_descriptor_layout():
    """[cell row][cell col][bin]: a map that is 5 in one cell and 0 elsewhere"""
    mim = np.zeros((48, 48), np.uint8)
    mim[16:24, 32:40] = 5                   # patch 48 at (24, 24): cells of 8, this is cell (2, 4)
    d = R.descriptors(mim, [(24, 24)], 48).reshape(6, 6, 6)
    assert d[2, 4, 5] == 64 and d[2, 4, 0] == 0 and d.sum() == 48 * 48 and d[..., 0].sum() == 48 * 48 - 64
