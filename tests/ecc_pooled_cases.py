"""Cases of the pooled ECC tests: the six-pair planted recording of registration_cases.cli_pairs() as 8- and
16-bit files hold it, the same recording with one mis-paired frame, with static artefacts (a black margin and a burnt-in
overlay in both cameras), the four-pair group and the three groups with three planted shifts.  Frames are float32 (/ 255 and
/ 65535); a transform maps thermal pixels to optical ones; errors are corner errors in thermal pixels (ecc_cases.cli_error)."""
import functools

import numpy as np

import ecc_cases as C
import ecc_pooled_restatement as PR
import ecc_restatement as E
import registration_cases as RC

KSIZE = 5
FIXTURE_EPS = 1e-8
THERMAL_HW = RC.GROUP['thermal_hw']
# host caps (px) of the pooled result on the clean recording and with the grown static masks on the artefact recording
CLEAN_CAP = {'similarity': 0.25, 'affine': 0.3, 'homography': 0.5}
MASKED_CAP = {'similarity': 0.25, 'affine': 0.3, 'homography': 0.8}
SAME_POINT = 0.05
REJECTED_CAP = 0.3                                             # homography after the rejection round
MISPAIRED = 2


def to_float(optical_u8, thermal_u16):
    return (optical_u8.astype(np.float32) / np.float32(255.0)), (thermal_u16.astype(np.float32) / np.float32(65535.0))


@functools.lru_cache(maxsize=None)
def raw(kind='clean'):
    """(optical uint8 [6][96][128], thermal uint16 [6][72][96]) of a recording: 'clean', 'mispaired' or 'artefact'."""
    optical, thermal, _ = RC.cli_pairs()
    optical, thermal = optical.copy(), thermal.copy()
    if kind == 'mispaired':
        other = RC.make_pair(181, (72, 96), -6.0, 0.9, (8.0, -7.0))[1]
        thermal[MISPAIRED] = np.rint(other.astype(np.float64) * 65535.0).astype(np.uint16)
    elif kind == 'artefact':
        o, t = planted_masks()
        optical[:, o == 0] = 0
        optical[:, 70:78, 30:60] = 255
        thermal[:, t == 0] = 0
        thermal[:, 50:56, 20:44] = 65535
    else:
        assert kind == 'clean'
    return optical, thermal


@functools.lru_cache(maxsize=None)
def planted_masks():
    """(optical use-mask [96][128], thermal use-mask [72][96]) of the artefact recording: margins of 6 and 5 px and the overlays."""
    o = np.zeros(RC.OPTICAL_HW, np.uint8)
    o[6:-6, 6:-6] = 1
    o[70:78, 30:60] = 0
    t = np.zeros(THERMAL_HW, np.uint8)
    t[5:-5, 5:-5] = 1
    t[50:56, 20:44] = 0
    return o, t


@functools.lru_cache(maxsize=None)
def recording(kind='clean'):
    """(optical float32 [6][96][128], thermal float32 [6][72][96])"""
    return to_float(*raw(kind))


@functools.lru_cache(maxsize=None)
def start(target):
    """The shared start, `target` px off the planted transform."""
    return C.cli_start(float(target))


error = C.cli_error


@functools.lru_cache(maxsize=None)
def features(kind='clean', f32=False, feature='gradient'):
    """(planes [P] of (f, gx, gy), templates [P]) of a recording under the restatement."""
    optical, thermal = recording(kind)
    planes = [E.image_planes(E.features(o, KSIZE, feature, f32), f32) for o in optical]
    templates = [E.features(t, KSIZE, feature, f32) for t in thermal]
    return planes, templates


@functools.lru_cache(maxsize=None)
def grown_masks(feature='gradient'):
    """(thermal, optical) planted use-masks grown by the feature's support."""
    rt, ro = PR.mask_radii(feature, KSIZE)
    o, t = planted_masks()
    return PR.grow(t, rt), PR.grow(o, ro)


@functools.lru_cache(maxsize=None)
def restated(kind, target, model, masked=False, eps=FIXTURE_EPS, maxiter=50, f32=False, reject_ratio=0.0):
    planes, templates = features(kind, f32)
    tkeep, okeep = grown_masks() if masked else (None, None)
    return PR.estimate(planes, templates, start(target), model, eps, maxiter, 0.25, f32, tkeep, okeep, None, reject_ratio)


def noise_floor(kind, target, model, maxiter, masked=False):
    """The corner distance, in optical pixels, between the restatement's float32-mode and float64 iterates after maxiter updates."""
    a = restated(kind, target, model, masked, 0.0, maxiter, False)
    b = restated(kind, target, model, masked, 0.0, maxiter, True)
    return C.corner_distance(a['transform'], b['transform'], THERMAL_HW)


@functools.lru_cache(maxsize=None)
def group_features(f32=False):
    optical, thermal, _ = RC.group_case()
    return ([E.image_planes(E.features(o, KSIZE, 'gradient', f32), f32) for o in optical],
            [E.features(t, KSIZE, 'gradient', f32) for t in thermal])


@functools.lru_cache(maxsize=None)
def group_restated(target, model, eps=FIXTURE_EPS, maxiter=50, f32=False):
    planes, templates = group_features(f32)
    return PR.refine_group(planes, templates, start(target), model, eps, maxiter, 0.25, f32)


def group_noise_floor(target, model, maxiter):
    a, b = group_restated(target, model, 0.0, maxiter, False), group_restated(target, model, 0.0, maxiter, True)
    return C.corner_distance(a['transform'], b['transform'], THERMAL_HW)


@functools.lru_cache(maxsize=None)
def shift_groups(target=7.0):
    """(optical [6], thermal [6], group ids [6], truths [3] thermal -> optical, starts [3]) of registration_cases.shift_groups_case."""
    optical, thermal, gid, T = RC.shift_groups_case()
    truths = np.stack([np.linalg.inv(t) for t in T])
    starts = np.stack([C._start_at(truths[g], THERMAL_HW, target, lambda M, g=g: shift_error(M, g)) for g in range(len(T))])
    return optical, thermal, gid, truths, starts


def shift_error(T, g):
    return RC.corner_error(np.linalg.inv(np.asarray(T, np.float64).reshape(3, 3)), RC.shift_groups_case()[3][g])
