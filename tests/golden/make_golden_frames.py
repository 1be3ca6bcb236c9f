#!/usr/bin/env python3
"""Generates tests/golden/frames.npz by running the IMPORTED reference's ImageExtractorRos.preprocess_images on the CPU.  Build
container only:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_frames.py

rosbag, rospy, cv_bridge, tqdm and cv2 are not installed: they are import-time stubs, the five cv2 calls of preprocess_images
(getOptimalNewCameraMatrix, undistort, resize, normalize and the constants) are the restatements of tests/frames_restatement.py,
and cv_bridge hands the seeded arrays through.  The instance is made with object.__new__ (the initialiser opens a bag) and its
name-mangled attributes are set.  What runs is the reference's OWN sequencing: the loop over the calibration file's cameras, the
rotation as a negative-stride view, the size arithmetic of the down-scale, np.percentile and the clip through the alias
`cv_thermal_rescaled = cv_thermal`.  The fixture holds data only: seeds, sizes, parameters and the three outputs per pair."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import frames_restatement as R  # noqa: E402

REFERENCE_CREATE_DATASET = '/root/reference/create_dataset'

# name, optical seed / size, thermal seed / size, params, cameras (label, K size, D)
CASES = [
    ('all_steps', (11, 36, 52), (12, 24, 32),
     {'undistort_images': True, 'image/undistort_alpha': 0.0, 'image/thermal/rotate': True, 'image/optical/downscale': True,
      'image/thermal/rescale_outlier_rejection': True},
     [('optical', R.DISTORTIONS[1]), ('thermal', R.DISTORTIONS[2])]),
    ('alpha_one_no_rotation', (21, 37, 53), (22, 25, 31),
     {'undistort_images': True, 'image/undistort_alpha': 1.0, 'image/thermal/rotate': False, 'image/optical/downscale': True,
      'image/thermal/rescale_outlier_rejection': True},
     [('thermal', R.DISTORTIONS[1]), ('optical', R.DISTORTIONS[2])]),
]


def install_stubs():
    for name in ('rosbag', 'rospy', 'cv_bridge', 'tqdm', 'cv2'):
        sys.modules[name] = types.ModuleType(name)
    sys.modules['tqdm'].tqdm = None
    cv2 = sys.modules['cv2']
    cv2.NORM_MINMAX, cv2.CV_32F = 32, 5
    cv2.getOptimalNewCameraMatrix = lambda K, D, size, alpha: (R.optimal_new_camera_matrix(K, D, size, alpha), (0, 0, 0, 0))

    def undistort(src, K, D, dst, K_new):
        assert dst is None
        return R.undistort(src, K, D, K_new)

    def resize(src, dsize):
        return R.resize_bgr8(src, (dsize[1], dsize[0]))

    def normalize(src, dst, alpha, beta, norm_type, dtype):
        assert dst is None and alpha == 0.0 and beta == 1.0 and norm_type == cv2.NORM_MINMAX and dtype == cv2.CV_32F
        return R.thermal_rescale(src, outlier_rejection=False)[1]
    cv2.undistort, cv2.resize, cv2.normalize = undistort, resize, normalize

    class Bridge:
        def imgmsg_to_cv2(self, msg, encoding):
            assert (encoding, msg.dtype) in (('bgr8', np.uint8), ('mono16', np.uint16))
            return np.array(msg)
    sys.modules['cv_bridge'].CvBridge = Bridge
    sys.path.insert(0, REFERENCE_CREATE_DATASET)
    sys.dont_write_bytecode = True


def main():
    install_stubs()
    import extract_images as E
    out, names = {}, []
    for name, (so, Ho, Wo), (st, Ht, Wt), params, cameras in CASES:
        optical, thermal = R.smooth_bgr8(so, Ho, Wo), R.thermal_u16(st, Ht, Wt)
        calibration = R.calibration_of(cameras, (Ho, Wo), (Ht, Wt))
        ex = object.__new__(E.ImageExtractorRos)
        ex._ImageExtractorRos__params = dict(params)
        ex._ImageExtractorRos__calibration_params = calibration
        ex._ImageExtractorRos__cv_bridge = sys.modules['cv_bridge'].CvBridge()
        o, raw, rescaled = ex.preprocess_images(optical, thermal)
        assert rescaled.dtype == np.float32 and raw.dtype == np.uint16 and o.dtype == np.uint8
        out['case_%s_setup' % name] = np.array([so, Ho, Wo, st, Ht, Wt], np.int64)
        out['case_%s_params' % name] = np.array([float(params[k]) for k in sorted(params)], np.float64)
        out['case_%s_param_keys' % name] = np.array(sorted(params))
        out['case_%s_labels' % name] = np.array([c[0] for c in cameras])
        for k, (label, D) in enumerate(cameras):
            out['case_%s_D%d' % (name, k)] = np.array(D, np.float64)
        out['case_%s_optical_in' % name], out['case_%s_thermal_in' % name] = optical, thermal
        out['case_%s_optical' % name] = np.ascontiguousarray(o)
        out['case_%s_thermal_raw' % name] = np.ascontiguousarray(raw)
        out['case_%s_thermal_rescaled' % name] = np.ascontiguousarray(rescaled)
        names.append(name)
        print(name, 'optical', o.shape, 'thermal', raw.shape, 'counts', raw.min(), raw.max())
    out['case_names'] = np.array(names)
    path = os.path.join(HERE, 'frames.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
