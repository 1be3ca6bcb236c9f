"""ctypes binding of libmultipoint_hip.so (C ABI: include/multipoint_hip.h).

There is NO fallback: if the shared library is missing or no gfx950 device is visible, every compute
entry point raises.  PyTorch is used only for device memory and streams.
"""
import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# MP_LIB selects another build of the library (developer tools: the -DMP_TIMING instrumented variant)
LIB_PATH = os.environ.get('MP_LIB') or os.path.join(_HERE, 'libmultipoint_hip.so')



def debug_switch(key, default=None):
    """Developer switch `key` of the MP_DEBUG environment variable (a comma-separated list of `key` / `key=value`; the library
    reads the kernel-selection keys in mp_create, see csrc/api.hip): the value behind '=', '1' for a bare key, `default` if absent."""
    for tok in os.environ.get('MP_DEBUG', '').split(','):
        k, eq, v = tok.strip().partition('=')
        if k == key:
            return v if eq else '1'
    return default


MP_OK = 0
c_void_p, c_int, c_float, c_ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong


class ModelConfig(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ('multispectral', 'descriptor_head', 'descriptor_size',
                                     'normalize_descriptors', 'final_batchnorm', 'reflection_pad',
                                     'bn_first', 'double_convolution', 'channel_version', 'batchnorm',
                                     'key_layout', 'softmax_mode', 'mixed_precision', 'conv_algorithm', 'batch_invariant')]


class Tensor(ctypes.Structure):
    _fields_ = [('name', ctypes.c_char_p), ('data', c_void_p), ('numel', c_ll)]


class PlanLaunch(ctypes.Structure):
    _fields_ = [('name', ctypes.c_char_p)] + [(n, c_int) for n in (
        'kernel', 'images', 'H', 'W', 'pooled', 'tc4', 'ks_shift', 'vin', 'fuse_first', 'in_layout', 'out_layout',
        'workgroups')] + [('items', c_ll)]


MP_PLAN_KERNELS = ('first', 'direct', 'wino43', 'wino43b', 'f16', 'f16_res', 'f16_res_slices')
MP_LAYOUTS = ('nhwc', 'planar', 'xplanar')

MP_PHOTO_MAX_OPS, MP_PHOTO_MAX_TAPS, MP_PHOTO_MAX_BLUR = 16, 11, 801


class PhotometricOp(ctypes.Structure):
    _fields_ = [('kind', c_int), ('ksize', c_int), ('mode', c_int), ('ellipse_offset', c_int), ('ellipse_count', c_int),
                ('field', c_int), ('value', ctypes.c_double), ('key', ctypes.c_ulonglong),
                ('taps', c_float * MP_PHOTO_MAX_TAPS), ('pad', c_int)]


class PhotometricPlan(ctypes.Structure):
    _fields_ = [('n_ops', c_int), ('noise_device', c_int), ('op', PhotometricOp * MP_PHOTO_MAX_OPS)]


(MP_SHAPES_THRESHOLD, MP_SHAPES_MEAN, MP_SHAPES_BLOBS, MP_SHAPES_BOX_BLUR, MP_SHAPES_LINE, MP_SHAPES_CONVEX, MP_SHAPES_POLY,
 MP_SHAPES_ELLIPSE, MP_SHAPES_RANDU) = range(9)
MP_SHAPES_MAX_VERTS, MP_SHAPES_MAX_RADIUS, MP_SHAPES_MAX_BLOBS = 64, 255, 15000


class ShapesCmd(ctypes.Structure):
    _fields_ = [('kind', c_int), ('target', c_int), ('a', c_int * 6), ('resolve', c_int), ('pad', c_int),
                ('u', ctypes.c_double), ('col_a', ctypes.c_double), ('col_b', ctypes.c_double),
                ('min_contrast', ctypes.c_double), ('t', ctypes.c_double), ('key', ctypes.c_ulonglong)]


class MiProblem(ctypes.Structure):
    _fields_ = [('pair', c_int), ('bins', c_int), ('maxiter', c_int), ('maxfun', c_int), ('xatol', ctypes.c_double),
                ('fatol', ctypes.c_double)]


MP_MI_SLOTS = 10
MP_MI_PARAMS_MAX = 9
MP_FRAMES_U8, MP_FRAMES_BGR8, MP_FRAMES_U16 = 0, 1, 2
MP_DRAW_MAX_RADIUS = 64
MP_DRAW_KINDS = {'ring': 0, 'disc': 1, 'cross': 2}
MP_DRAW_MODES = {'blend': 0, 'checker': 1, 'anaglyph': 2, 'difference': 3}

# name -> (restype, argtypes); every symbol declared in include/multipoint_hip.h
SIGNATURES = {
    'mp_create': (c_int, [ctypes.POINTER(c_void_p), c_int]),
    'mp_destroy': (None, [c_void_p]),
    'mp_last_error': (ctypes.c_char_p, [c_void_p]),
    'mp_version': (ctypes.c_char_p, []),
    'mp_device_shape': (c_int, [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    'mp_load_weights': (c_int, [c_void_p, ctypes.POINTER(ModelConfig), ctypes.POINTER(Tensor), c_int]),
    'mp_forward': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p,
                           c_void_p, c_void_p]),
    'mp_forward_plan': (c_int, [c_void_p, c_int, c_int, c_int, c_int, ctypes.POINTER(PlanLaunch), c_int, ctypes.POINTER(c_int)]),
    'mp_forward_batch_stats': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                       c_void_p]),
    'mp_batch_stats_count': (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    'mp_batch_stats_layer': (c_int, [c_void_p, c_int, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(c_int)]),
    'mp_box_nms': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, ctypes.c_double,
                           c_int, c_void_p, c_int, c_void_p]),
    'mp_detect_keypoints': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float,
                                    ctypes.c_double, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    'mp_box_nms_spread': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, ctypes.c_double,
                                  c_int, c_void_p, c_int, c_float, c_void_p]),
    'mp_detect_keypoints_spread': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float,
                                           ctypes.c_double, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_float,
                                           c_void_p, c_void_p]),
    'mp_suppression_radii': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_float, c_void_p, c_void_p]),
    'mp_nms_unresolved': (c_int, [c_void_p, ctypes.POINTER(c_int), c_void_p]),
    'mp_topk_tie_guard': (c_int, [c_void_p, c_float, c_int]),
    'mp_nms_tie_guard': (c_int, [c_void_p, c_int]),
    'mp_topk_ambiguous': (c_int, [c_void_p, ctypes.POINTER(c_int), c_int, ctypes.POINTER(c_int), c_void_p]),
    'mp_extract_keypoints': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, c_void_p,
                                     c_void_p, c_void_p, c_void_p]),
    'mp_sample_descriptors': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                      c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'mp_refine_keypoints': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'mp_sample_descriptors_f': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                        c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'mp_match_mutual_nn': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_ll, c_int, c_int,
                                   c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    'mp_match_nearest': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_ll, c_int, c_int, c_int, c_int,
                                 ctypes.c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'mp_match_guided': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_ll, c_int, c_int, c_int, c_int,
                                c_void_p, c_void_p, c_void_p, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    'mp_match_knn2': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_ll, c_int, c_int, c_int, c_int,
                              c_void_p, c_void_p, c_void_p]),
    'mp_match_threshold': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_ll, c_int, c_int, c_int, c_int,
                                   c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'mp_pair_metrics': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float,
                                c_void_p, c_void_p, c_void_p]),
    'mp_repeatability': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, ctypes.c_double,
                                 c_void_p, c_void_p]),
    'mp_find_homography': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_double, c_int,
                                   ctypes.c_ulonglong, c_void_p, c_void_p, c_void_p, c_void_p]),
    'mp_refine_homography': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_double, c_int,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'mp_find_homography_f': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_double, c_int,
                                     ctypes.c_ulonglong, c_void_p, c_void_p, c_void_p, c_void_p]),
    'mp_refine_homography_f': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, ctypes.c_double, c_int,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'mp_pooled_chunk': (c_int, [ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    'mp_pooled_workspace_bytes': (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_ll)]),
    'mp_pool_matches': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_ll,
                                c_void_p, c_void_p, c_void_p, c_ll, c_void_p]),
    'mp_pool_matches_f': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_ll,
                                  c_void_p, c_void_p, c_void_p, c_ll, c_void_p]),
    'mp_find_homography_pooled': (c_int, [c_void_p, c_void_p, c_void_p, c_ll, c_int, ctypes.c_double, c_int, ctypes.c_ulonglong,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_ll, c_void_p]),
    'mp_refine_homography_pooled': (c_int, [c_void_p, c_void_p, c_void_p, c_ll, c_int, ctypes.c_double, c_int, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_void_p]),
    'mp_find_transform': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, ctypes.c_double, c_int,
                                  ctypes.c_ulonglong, c_void_p, c_void_p, c_void_p, c_void_p]),
    'mp_find_transform_f': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, ctypes.c_double, c_int,
                                    ctypes.c_ulonglong, c_void_p, c_void_p, c_void_p, c_void_p]),
    'mp_refine_transform': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, ctypes.c_double, c_int,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'mp_refine_transform_f': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, ctypes.c_double, c_int,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'mp_find_transform_pooled': (c_int, [c_void_p, c_void_p, c_void_p, c_ll, c_int, c_int, ctypes.c_double, c_int,
                                         ctypes.c_ulonglong, c_void_p, c_void_p, c_void_p, c_void_p, c_ll, c_void_p]),
    'mp_refine_transform_pooled': (c_int, [c_void_p, c_void_p, c_void_p, c_ll, c_int, c_int, ctypes.c_double, c_int, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p]),
    'mp_detector_metrics': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'mp_warp_perspective': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                    c_void_p, c_void_p]),
    'mp_warp_perspective_cv': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    'mp_ha_valid_mask': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'mp_ha_begin': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'mp_ha_accumulate': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                 c_void_p, c_void_p, c_void_p]),
    'mp_ha_finalize': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    'mp_gaussian_filter': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'mp_loss_workspace_bytes': (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_ll)]),
    'mp_detector_loss': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int,
                                 c_void_p, ctypes.c_ulonglong, c_void_p, c_ll, c_void_p, c_void_p]),
    'mp_descriptor_loss': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_int, c_int, c_float, c_float, c_float, c_float, c_int, c_void_p, c_ll,
                                   c_void_p, c_void_p, c_void_p]),
    'mp_detector_loss_backward': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int,
                                          c_int, c_void_p, ctypes.c_ulonglong, c_void_p, c_void_p, c_void_p, c_ll, c_void_p,
                                          c_void_p]),
    'mp_descriptor_loss_backward': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_int, c_int, c_float, c_float, c_float, c_float, c_int,
                                            c_void_p, c_void_p, c_void_p, c_ll, c_void_p, c_void_p, c_void_p]),
    'mp_photometric_workspace_bytes': (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(c_ll)]),
    'mp_photometric_augment': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(PhotometricPlan),
                                       c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_ll, c_void_p]),
    'mp_photometric_shade_mask': (c_int, [c_void_p, c_int, c_int, c_int, ctypes.POINTER(PhotometricPlan), c_void_p, c_int,
                                          c_int, c_int, c_void_p, c_void_p, c_ll, c_void_p]),
    'mp_shapes_workspace_bytes': (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_ll)]),
    'mp_shapes_render': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(ShapesCmd), c_void_p,
                                 c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_ll, c_void_p]),
    'mp_shapes_finish': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                 c_void_p, c_ll, c_void_p]),
    'mp_mi_workspace_bytes': (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_ll)]),
    'mp_mi_joint_histogram': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, ctypes.POINTER(c_int),
                                      ctypes.POINTER(c_int), c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_ll, c_void_p]),
    'mp_mi_objective': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, ctypes.POINTER(c_int),
                                ctypes.POINTER(c_int), c_void_p, c_int, ctypes.c_double, c_int, c_void_p, c_void_p, c_void_p,
                                c_ll, c_void_p]),
    'mp_mi_refine_begin': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, ctypes.POINTER(MiProblem),
                                   c_void_p, c_int, ctypes.c_double, c_int, c_int, c_void_p, c_ll, c_void_p]),
    'mp_mi_refine_step': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'mp_mi_refine_result': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'mp_mi_refine_begin_model': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int,
                                         ctypes.POINTER(MiProblem), c_void_p, c_int, ctypes.c_double, c_int, c_int, c_void_p,
                                         c_ll, c_void_p, c_int, c_void_p]),
    'mp_mi_refine_result_model': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p]),
    'mp_mi_model_transform': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    'mp_gaussian_weights': (c_int, [c_int, ctypes.POINTER(c_float)]),
    'mp_gaussian_blur': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'mp_frames_to_float': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'mp_undistort': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_double),
                             ctypes.POINTER(ctypes.c_double), c_int, ctypes.POINTER(ctypes.c_double), c_int, c_void_p, c_void_p]),
    'mp_resize_bgr8': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'mp_thermal_rescale_workspace_bytes': (c_int, [c_int, ctypes.POINTER(c_ll)]),
    'mp_thermal_rescale': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_ll,
                                   c_void_p]),
    'mp_draw_gray_to_rgb': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_int, c_int, c_int, c_int,
                                    c_void_p]),
    'mp_draw_marks': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int,
                              c_int, c_int, c_int, c_void_p]),
    'mp_draw_matches': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p]),
    'mp_draw_compose': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int,
                                c_int, c_int, c_void_p]),
    'mp_fft_supported': (c_int, [c_int]),
    'mp_fft2d': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    'mp_lghd_quantize': (c_int, [c_void_p, c_void_p, c_void_p, c_ll, c_void_p]),
    'mp_lghd_detect': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    'mp_lghd_workspace_bytes': (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_ll)]),
    'mp_lghd_orientation': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_ll, c_void_p]),
    'mp_lghd_describe': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                 c_void_p]),
    'mp_rift_workspace_bytes': (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_ll)]),
    'mp_phase_congruency': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_float, c_float, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_ll, c_void_p]),
    'mp_rift_detect': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p]),
    'mp_rift_describe': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                 c_void_p]),
    'mp_sift_workspace_bytes': (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(c_ll)]),
    'mp_sift_layout': (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(c_ll)]),
    'mp_sift_scale_space': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_ll, c_void_p]),
    'mp_sift_detect': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_ll, c_void_p, c_void_p, c_void_p,
                               c_int, c_void_p]),
    'mp_sift_select': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_ll,
                               c_void_p]),
    'mp_sift_describe': (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_ll, c_void_p, c_void_p, c_int, c_void_p,
                                 c_void_p]),
    'mp_sift_scatter': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'mp_register_prepare': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    'mp_register_logpolar': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p,
                                     c_void_p]),
    'mp_register_cross_power': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
                                        c_void_p]),
    'mp_register_peak_workspace_bytes': (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_ll)]),
    'mp_register_peak': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_ll, c_void_p]),
    'mp_ecc_workspace_bytes': (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_ll)]),
    'mp_ecc_prepare': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'mp_ecc_sums': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, ctypes.POINTER(c_int), c_void_p, c_int,
                            c_int, c_void_p, c_void_p, c_ll, c_void_p]),
    'mp_ecc_begin': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, ctypes.POINTER(c_int), c_void_p, c_int,
                             c_int, ctypes.c_double, c_int, ctypes.c_double, c_void_p, c_ll, c_void_p]),
    'mp_ecc_step': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'mp_ecc_result': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'mp_ecc_mask_grow': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'mp_ecc_static_update': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'mp_ecc_static_finish': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    'mp_ecc_flag_packed': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, ctypes.POINTER(c_int), c_void_p]),
    'mp_ecc_pooled_workspace_bytes': (c_int, [c_int, c_int, c_int, c_int, ctypes.POINTER(c_ll)]),
    'mp_ecc_pooled_sums': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, ctypes.POINTER(c_int), c_int,
                                   c_void_p, c_void_p, c_int, ctypes.POINTER(c_int), c_int, c_void_p, c_void_p, c_ll, c_void_p]),
    'mp_ecc_pooled_begin': (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, ctypes.POINTER(c_int),
                                    ctypes.POINTER(c_int), c_int, c_void_p, c_void_p, c_int, ctypes.POINTER(c_int), c_int,
                                    ctypes.c_double, c_int, ctypes.c_double, c_void_p, c_ll, c_void_p]),
    'mp_ecc_pooled_step': (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    'mp_ecc_pooled_result': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p]),
    'mp_segments_draw': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_int,
                                 c_void_p]),
    'mp_residual_grid': (c_int, [c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    'mp_residual_field': (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                  ctypes.c_double, ctypes.c_double, c_void_p, c_void_p, c_void_p]),
    'mp_field_fit_workspace': (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_ll)]),
    'mp_field_fit': (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, ctypes.c_double, ctypes.c_double, c_int,
                             ctypes.c_double, c_int, c_void_p, c_ll, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    'mp_field_warp': (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, ctypes.c_double, ctypes.c_double,
                              ctypes.c_double, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    'mp_profile_enable': (c_int, [c_void_p, c_int]),
    'mp_profile_read': (c_int, [c_void_p, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(c_float),
                                ctypes.POINTER(ctypes.c_double), c_int, ctypes.POINTER(c_int)]),
}

_lib = None
_lock = threading.Lock()
_handles = {}


def load_library():
    """dlopen the HIP library and bind every C-ABI symbol (no GPU needed for this step)."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    'multipoint_amd: %s not found. Build it with `python -m multipoint_amd.build` '
                    '(hipcc --offload-arch=gfx950). There is no CPU fallback.' % LIB_PATH)
            lib = ctypes.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
            _lib = lib
    return _lib


class MultiPointHipError(RuntimeError):
    pass


def _err(lib, handle):
    msg = lib.mp_last_error(handle)
    return msg.decode() if msg else 'unknown error'


def check(rc, handle=None):
    if rc != MP_OK:
        lib = load_library()
        msg = _err(lib, handle)
        if rc == -1:
            raise ValueError(msg)
        raise MultiPointHipError('libmultipoint_hip error %d: %s' % (rc, msg))


def require_cuda(device=None):
    if not torch.cuda.is_available():
        raise RuntimeError('multipoint_amd needs an MI355X (gfx950) visible to PyTorch-ROCm; '
                           'torch.cuda.is_available() is False and there is no CPU fallback.')
    if device is None:
        return torch.device('cuda', torch.cuda.current_device())
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError('multipoint_amd computes on the GPU only (got device %s)' % device)
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    return device


class Handle:
    """One mp_handle per (process, device)."""

    def __init__(self, device_index):
        self.lib = load_library()
        self.device_index = device_index
        self.ptr = c_void_p()
        rc = self.lib.mp_create(ctypes.byref(self.ptr), device_index)
        if rc != MP_OK:
            raise MultiPointHipError('mp_create failed: %s' % _err(self.lib, None))

    def check(self, rc):
        check(rc, self.ptr)

    def device_shape(self):
        """(compute units, XCDs, workgroups of a one-per-CU persistent launch) the handle derived from the device."""
        a, b, c = c_int(), c_int(), c_int()
        self.check(self.lib.mp_device_shape(self.ptr, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value

    def forward_plan(self, B, H, W, n_optical=None):
        """The launch plan of mp_forward for a B x H x W forward of the loaded model (n_optical: images the optical encoder of a
        multispectral model receives; default B): a list of dicts, one per planned convolution launch in launch order, with the
        fields of mp_plan_launch (kernel and layouts as names).  Launches nothing."""
        n = c_int()
        no = B if n_optical is None else int(n_optical)
        self.check(self.lib.mp_forward_plan(self.ptr, B, H, W, no, None, 0, ctypes.byref(n)))
        recs = (PlanLaunch * max(n.value, 1))()
        self.check(self.lib.mp_forward_plan(self.ptr, B, H, W, no, recs, n.value, ctypes.byref(n)))
        out = []
        for r in recs[:n.value]:
            d = {k: getattr(r, k) for k, _ in PlanLaunch._fields_}
            d['name'] = r.name.decode()
            d['kernel'] = MP_PLAN_KERNELS[r.kernel]
            d['in_layout'], d['out_layout'] = MP_LAYOUTS[r.in_layout], MP_LAYOUTS[r.out_layout]
            out.append(d)
        return out

    def __del__(self):
        try:
            if self.ptr:
                self.lib.mp_destroy(self.ptr)
        except Exception:
            pass


def get_handle(device=None, key='default'):
    """Shared handle for stateless ops (nms / sampling / matching); models own their own handle."""
    device = require_cuda(device)
    k = (device.index, key)
    with _lock:
        h = _handles.get(k)
    if h is None:
        h = Handle(device.index)
        with _lock:
            _handles[k] = h
    return h


def stream_ptr(device):
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(None)
