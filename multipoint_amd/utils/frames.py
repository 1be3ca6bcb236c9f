"""Frame preparation: the pixel work of the reference's ImageExtractorRos.preprocess_images (create_dataset/extract_images.py:
167-242) on batches of raw camera frames -- lens undistortion of both cameras, the 180-degree rotation of the thermal frame,
the down-scale of the optical frame to the thermal height, the 1 % / 99 % outlier rejection of the 16-bit thermal frame and its
min-max normalisation.  Reading the bag needs ROS and is not part of this package; everything behind it is arithmetic on two
arrays and a calibration file, and runs in HIP (csrc/frames.hip).  DESIGN.md 3.13 states the arithmetic of every step; cv2 was
not available where this was written, so that section, not OpenCV, is the specification.

    K_new = optimal_new_camera_matrix(K, D, (w, h), alpha)            host, float64
    undistort(frames, K, D, K_new, rotate180=False)                   uint8 (B, H, W, 3) or uint16 (B, H, W)
    resize_bgr8(frames, (oh, ow))                                     uint8 (B, H, W, 3)
    thermal_rescale(thermal_u16, outlier_rejection=True)              -> (thermal_raw_u16, rescaled_fp32, rescaled_u16)
    prepare_frames(optical_bgr8, thermal_u16, params, calibration)    the whole sequence under the reference's yaml keys

Frames are numpy arrays or CUDA tensors; results are CUDA tensors.  There is no CPU path."""
import ctypes

import numpy as np
import torch

from .. import _lib

__all__ = ['optimal_new_camera_matrix', 'undistort', 'resize_bgr8', 'thermal_rescale', 'prepare_frames', 'camera_from_calibration']


def _camera(K, D):
    K = np.asarray(K, np.float64)
    if K.shape != (3, 3):
        raise ValueError('the camera matrix must be 3 x 3, got %s' % (K.shape,))
    D = np.asarray(D, np.float64).reshape(-1)
    if D.size not in (4, 5):
        raise ValueError('4 or 5 distortion coefficients (k1, k2, p1, p2[, k3]), got %d' % D.size)
    return np.ascontiguousarray(K), np.ascontiguousarray(D)


def optimal_new_camera_matrix(K, D, size, alpha):
    """cv2.getOptimalNewCameraMatrix(K, D, (w, h), alpha)[0] as DESIGN.md 3.13 restates it (host, float64): a 9 x 9 grid of
    points (j w / 8, i h / 8), float32, is undistorted to normalised coordinates by FIVE fixed-point iterations (OpenCV releases
    after 4.2 stop on an error bound instead); the inner rectangle is bounded by the innermost points of the grid's four sides,
    the outer one is the bounding box; every entry is v_inner (1 - alpha) + v_outer alpha.  Returns the 3 x 3 matrix."""
    K, D = _camera(K, D)
    w, h = int(size[0]), int(size[1])
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    k1, k2, p1, p2 = D[:4]
    k3 = D[4] if D.size == 5 else 0.0
    j = np.arange(9, dtype=np.float32)
    u = np.broadcast_to(j * np.float32(w) / np.float32(8), (9, 9)).astype(np.float64)
    v = np.broadcast_to((j * np.float32(h) / np.float32(8))[:, None], (9, 9)).astype(np.float64)
    x0, y0 = (u - cx) / fx, (v - cy) / fy
    x, y = x0, y0
    for _ in range(5):
        r2 = x * x + y * y
        icd = 1.0 / (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (x0 - dx) * icd, (y0 - dy) * icd
    inner = (x[:, 0].max(), y[0, :].max(), x[:, 8].min() - x[:, 0].max(), y[8, :].min() - y[0, :].max())
    outer = (x.min(), y.min(), x.max() - x.min(), y.max() - y.min())

    def entries(r):
        f_x, f_y = (w - 1) / r[2], (h - 1) / r[3]
        return f_x, f_y, -f_x * r[0], -f_y * r[1]
    alpha = float(alpha)
    fxn, fyn, cxn, cyn = [a * (1.0 - alpha) + b * alpha for a, b in zip(entries(inner), entries(outer))]
    return np.array([[fxn, 0.0, cxn], [0.0, fyn, cyn], [0.0, 0.0, 1.0]], np.float64)


def _device_frames(frames, name, kinds):
    """frames as a contiguous CUDA tensor of one of `kinds` = {(dtype, rank of a batch)}; one frame may come without the batch
    axis.  Returns (tensor with the batch axis, whether it was added)."""
    if isinstance(frames, np.ndarray):
        a = np.ascontiguousarray(frames)
        if a.dtype == np.uint16:
            x = torch.from_numpy(a.view(np.int16)).to(_lib.require_cuda()).view(torch.uint16)
        elif a.dtype == np.uint8:
            x = torch.from_numpy(a).to(_lib.require_cuda())
        else:
            raise ValueError('%s must be uint8 or uint16, got %s' % (name, a.dtype))
    elif isinstance(frames, torch.Tensor):
        if not frames.is_cuda:
            raise RuntimeError('%s must be a numpy array or a CUDA tensor (multipoint_amd computes on the GPU only)' % name)
        x = frames.contiguous()
    else:
        raise TypeError('%s must be a numpy array or a CUDA tensor' % name)
    for dtype, rank in kinds:
        if x.dtype == dtype and x.dim() in (rank, rank - 1) and (rank == 3 or x.shape[-1] == 3):
            return (x, False) if x.dim() == rank else (x[None], True)
    raise ValueError('%s must be %s, got %s %s' % (name, ' or '.join(
        '%s %s' % (str(d).replace('torch.', ''), '(B, H, W, 3)' if r == 4 else '(B, H, W)') for d, r in kinds),
        str(x.dtype).replace('torch.', ''), tuple(x.shape)))


def _doubles(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def undistort(frames, K, D, K_new, rotate180=False):
    """cv2.undistort(frame, K, D, None, K_new) of uint8 BGR frames (B, H, W, 3) or uint16 frames (B, H, W), one frame without
    the batch axis allowed: the radial-tangential model in float64 per destination pixel, a source position in 1/32 pixel,
    bilinear taps with border 0 (include/multipoint_hip.h, mp_undistort).  rotate180=True returns the result rotated by 180
    degrees ([..., ::-1, ::-1] of the frame axes) from the same pass.  ValueError: other than 4 or 5 coefficients, a matrix
    that is not 3 x 3, a non-finite parameter."""
    K, D = _camera(K, D)
    K_new, _ = _camera(K_new, D)
    x, single = _device_frames(frames, 'frames', ((torch.uint8, 4), (torch.uint16, 3)))
    B, H, W = x.shape[:3]
    out = torch.empty_like(x)
    h = _lib.get_handle(x.device)
    mode = _lib.MP_FRAMES_U16 if x.dtype == torch.uint16 else _lib.MP_FRAMES_BGR8
    h.check(h.lib.mp_undistort(h.ptr, _lib.ptr(x), mode, B, H, W, _doubles(K), _doubles(D), int(D.size), _doubles(K_new),
                               int(bool(rotate180)), _lib.ptr(out), _lib.stream_ptr(x.device)))
    return out[0] if single else out


def resize_bgr8(frames, size):
    """cv2.resize(frame, (ow, oh)) (INTER_LINEAR) of uint8 BGR frames (B, H, W, 3) to size = (oh, ow): OpenCV's 11-bit
    fixed-point path for 8-bit images (mp_resize_bgr8).  The fp32 resize of the SyntheticShapes renderer is another arithmetic."""
    x, single = _device_frames(frames, 'frames', ((torch.uint8, 4),))
    B, H, W = x.shape[:3]
    oh, ow = int(size[0]), int(size[1])
    if oh <= 0 or ow <= 0:
        raise ValueError('resize_bgr8: the target size must be positive, got %s' % ((oh, ow),))
    out = torch.empty((B, oh, ow, 3), dtype=torch.uint8, device=x.device)
    h = _lib.get_handle(x.device)
    h.check(h.lib.mp_resize_bgr8(h.ptr, _lib.ptr(x), B, H, W, oh, ow, _lib.ptr(out), _lib.stream_ptr(x.device)))
    return out[0] if single else out


def thermal_rescale(thermal_u16, outlier_rejection=True):
    """The thermal frame's rescale (extract_images.py:232-240) of uint16 frames (B, H, W), each on its own:

      thermal_raw_u16   the frame with every pixel below np.percentile(frame, 1) set to that bound and every pixel above
                        np.percentile(frame, 99) set to that one -- the float64 bounds land in a uint16 array, so they truncate
      rescaled_fp32     cv2.normalize(thermal_raw, None, 0.0, 1.0, cv2.NORM_MINMAX, cv2.CV_32F)
      rescaled_u16      (rescaled * 65535).astype('uint16'), what the reference saves as <index>_thermal.png

    The order statistics are exact.  outlier_rejection=False: thermal_raw_u16 is the frame itself and the rescale is a plain
    min-max one.  The input is not modified."""
    x, single = _device_frames(thermal_u16, 'thermal_u16', ((torch.uint16, 3),))
    B, H, W = x.shape
    raw = torch.empty_like(x)
    rescaled = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
    saved = torch.empty_like(x)
    h = _lib.get_handle(x.device)
    need = ctypes.c_longlong()
    if h.lib.mp_thermal_rescale_workspace_bytes(B, ctypes.byref(need)) != _lib.MP_OK:
        raise ValueError('thermal_rescale: 1 to 65535 frames, got %d' % B)
    ws = torch.empty(need.value, dtype=torch.uint8, device=x.device)
    h.check(h.lib.mp_thermal_rescale(h.ptr, _lib.ptr(x), B, H, W, int(bool(outlier_rejection)), _lib.ptr(raw), _lib.ptr(rescaled),
                                     _lib.ptr(saved), _lib.ptr(ws), need.value, _lib.stream_ptr(x.device)))
    if single:
        return raw[0], rescaled[0], saved[0]
    return raw, rescaled, saved


def camera_from_calibration(calibration, label):
    """(K, D) of the camera `label` in the reference's calibration layout
    cameras: [{camera: {label, intrinsics: {data: [fx, fy, cx, cy]}, distortion: {parameters: {data: [...]}}}}]"""
    for entry in calibration['cameras']:
        cam = entry['camera']
        if cam['label'] == label:
            i = cam['intrinsics']['data']
            K = np.array([[i[0], 0.0, i[2]], [0.0, i[1], i[3]], [0.0, 0.0, 1.0]], np.float64)
            return K, np.array(cam['distortion']['parameters']['data'], np.float64)
    raise KeyError(label)


_IDENTITY = (np.eye(3), np.zeros(4))          # the undistortion that copies: rotation alone goes through the same kernel


def prepare_frames(optical_bgr8, thermal_u16, params, calibration=None, return_saved=False):
    """preprocess_images (extract_images.py:195-242) on a batch: optical_bgr8 uint8 (B, H, W, 3), thermal_u16 uint16 (B, h, w),
    params the reference's yaml keys

      undistort_images                          undistort both cameras with cv2.getOptimalNewCameraMatrix(K, D, (w, h),
      image/undistort_alpha                     alpha) as the new camera matrix; needs `calibration` (the reference's layout, see
                                                camera_from_calibration) with the labels 'optical' and 'thermal'
      image/thermal/rotate                      thermal[..., ::-1, ::-1] (fused into the undistortion)
      image/optical/downscale                   resize to (int(optical_W * ratio), thermal_H), ratio = float(thermal_H) / optical_H
      image/thermal/rescale_outlier_rejection   the 1 % / 99 % clip in front of the min-max normalisation

    Returns (optical uint8 (B, H', W', 3), thermal_raw uint16 (B, h, w), thermal_rescaled fp32 (B, h, w)) as CUDA tensors: the
    three arrays preprocess_images returns; return_saved=True appends the 16-bit form the reference saves as <index>_thermal.png,
    (thermal_rescaled * 65535).astype('uint16') (B, h, w).  The reference is reproduced as written: it clips through an alias
    (`cv_thermal_rescaled = cv_thermal`), so with outlier rejection thermal_raw is the CLIPPED frame.  Without outlier
    rejection the reference raises NameError (the alias is never bound); here that case is a plain min-max rescale of the
    unclipped frame.  A camera of the calibration file with a label other than 'optical' or 'thermal' raises ValueError with
    the reference's text."""
    opt, _ = _device_frames(optical_bgr8, 'optical_bgr8', ((torch.uint8, 4),))
    th, _ = _device_frames(thermal_u16, 'thermal_u16', ((torch.uint16, 3),))
    if opt.shape[0] != th.shape[0]:
        raise ValueError('prepare_frames: %d optical frames and %d thermal frames' % (opt.shape[0], th.shape[0]))
    rotate = bool(params['image/thermal/rotate'])
    rotated = False
    if params['undistort_images']:
        if calibration is None:
            raise ValueError('prepare_frames: undistort_images needs the calibration parameters')
        alpha = params['image/undistort_alpha']
        for entry in calibration['cameras']:
            label = entry['camera']['label']
            if label not in ('optical', 'thermal'):
                raise ValueError('ERROR unknown camera label: ' + label)
            K, D = camera_from_calibration({'cameras': [entry]}, label)
            if label == 'optical':
                opt = undistort(opt, K, D, optimal_new_camera_matrix(K, D, (opt.shape[2], opt.shape[1]), alpha))
            else:
                # (a second 'thermal' entry undistorts the frame again, as the reference's loop does; only the last pass rotates)
                th = undistort(th, K, D, optimal_new_camera_matrix(K, D, (th.shape[2], th.shape[1]), alpha),
                               rotate180=rotate and entry is _last_thermal(calibration))
                rotated = rotated or (rotate and entry is _last_thermal(calibration))
    if rotate and not rotated:
        th = undistort(th, _IDENTITY[0], _IDENTITY[1], _IDENTITY[0], rotate180=True)
    if params['image/optical/downscale']:
        ratio = float(th.shape[1]) / opt.shape[1]
        opt = resize_bgr8(opt, (int(th.shape[1]), int(opt.shape[2] * ratio)))
    raw, rescaled, saved = thermal_rescale(th, bool(params['image/thermal/rescale_outlier_rejection']))
    return (opt, raw, rescaled, saved) if return_saved else (opt, raw, rescaled)


def _last_thermal(calibration):
    last = None
    for entry in calibration['cameras']:
        if entry['camera']['label'] == 'thermal':
            last = entry
    return last
