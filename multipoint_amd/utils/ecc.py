"""ECC direct alignment: Gauss-Newton maximisation of the enhanced correlation coefficient (Evangelidis &
Psarakis, PAMI 2008) between a thermal (template) and an optical (image) feature frame on the GPU (csrc/ecc.hip), next to the
mutual-information search of utils.alignment.  An extension: the reference has no gradient-based refinement.

Conventions are those of utils.alignment: frames are fp32 CUDA tensors (H, W), (B, H, W) or (B, 1, H, W); a transform is a 3x3
float64 matrix that maps thermal (template) pixel coordinates to optical (image) ones; results are float64 numpy arrays.

The default feature is the gradient magnitude of the blurred frame: it is the same for a frame and for its contrast-inverted
twin, which is what a visible and a thermal frame of one scene often are.  On raw intensities ('intensity') such a pair has a
correlation near -1, lambda's denominator is not positive and the refinement stops at once with status ECC_LAMBDA.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from .alignment import _frames, _ints, _transforms, gaussian_blur, model_parameters, model_transform

__all__ = ['ecc_features', 'ecc_sums', 'ecc_correlation', 'refine_alignment_ecc_batch', 'ecc_start_transform', 'ECC_MODELS',
           'ECC_FEATURES', 'ECC_OK', 'ECC_FEW_VALID', 'ECC_NOT_POSITIVE', 'ECC_LAMBDA', 'ECC_NONFINITE', 'ecc_sum_count']

ECC_MODELS = {'translation': (3, 2), 'similarity': (1, 4), 'affine': (2, 6), 'homography': (0, 8)}      # (MP_MODEL_*, K)
ECC_FEATURES = {'gradient': 0, 'intensity': 1}                                                           # MP_ECC_*
ECC_OK, ECC_FEW_VALID, ECC_NOT_POSITIVE, ECC_LAMBDA, ECC_NONFINITE = 0, 1, 2, 3, 4


def _model(model):
    if model not in ECC_MODELS:
        raise ValueError('unknown ECC model %r: expected one of %s' % (model, sorted(ECC_MODELS)))
    return ECC_MODELS[model]


def _feature(feature):
    if feature not in ECC_FEATURES:
        raise ValueError('unknown ECC feature %r: expected one of %s' % (feature, sorted(ECC_FEATURES)))
    return ECC_FEATURES[feature]


def ecc_sum_count(model):
    """How many sums one problem of this model has: 6 + K + K (K + 1) / 2 + 2 K."""
    K = _model(model)[1]
    return 6 + K + K * (K + 1) // 2 + 2 * K


def ecc_features(frames, feature='gradient', ksize=5, packed=False):
    """The feature frames of fp32 CUDA frames (H, W), (B, H, W) or (B, 1, H, W): gaussian_blur(., ksize) (ksize odd in 1..31; 1:
    no blur), then for 'gradient' the magnitude of the central differences (BORDER_REFLECT_101: 0 on the border lines), for
    'intensity' the blurred frame itself.  Returns a (B, H, W) tensor; with packed=True also the (B, H, W, 4) tensor
    (f, gx, gy, 0) the sums pass samples as the image.  ValueError: sizes outside 8 x 8 .. 4096 x 4096, an unknown feature, a
    ksize the blur refuses."""
    fid = _feature(feature)
    x = _frames(frames, 'frames')
    ksize = int(ksize)
    if ksize % 2 == 0 or not 1 <= ksize <= 31:
        raise ValueError('ksize must be odd and in [1, 31], got %s' % (ksize,))
    B, H, W = x.shape
    blurred = gaussian_blur(x, ksize) if ksize > 1 else x
    feat = torch.empty_like(blurred)
    pk = torch.empty((B, H, W, 4), dtype=torch.float32, device=x.device) if packed else None
    h = _lib.get_handle(x.device)
    h.check(h.lib.mp_ecc_prepare(h.ptr, _lib.ptr(blurred), B, H, W, fid, _lib.ptr(feat), _lib.ptr(pk), _lib.stream_ptr(x.device)))
    return (feat, pk) if packed else feat


class _Prepared:
    """Both sides' feature frames and a workspace for P problems."""

    def __init__(self, optical, thermal, pair_index, feature, ksize):
        opt, th = _frames(optical, 'optical'), _frames(thermal, 'thermal')
        if opt.shape[0] != th.shape[0]:
            raise ValueError('optical and thermal must hold the same number of frames')
        if opt.device != th.device:
            raise ValueError('optical and thermal must be on the same device')
        self.dev = opt.device
        self.h = _lib.get_handle(self.dev)
        self.B, self.Ho, self.Wo = opt.shape
        self.H, self.W = th.shape[1:]
        self.pair = [int(p) for p in pair_index]
        self.P = len(self.pair)
        _, self.packed = ecc_features(opt, feature, ksize, packed=True)
        self.template = ecc_features(th, feature, ksize)
        need = _lib.c_ll()
        if self.h.lib.mp_ecc_workspace_bytes(self.P, self.H, self.W, ctypes.byref(need)) != _lib.MP_OK:
            raise ValueError('ECC: unsupported sizes (%d problems at %dx%d)' % (self.P, self.H, self.W))
        self.workspace = torch.empty(need.value, dtype=torch.uint8, device=self.dev)
        self.stream = _lib.stream_ptr(self.dev)

    def head(self):
        return (self.h.ptr, _lib.ptr(self.packed), self.Ho, self.Wo, _lib.ptr(self.template), self.H, self.W, self.B,
                _ints(self.pair))

    def tail(self):
        return (_lib.ptr(self.workspace), self.workspace.numel(), self.stream)


def ecc_sums(optical, thermal, pair_index, transforms, model='similarity', feature='gradient', ksize=5):
    """The raw sums of the problems (pair_index[q], transforms[q]) at the given transforms, used as they are: a (P, S) float64
    numpy array in the order n, w, r, ww, rr, wr, G_k, G_k G_l (k <= l, row by row), G_k w, G_k r."""
    mid, _ = _model(model)
    T = _transforms(transforms)
    c = _Prepared(optical, thermal, pair_index, feature, ksize)
    if T.shape[0] != c.P:
        raise ValueError('one pair index and transform per problem')
    Td = torch.from_numpy(T).to(c.dev)
    out = torch.empty((c.P, ecc_sum_count(model)), dtype=torch.float64, device=c.dev)
    c.h.check(c.h.lib.mp_ecc_sums(*c.head(), _lib.ptr(Td), c.P, mid, _lib.ptr(out), *c.tail()))
    return out.cpu().numpy()


def ecc_correlation(optical, thermal, pair_index, transforms, feature='gradient', ksize=5):
    """(rho (P,), valid (P,) int64): the correlation coefficient of the template and the image sampled through each transform
    over the pixels whose footprint lies inside the image, and how many those are.  rho is NaN where none is valid or a side is
    constant."""
    s = ecc_sums(optical, thermal, pair_index, transforms, 'translation', feature, ksize)
    n = s[:, 0]
    with np.errstate(all='ignore'):
        mw, mr = s[:, 1] / n, s[:, 2] / n
        rho = (s[:, 5] - n * mw * mr) / (np.sqrt(s[:, 3] - n * mw * mw) * np.sqrt(s[:, 4] - n * mr * mr))
    return np.where(np.isfinite(rho), rho, np.nan), n.astype(np.int64)


def ecc_start_transform(T0, model, device=None):
    """The matrices a refinement starts from, (P, 3, 3): T0 / T0[2,2] for 'homography' and 'translation';
    model_transform(model_parameters(T0, model), model) for 'similarity' and 'affine' (with their ValueErrors)."""
    _model(model)
    T = _transforms(T0)
    if model in ('similarity', 'affine'):
        return model_transform(model_parameters(T.reshape(-1, 3, 3), model).reshape(T.shape[0], -1), model, device)
    if not (np.isfinite(T).all() and (T[:, 8] != 0.0).all()):
        raise ValueError('ecc_start_transform: need finite 3x3 matrices with T[2,2] != 0')
    return (T / T[:, 8:9]).reshape(-1, 3, 3)


def refine_alignment_ecc_batch(optical, thermal, pair_index, init_transforms, model='similarity', feature='gradient', ksize=5,
                               eps=1e-6, maxiter=50, min_valid=0.25, chunk=8):
    """ECC refinement of a batch of problems (pair_index[q], init_transforms[q]); several problems may share a pair.  Every
    iteration is one sums launch and one solve launch; they are enqueued `chunk` at a time and between chunks one integer, the
    number of problems still running, is read back.  A problem stops when |rho - rho_prev| < eps (converged) or after maxiter
    updates (success without converged); it fails (success False, the last iterate returned) with status ECC_FEW_VALID (fewer
    than min_valid H W template pixels inside the image), ECC_NOT_POSITIVE (G^T G not positive definite), ECC_LAMBDA (lambda's
    denominator <= 0) or ECC_NONFINITE.
    Returns dict(transform (P, 3, 3), rho, nit, success, converged, status) of numpy arrays and 'rounds', the iterations that were
    enqueued (a multiple of `chunk`)."""
    mid, _ = _model(model)
    c = _Prepared(optical, thermal, pair_index, feature, ksize)
    T = ecc_start_transform(init_transforms, model, c.dev).reshape(-1, 9)
    if T.shape[0] != c.P:
        raise ValueError('one pair index and initial transform per problem')
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError('chunk must be positive')
    Td = torch.from_numpy(np.ascontiguousarray(T)).to(c.dev)
    lib = c.h.lib
    c.h.check(lib.mp_ecc_begin(*c.head(), _lib.ptr(Td), c.P, mid, float(eps), int(maxiter), float(min_valid), *c.tail()))
    live = torch.zeros(1, dtype=torch.int32, device=c.dev)
    rounds = 0
    while True:
        c.h.check(lib.mp_ecc_step(c.h.ptr, _lib.ptr(c.workspace), chunk, _lib.ptr(live), c.stream))
        rounds += chunk
        if int(live.item()) == 0:
            break
        if rounds >= int(maxiter) + chunk:                    # every problem stops after maxiter updates at the latest
            raise RuntimeError('ECC: %d problems still run after %d iterations' % (int(live.item()), rounds))
    out_T = torch.empty((c.P, 9), dtype=torch.float64, device=c.dev)
    rho = torch.empty(c.P, dtype=torch.float64, device=c.dev)
    nit, status, conv = (torch.empty(c.P, dtype=torch.int32, device=c.dev) for _ in range(3))
    c.h.check(lib.mp_ecc_result(c.h.ptr, _lib.ptr(c.workspace), _lib.ptr(out_T), _lib.ptr(rho), _lib.ptr(nit), _lib.ptr(status),
                                _lib.ptr(conv), c.stream))
    status = status.cpu().numpy()
    return {'transform': out_T.cpu().numpy().reshape(c.P, 3, 3), 'rho': rho.cpu().numpy(), 'nit': nit.cpu().numpy(),
            'success': status == ECC_OK, 'converged': conv.cpu().numpy().astype(bool), 'status': status, 'rounds': rounds}
