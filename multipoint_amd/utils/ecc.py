"""ECC direct alignment: Gauss-Newton maximisation of the enhanced correlation coefficient (Evangelidis &
Psarakis, PAMI 2008) between a thermal (template) and an optical (image) feature frame on the GPU (csrc/ecc.hip), next to the
mutual-information search of utils.alignment.  An extension: the reference has no gradient-based refinement.

Conventions are those of utils.alignment: frames are fp32 CUDA tensors (H, W), (B, H, W) or (B, 1, H, W); a transform is a 3x3
float64 matrix that maps thermal (template) pixel coordinates to optical (image) ones; results are float64 numpy arrays.

The default feature is the gradient magnitude of the blurred frame: it is the same for a frame and for its contrast-inverted
twin, which is what a visible and a thermal frame of one scene often are.  On raw intensities ('intensity') such a pair has a
correlation near -1, lambda's denominator is not positive and the refinement stops at once with status ECC_LAMBDA.

The pooled form (csrc/ecc_pooled.hip) refines ONE transform per group of pairs -- a rig has one for a whole
recording -- with static masks (grow_mask, StaticMask) and per-pair correlations that drive one rejection round:
estimate_shared_transform_ecc, or SharedEccProblem when the frames arrive in batches.
"""
import ctypes

import numpy as np
import torch

from .. import _lib
from .alignment import _frames, _ints, _transforms, gaussian_blur, model_parameters, model_transform

__all__ = ['ecc_features', 'ecc_sums', 'ecc_correlation', 'refine_alignment_ecc_batch', 'ecc_start_transform', 'ECC_MODELS',
           'ECC_FEATURES', 'ECC_OK', 'ECC_FEW_VALID', 'ECC_NOT_POSITIVE', 'ECC_LAMBDA', 'ECC_NONFINITE', 'ecc_sum_count',
           'grow_mask', 'ecc_mask_radii', 'StaticMask', 'SharedEccProblem', 'SharedEccResult', 'ecc_pooled_sums',
           'estimate_shared_transform_ecc']

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


# ---------------------------------------------------------------------------------------------------------------------------
# Pooled ECC: one transform per group of pairs, static masks, one rejection round
# ---------------------------------------------------------------------------------------------------------------------------
def ecc_mask_radii(feature='gradient', ksize=5):
    """(R_t, R_o): the Chebyshev radii by which the excluded set of a thermal (template) and an optical (image) mask is grown so
    that no kept pixel's feature saw an excluded pixel: ksize // 2 for the blur, + 1 for the gradient's central differences; the
    image one more, because the packed plane takes central differences of the feature frame."""
    _feature(feature)
    ksize = int(ksize)
    if ksize % 2 == 0 or not 1 <= ksize <= 31:
        raise ValueError('ksize must be odd and in [1, 31], got %s' % (ksize,))
    rt = ksize // 2 + (1 if feature == 'gradient' else 0)
    return rt, rt + 1


def _ndim(x):
    return x.ndim if hasattr(x, 'ndim') else np.ndim(x)


def _mask_tensor(mask, name, device=None):
    """a bool / uint8 mask (numpy or CUDA tensor), (H, W) or (n, H, W) -> contiguous uint8 CUDA tensor (n, H, W) of 0 / 1."""
    if isinstance(mask, np.ndarray):
        mask = torch.from_numpy(np.ascontiguousarray(mask != 0)).to(_lib.require_cuda(device))
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda:
        raise RuntimeError('%s must be a numpy array or a CUDA tensor (multipoint_amd computes on the GPU only)' % name)
    if mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError('%s must be bool or uint8, got %s' % (name, mask.dtype))
    if mask.dim() == 2:
        mask = mask[None]
    if mask.dim() != 3:
        raise ValueError('%s must be (H, W) or (n, H, W), got %s' % (name, tuple(mask.shape)))
    return (mask != 0).to(torch.uint8).contiguous()


def grow_mask(mask, radius):
    """A use-mask (nonzero = use; bool or uint8, (H, W) or (n, H, W)) with its excluded set grown to every pixel within Chebyshev
    distance `radius` of an excluded one, clipped at the frame (no reflection); radius 0 copies.  Returns a uint8 CUDA tensor of
    0 / 1 in the input's shape."""
    single = mask.ndim == 2
    m = _mask_tensor(mask, 'mask')
    radius = int(radius)
    if radius < 0:
        raise ValueError('radius must not be negative')
    n, H, W = m.shape
    tmp, out = torch.empty_like(m), torch.empty_like(m)
    h = _lib.get_handle(m.device)
    h.check(h.lib.mp_ecc_mask_grow(h.ptr, _lib.ptr(m), n, H, W, radius, _lib.ptr(tmp), _lib.ptr(out), _lib.stream_ptr(m.device)))
    return out[0] if single else out


class StaticMask:
    """The static structure of one camera: a pixel is excluded iff its value is equal in every frame seen (running minimum ==
    running maximum), as a black undistortion margin or a burnt-in overlay is.  update() takes the float frames the features
    are taken from, in any number of batches; mask() the uint8 use-mask (H, W) of 0 / 1."""

    def __init__(self, shape, device=None):
        self.H, self.W = (int(v) for v in shape)
        self.dev = _lib.require_cuda(device)
        self.h = _lib.get_handle(self.dev)
        self.lo = torch.empty((self.H, self.W), dtype=torch.float32, device=self.dev)
        self.hi = torch.empty_like(self.lo)
        self.frames = 0

    def update(self, frames):
        x = _frames(frames, 'frames')
        if tuple(x.shape[1:]) != (self.H, self.W) or x.device != self.dev:
            raise ValueError('StaticMask: frames must be %d x %d on %s' % (self.H, self.W, self.dev))
        self.h.check(self.h.lib.mp_ecc_static_update(self.h.ptr, _lib.ptr(x), x.shape[0], self.H, self.W, int(self.frames == 0),
                                                     _lib.ptr(self.lo), _lib.ptr(self.hi), _lib.stream_ptr(self.dev)))
        self.frames += x.shape[0]
        return self

    def mask(self):
        if self.frames == 0:
            raise ValueError('StaticMask: no frame was seen')
        out = torch.empty((self.H, self.W), dtype=torch.uint8, device=self.dev)
        self.h.check(self.h.lib.mp_ecc_static_finish(self.h.ptr, _lib.ptr(self.lo), _lib.ptr(self.hi), self.H, self.W, _lib.ptr(out),
                                                     _lib.stream_ptr(self.dev)))
        return out


class SharedEccResult:
    """The result of a pooled refinement.  Per group (numpy arrays over G): transform (G, 3, 3), rho, nit, success, converged,
    status, n_included.  Per pair (arrays over the pairs): rho_pair (NaN for a pair that was not included at its group's final
    evaluation), valid_pair (its valid and unmasked pixels there), included, rejected (dropped by the rejection round).  rounds:
    the iterations enqueued over all runs; first: the first run's result when a rejection round followed it, else None."""

    def __init__(self, **fields):
        self.__dict__.update(fields)

    def __repr__(self):
        return 'SharedEccResult(%s)' % ', '.join('%s=%r' % kv for kv in sorted(self.__dict__.items()) if kv[0] != 'first')


class SharedEccProblem:
    """The resident feature planes of a recording's pairs and their groups, for pooled sums and refinements.  add() takes the
    frames in any number of batches (only their feature planes are kept), finish() fixes the masks, then sums(), correlation()
    and refine() may be called any number of times.  auto_mask: build a StaticMask per group and camera from the frames added and
    intersect it with the masks given to finish()."""

    def __init__(self, feature='gradient', ksize=5, auto_mask=False):
        _feature(feature)
        self.feature, self.ksize = feature, int(ksize)
        self.radii = ecc_mask_radii(feature, ksize)
        self.auto_mask = bool(auto_mask)
        self.static = {}                                      # group -> (thermal StaticMask, optical StaticMask)
        self._packed, self._template, self.group = [], [], []
        self.packed = self.template = None
        self.dev = None

    def add(self, optical, thermal, group_index=None):
        if self.packed is not None:
            raise RuntimeError('SharedEccProblem: add() after finish()')
        opt, th = _frames(optical, 'optical'), _frames(thermal, 'thermal')
        if opt.shape[0] != th.shape[0]:
            raise ValueError('optical and thermal must hold the same number of frames')
        if opt.device != th.device:
            raise ValueError('optical and thermal must be on the same device')
        group = [0] * opt.shape[0] if group_index is None else [int(g) for g in group_index]
        if len(group) != opt.shape[0]:
            raise ValueError('one group index per pair')
        if any(g < 0 for g in group):
            raise ValueError('group index outside [0, n_groups)')
        if self.dev is None:
            self.dev, self.ohw, self.thw = opt.device, tuple(opt.shape[1:]), tuple(th.shape[1:])
        elif (opt.device, tuple(opt.shape[1:]), tuple(th.shape[1:])) != (self.dev, self.ohw, self.thw):
            raise ValueError('all optical frames must have one size and all thermal frames one size, on one device')
        self._packed.append(ecc_features(opt, self.feature, self.ksize, packed=True)[1])
        self._template.append(ecc_features(th, self.feature, self.ksize))
        self.group.extend(group)
        if self.auto_mask:
            for g in sorted(set(group)):
                sel = torch.tensor([i for i, v in enumerate(group) if v == g], device=self.dev)
                if g not in self.static:
                    self.static[g] = (StaticMask(self.thw, self.dev), StaticMask(self.ohw, self.dev))
                self.static[g][0].update(th[sel])
                self.static[g][1].update(opt[sel])
        return self

    def _group_masks(self, mask, hw, name, camera):
        """(masks uint8 (n, H, W) grown or None, plane of every group or None, kept share of every group)"""
        G = self.G
        m = None
        if mask is not None:
            m = _mask_tensor(mask, name, self.dev)
            if tuple(m.shape[1:]) != tuple(hw) or m.shape[0] not in (1, G) or (mask.ndim == 3 and m.shape[0] != G):
                raise ValueError('%s must be (H, W) = %s or (G, H, W) with G = %d, got %s' % (name, tuple(hw), G, tuple(m.shape)))
        if self.auto_mask:
            if any(g not in self.static for g in range(G)):
                raise ValueError('a group without a pair has no static mask')
            auto = torch.stack([self.static[g][camera].mask() for g in range(G)])
            m = auto if m is None else (auto & m.expand(G, -1, -1)).contiguous()
        if m is None:
            return None, None, [1.0] * G
        m = grow_mask(m, self.radii[camera])
        index = [0] * G if m.shape[0] == 1 else list(range(G))
        share = m.to(torch.float32).mean(dim=(1, 2)).cpu().numpy()
        return m, index, [float(share[i]) for i in index]

    def finish(self, thermal_mask=None, optical_mask=None, n_groups=None):
        """Fixes the groups (n_groups: their number, default the largest index + 1) and the masks: (H, W) for all groups or
        (G, H, W), nonzero = use, of the thermal and the optical camera.  They are grown by ecc_mask_radii here."""
        if self.packed is not None:
            raise RuntimeError('SharedEccProblem: finish() twice')
        if not self.group:
            raise ValueError('SharedEccProblem: no pair was added')
        self.G = max(self.group) + 1 if n_groups is None else int(n_groups)
        self.P = len(self.group)
        self.h = _lib.get_handle(self.dev)
        self.stream = _lib.stream_ptr(self.dev)
        self.tmasks, self.tindex, self.thermal_kept = self._group_masks(thermal_mask, self.thw, 'thermal_mask', 0)
        omasks, oindex, self.optical_kept = self._group_masks(optical_mask, self.ohw, 'optical_mask', 1)
        need = _lib.c_ll()
        if self.h.lib.mp_ecc_pooled_workspace_bytes(self.P, self.G, self.thw[0], self.thw[1], ctypes.byref(need)) != _lib.MP_OK:
            raise ValueError('pooled ECC: unsupported sizes (%d pairs in %d groups at %dx%d)' % ((self.P, self.G) + self.thw))
        if any(g >= self.G for g in self.group):
            raise ValueError('group index outside [0, n_groups)')
        packed = self._packed[0] if len(self._packed) == 1 else torch.cat(self._packed)
        self.template = self._template[0] if len(self._template) == 1 else torch.cat(self._template)
        self._packed, self._template = [], []
        if omasks is not None:
            self.h.check(self.h.lib.mp_ecc_flag_packed(self.h.ptr, _lib.ptr(packed), self.P, self.ohw[0], self.ohw[1],
                                                       _lib.ptr(omasks), omasks.shape[0], _ints(oindex[g] for g in self.group),
                                                       self.stream))
        self.packed = packed
        self.workspace = torch.empty(need.value, dtype=torch.uint8, device=self.dev)
        return self

    def bytes_resident(self):
        """Bytes of the planes and the workspace that stay on the device between calls."""
        t = [self.packed, self.template, self.workspace] + ([self.tmasks] if self.tmasks is not None else [])
        return int(sum(x.numel() * x.element_size() for x in t))

    def _head(self):
        return (self.h.ptr, _lib.ptr(self.packed), self.ohw[0], self.ohw[1], _lib.ptr(self.template), self.thw[0], self.thw[1],
                self.P, _ints(self.group))

    def _masks(self):
        if self.tmasks is None:
            return (_lib.ptr(None), 0, None)
        return (_lib.ptr(self.tmasks), self.tmasks.shape[0], _ints(self.tindex))

    def _group_transforms(self, transforms):
        T = _transforms(transforms)
        if T.shape[0] == 1 and _ndim(transforms) == 2:
            T = np.repeat(T, self.G, axis=0)
        if T.shape[0] != self.G:
            raise ValueError('one transform, or one per group (%d), got %d' % (self.G, T.shape[0]))
        return T

    def sums(self, transforms, model='similarity'):
        """The raw sums of every pair at the transform of its group over its valid and unmasked pixels: (P, S) float64."""
        mid, _ = _model(model)
        Td = torch.from_numpy(self._group_transforms(transforms)).to(self.dev)
        out = torch.empty((self.P, ecc_sum_count(model)), dtype=torch.float64, device=self.dev)
        self.h.check(self.h.lib.mp_ecc_pooled_sums(*self._head(), self.G, _lib.ptr(Td), *self._masks(), mid, _lib.ptr(out),
                                                   _lib.ptr(self.workspace), self.workspace.numel(), self.stream))
        return out.cpu().numpy()

    def correlation(self, transforms):
        """(rho (G,), rho_pair (P,), valid_pair (P,) int64) at given transforms: the pooled correlation coefficient of every
        group over its pairs with a positive variance on both sides, and each pair's own."""
        s = self.sums(transforms, 'translation')
        n = s[:, 0]
        with np.errstate(all='ignore'):
            mw, mr = s[:, 1] / n, s[:, 2] / n
            ww, rr, c = s[:, 3] - n * mw * mw, s[:, 4] - n * mr * mr, s[:, 5] - n * mw * mr
            ok = np.isfinite(s).all(axis=1) & (ww > 0) & (rr > 0)
            rho_pair = np.where(ok, c / (np.sqrt(ww) * np.sqrt(rr)), np.nan)
            rho = np.full(self.G, np.nan)
            group = np.asarray(self.group)
            for g in range(self.G):
                sel = ok & (group == g)
                if sel.any():
                    rho[g] = c[sel].sum() / (np.sqrt(ww[sel].sum()) * np.sqrt(rr[sel].sum()))
        return rho, rho_pair, n.astype(np.int64)

    def _run(self, T, mid, eps, maxiter, min_valid, chunk, active):
        lib = self.h.lib
        Td = torch.from_numpy(np.ascontiguousarray(T.reshape(-1, 9))).to(self.dev)
        self.h.check(lib.mp_ecc_pooled_begin(*self._head(), _ints(active), self.G, _lib.ptr(Td), *self._masks(), mid, float(eps),
                                             int(maxiter), float(min_valid), _lib.ptr(self.workspace), self.workspace.numel(),
                                             self.stream))
        live = torch.zeros(1, dtype=torch.int32, device=self.dev)
        rounds = 0
        while True:
            self.h.check(lib.mp_ecc_pooled_step(self.h.ptr, _lib.ptr(self.workspace), chunk, _lib.ptr(live), self.stream))
            rounds += chunk
            if int(live.item()) == 0:
                break
            if rounds >= int(maxiter) + chunk:                # every group stops after maxiter updates at the latest
                raise RuntimeError('pooled ECC: %d groups still run after %d iterations' % (int(live.item()), rounds))
        G, P = self.G, self.P
        out_T = torch.empty((G, 9), dtype=torch.float64, device=self.dev)
        rho = torch.empty(G, dtype=torch.float64, device=self.dev)
        nit, status, conv, ninc = (torch.empty(G, dtype=torch.int32, device=self.dev) for _ in range(4))
        rho_pair, n_pair = (torch.empty(P, dtype=torch.float64, device=self.dev) for _ in range(2))
        inc = torch.empty(P, dtype=torch.int32, device=self.dev)
        self.h.check(lib.mp_ecc_pooled_result(self.h.ptr, _lib.ptr(self.workspace), _lib.ptr(out_T), _lib.ptr(rho), _lib.ptr(nit),
                                              _lib.ptr(status), _lib.ptr(conv), _lib.ptr(ninc), _lib.ptr(rho_pair), _lib.ptr(n_pair),
                                              _lib.ptr(inc), self.stream))
        status = status.cpu().numpy()
        return SharedEccResult(transform=out_T.cpu().numpy().reshape(G, 3, 3), rho=rho.cpu().numpy(), nit=nit.cpu().numpy(),
                               success=status == ECC_OK, converged=conv.cpu().numpy().astype(bool), status=status,
                               n_included=ninc.cpu().numpy(), rho_pair=rho_pair.cpu().numpy(),
                               valid_pair=n_pair.cpu().numpy().astype(np.int64), included=inc.cpu().numpy().astype(bool),
                               rejected=np.zeros(P, bool), rounds=rounds, first=None)

    def refine(self, init_transforms, model='similarity', eps=1e-6, maxiter=50, min_valid=0.25, chunk=8, active=None,
               reject_ratio=0.5):
        """The pooled refinement and its rejection round: see estimate_shared_transform_ecc."""
        mid, _ = _model(model)
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError('chunk must be positive')
        reject_ratio = float(reject_ratio)
        if not 0.0 <= reject_ratio <= 1.0:
            raise ValueError('reject_ratio must be in [0, 1], got %s' % (reject_ratio,))
        T0 = _transforms(init_transforms)
        if not (T0.shape[0] == self.G or (T0.shape[0] == 1 and _ndim(init_transforms) == 2)):
            raise ValueError('one initial transform, or one per group (%d), got %d' % (self.G, T0.shape[0]))
        T = ecc_start_transform(T0, model, self.dev).reshape(-1, 9)
        if T.shape[0] != self.G:
            T = np.repeat(T, self.G, axis=0)
        active = np.ones(self.P, bool) if active is None else np.asarray(active).astype(bool).reshape(-1)
        if active.shape[0] != self.P:
            raise ValueError('one active flag per pair')
        first = self._run(T, mid, eps, maxiter, min_valid, chunk, active)
        if reject_ratio == 0.0:
            return first
        group = np.asarray(self.group)
        keep, rerun = active.copy(), np.zeros(self.G, bool)
        for g in range(self.G):
            mine = group == g
            inc = mine & first.included
            if not (first.success[g] and inc.any()):
                continue
            m = float(np.median(first.rho_pair[inc]))
            if not m > 0.0:
                continue
            stay = inc & (first.rho_pair >= reject_ratio * m)
            if stay.any() and (stay != (mine & active)).any():
                keep[mine] = stay[mine]
                rerun[g] = True
        if not rerun.any():
            return first
        second = self._run(first.transform, mid, eps, maxiter, min_valid, chunk, keep & rerun[group])
        out = SharedEccResult(**{k: np.array(v) if isinstance(v, np.ndarray) else v for k, v in first.__dict__.items()})
        for k in ('transform', 'rho', 'nit', 'success', 'converged', 'status', 'n_included'):
            getattr(out, k)[rerun] = getattr(second, k)[rerun]
        sel = rerun[group]
        for k in ('rho_pair', 'valid_pair', 'included'):
            getattr(out, k)[sel] = getattr(second, k)[sel]
        out.rejected = active & ~keep
        out.rounds = first.rounds + second.rounds
        out.first = first
        return out


def _problem(optical, thermal, group_index, feature, ksize, thermal_mask, optical_mask, n_groups=None):
    return SharedEccProblem(feature, ksize).add(optical, thermal, group_index).finish(thermal_mask, optical_mask, n_groups)


def ecc_pooled_sums(optical, thermal, group_index, transforms, model='similarity', feature='gradient', ksize=5, thermal_mask=None,
                    optical_mask=None):
    """The raw sums (ecc_sums' order) of every pair at the transform of its group, transforms (3, 3) or (G, 3, 3), over the pixels
    that are valid, kept by the thermal mask and sampled from four taps the optical mask keeps; the masks ((H, W) or (G, H, W),
    nonzero = use) are grown by ecc_mask_radii first.  A (P, S) float64 numpy array; with no mask its rows have the bits of
    ecc_sums."""
    T = _transforms(transforms)
    n_groups = T.shape[0] if _ndim(transforms) == 3 or T.shape[0] > 1 else None
    return _problem(optical, thermal, group_index, feature, ksize, thermal_mask, optical_mask, n_groups).sums(transforms, model)


def estimate_shared_transform_ecc(optical, thermal, init_transforms, group_index=None, model='similarity', feature='gradient',
                                  ksize=5, eps=1e-6, maxiter=50, min_valid=0.25, chunk=8, thermal_mask=None, optical_mask=None,
                                  active=None, reject_ratio=0.5):
    """ECC refinement of ONE transform per group of pairs: pair i (optical[i], thermal[i]) belongs to group
    group_index[i] (default: one group), whose transform maximises the correlation coefficient of the concatenation of its
    pairs' centred feature vectors.  init_transforms: (3, 3) for every group or (G, 3, 3); the start is ecc_start_transform.
    Masks: (H, W) for all groups or (G, H, W), bool or uint8, nonzero = use, one for the thermal and one for the optical camera;
    their excluded sets are grown by ecc_mask_radii(feature, ksize).  active: a flag per pair, False leaves the pair out.

    At every evaluation a pair is included iff it is active, at least min_valid of the template pixels its mask keeps are valid,
    its sums are finite and both its variances are positive; a group without an included pair fails with ECC_FEW_VALID, the other
    stop and failure rules are refine_alignment_ecc_batch's.  Iterations are enqueued `chunk` at a time.

    The rejection round: after a successful first run a group's pairs whose own correlation is below reject_ratio times the
    group's median (taken over the included pairs, if it is positive), and the pairs that were not included, are dropped; if that
    changed anything and a pair stays, the group runs once more from the first run's transform.  reject_ratio 0 switches the
    round off; the default of 0.5 is a guess: no recording was available to set it on.

    Returns a SharedEccResult: the fields are those of the last run of every group, `first` the first run's."""
    T = _transforms(init_transforms)
    n_groups = T.shape[0] if _ndim(init_transforms) == 3 or T.shape[0] > 1 else None
    reject_ratio = float(reject_ratio)
    if not 0.0 <= reject_ratio <= 1.0:
        raise ValueError('reject_ratio must be in [0, 1], got %s' % (reject_ratio,))
    prob = _problem(optical, thermal, group_index, feature, ksize, thermal_mask, optical_mask, n_groups)
    return prob.refine(init_transforms, model, eps, maxiter, min_valid, chunk, active, reject_ratio)
