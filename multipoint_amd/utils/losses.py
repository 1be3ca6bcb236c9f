"""SuperPointLoss (multipoint/utils/losses.py:8-272) on the GPU: the detector loss and the dense descriptor loss run as
HIP kernels (csrc/losses.hip through mp_detector_loss / mp_descriptor_loss) whose working set is O(B * Hc*Wc); the
reference's B x (Hc*Wc)^2 distance, correspondence, dot-product, hinge and mask tensors never exist.  Torch only
allocates, uploads and forms the batch means of the per-image sums the kernels return.

Reachable as getattr(multipoint_amd.utils.losses, config['loss']['type']) like the reference's module.  The loss is
differentiable: when grad mode is on and a `logits` / `desc` input requires grad, forward() and evaluate() return values
with an autograd graph whose backward runs the HIP gradient kernels (mp_detector_loss_backward /
mp_descriptor_loss_backward), so `loss.backward()` in train.py fills the inputs' .grad.  The values are the same bits as
without grad.  Double backward is not supported; the sparse descriptor loss still raises.

Two keys beyond the reference's default_config:
  label_noise       'host' (default): the cross-entropy labels' tie-break noise is torch.rand((B, 64, Hc, Wc)) from the CPU
                    default generator, drawn with the reference's call in its order (image 1, then image 2), so that
                    under the same torch.manual_seed the labels are the reference's; uploaded from pinned memory.
                    'device': a counter-based hash of (label_noise_seed, b, c, h, w) on the GPU, no host draw and no use of
                    the torch generator.  Labels equal 'host' ones in every cell with <= 1 keypoint; in cells with several
                    keypoints it picks one of them deterministically.
  label_noise_seed  seed of the 'device' noise (int).
"""
import copy
import ctypes

import torch

from .. import _lib
from .utils import dict_update

__all__ = ['SuperPointLoss', 'descriptor_loss_sums']

_DESC_SIZES = (64, 128, 256)


def _as_flag_map(t, dev):
    """(B, H, W) map -> contiguous uint8 device tensor, nonzero = set (bool is reinterpreted, CPU data is uploaded)."""
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    elif t.dtype != torch.uint8:
        t = (t != 0).view(torch.uint8)                   # label preprocessing: 0/1 numeric maps
    t = t.to(dev).contiguous()
    if t.data_ptr() % 8:                                 # the kernels read 8 pixels per load
        t = t.clone()
    return t


def _channels_last(desc, dev):
    """(B, D, Hc, Wc) -> [B][Hc][Wc][D] fp32 storage: the model's output (a permuted view of channels-last storage) is used
    as it is, any other tensor is copied into that layout."""
    d = desc.permute(0, 2, 3, 1)
    if d.dtype != torch.float32 or d.device != dev or not d.is_contiguous():
        d = d.to(dev, torch.float32).contiguous()
    return d


class SuperPointLoss(torch.nn.Module):
    '''
    Loss to train the SuperPoint model according to:
    "SuperPoint: Self-Supervised Interest Point Detection and Description"
    (forward-only evaluation; see the module docstring)
    '''
    default_config = {
        'detector_loss': True,
        'detector_use_cross_entropy': True,
        'descriptor_loss': True,
        'descriptor_loss_threshold': 8.0,
        'sparse_descriptor_loss': False,
        'sparse_descriptor_loss_num_cell_divisor': 64,
        'descriptor_loss_use_mask': True,
        'positive_margin': 1.0,
        'negative_margin': 0.2,
        'lambda_d': 250,
        'lambda': 0.0001,
    }
    noise_defaults = {
        'label_noise': 'host',
        'label_noise_seed': 0,
    }

    def __init__(self, config=None):
        super(SuperPointLoss, self).__init__()
        # merged into a copy: the reference's dict_update(self.default_config, config) also rewrites the class defaults
        self.config = dict_update(copy.deepcopy(self.default_config), copy.deepcopy(self.noise_defaults))
        if config:
            self.config = dict_update(self.config, config)
        self._check_config()

    def _check_config(self):
        if self.config['sparse_descriptor_loss'] and self.config['descriptor_loss']:
            raise NotImplementedError(
                'SuperPointLoss: sparse_descriptor_loss is not supported. It draws random cells, its `valid` term tests '
                'index 0 of the warped cells against both Hc and Wc (reference losses.py:159-162), and it is not the '
                'default; use the dense descriptor loss (sparse_descriptor_loss: false)')
        if self.config['label_noise'] not in ('host', 'device'):
            raise ValueError("SuperPointLoss: label_noise must be 'host' or 'device', got %r" % (self.config['label_noise'],))

    def component_keys(self, pair):
        """Keys of the components dict, in the order evaluate() returns their values."""
        keys = []
        if self.config['detector_loss']:
            keys.append('detector_loss1')
            if pair:
                keys.append('detector_loss2')
        if self.config['descriptor_loss']:
            keys += ['descriptor_loss', 'positive_dist', 'negative_dist']
        return tuple(keys)

    def forward(self, pred, data, pred2=None, data2=None):
        """(loss, components): loss a [1] fp32 device tensor, components a dict of floats (one host synchronisation)."""
        values, keys = self.evaluate(pred, data, pred2, data2)
        host = values.cpu().tolist()
        return values[:1].to(torch.float32), {k: host[i + 1] for i, k in enumerate(keys)}

    def evaluate(self, pred, data, pred2=None, data2=None):
        """(values, keys) without a host synchronisation: values is a float64 device tensor [1 + len(keys)] holding the
        total loss followed by the components named by keys (a loop can accumulate it on the device and sync once).
        With grad mode on and a logits / desc input that requires grad, values carries the graph of the HIP backward."""
        if ((pred2 is None and data2 is not None) or
                (pred2 is not None and data2 is None)):
            raise ValueError('The data and the label must be present to compute the loss')
        self._check_config()
        cfg = self.config
        if cfg['descriptor_loss'] and pred2 is None:
            raise ValueError('The descriptor loss requires predictions from two images')
        preds = (pred, pred2) if pred2 is not None else (pred,)
        used = [p.get(k) for k, on in (('logits', cfg['detector_loss']), ('desc', cfg['descriptor_loss'])) if on
                for p in preds]
        if torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in used):
            return self._evaluate_with_grad(pred, data, pred2, data2)
        with torch.no_grad():
            return self._evaluate(pred, data, pred2, data2)

    def _evaluate_with_grad(self, pred, data, pred2, data2):
        """The dtype / device / layout conversions as differentiable torch ops, then the kernels inside _LossFunction:
        the gradients come back in each input's dtype, device and shape."""
        cfg = self.config
        ref = pred['desc'] if cfg['descriptor_loss'] else pred['logits']
        dev = _lib.require_cuda(ref.device if ref.device.type == 'cuda' else None)
        sides = (pred, pred2)
        args = []
        for p in sides:
            lg = p.get('logits') if (p is not None and cfg['detector_loss']) else None
            args.append(lg.to(dev, torch.float32).contiguous() if torch.is_tensor(lg) else lg)
        for p in sides:
            d = p.get('desc') if (p is not None and cfg['descriptor_loss']) else None
            args.append(_channels_last(d, dev) if torch.is_tensor(d) and d.dim() == 4 else d)   # [B][Hc][Wc][D]
        return _LossFunction.apply(self, (pred, data, pred2, data2), *args), self.component_keys(pred2 is not None)

    def _evaluate(self, pred, data, pred2, data2, state=None):
        """The kernels' evaluation; `state` (a dict or None) receives what the backward needs."""
        cfg = self.config
        pair = pred2 is not None
        keys = self.component_keys(pair)

        ref = pred['desc'] if cfg['descriptor_loss'] else pred['logits']
        dev = _lib.require_cuda(ref.device if ref.device.type == 'cuda' else None)
        B, Hc, Wc = ref.shape[0], ref.shape[2], ref.shape[3]
        H, W = 8 * Hc, 8 * Wc
        h = _lib.get_handle(dev)
        nbytes = ctypes.c_longlong()
        if h.lib.mp_loss_workspace_bytes(B, H, W, ctypes.byref(nbytes)) != _lib.MP_OK:
            raise ValueError('SuperPointLoss: unsupported batch / frame %d x %dx%d' % (B, H, W))
        workspace = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        stream = _lib.stream_ptr(dev)
        valid = [self._valid(d, dev, B, H, W) for d in ((data, data2) if pair else (data,))]

        if state is not None:
            state.update(dev=dev, B=B, Hc=Hc, Wc=Wc, keys=keys, det=[], desc=None)
        parts = []
        total = torch.zeros((), dtype=torch.float64, device=dev)
        if cfg['detector_loss']:
            for side, (p, d) in enumerate(((pred, data), (pred2, data2))[:2 if pair else 1]):
                det = self._detector_loss(h, p, d, valid[side], side, B, Hc, Wc, dev, workspace, stream, state)
                total = total + det
                parts.append(det)
        if cfg['descriptor_loss']:
            desc = self._descriptor_loss(pred, data, pred2, data2, valid, workspace, state)
            total = total + float(cfg['lambda']) * desc[0]
            parts += list(desc)
        return torch.stack([total] + parts), keys

    @staticmethod
    def _valid(d, dev, B, H, W):
        v = d.get('valid_mask')
        if v is None:
            return None
        if tuple(v.shape) not in ((B, 1, H, W), (B, H, W)):
            raise ValueError('SuperPointLoss: valid_mask of shape %s does not match %d x 1 x %d x %d'
                             % (tuple(v.shape), B, H, W))
        return _as_flag_map(v.reshape(B, H, W), dev)

    def _noise(self, B, Hc, Wc, dev):
        """The reference's torch.rand(labels.shape) (losses.py:102), drawn into pinned memory and uploaded asynchronously."""
        buf = torch.empty((B, 64, Hc, Wc), dtype=torch.float32, pin_memory=True)
        torch.rand((B, 64, Hc, Wc), out=buf)
        return buf.to(dev, non_blocking=True)

    def _detector_loss(self, h, pred, data, valid, side, B, Hc, Wc, dev, workspace, stream, state=None):
        cfg = self.config
        logits = pred['logits']
        if logits is None:
            raise ValueError('SuperPointLoss: the detector loss needs pred["logits"] (set the model\'s force_return_logits)')
        if tuple(logits.shape) != (B, 65, Hc, Wc):
            raise ValueError('SuperPointLoss: logits of shape %s, expected %s' % (tuple(logits.shape), (B, 65, Hc, Wc)))
        logits = logits.to(dev, torch.float32).contiguous()
        kp = data['keypoints']
        if tuple(kp.shape) != (B, 8 * Hc, 8 * Wc):
            raise ValueError('SuperPointLoss: keypoints of shape %s, expected %s' % (tuple(kp.shape), (B, 8 * Hc, 8 * Wc)))
        kp = _as_flag_map(kp, dev)
        use_ce = bool(cfg['detector_use_cross_entropy'])
        noise, seed = None, 0
        if use_ce:
            if cfg['label_noise'] == 'host':
                noise = self._noise(B, Hc, Wc, dev)
            else:
                seed = (int(cfg['label_noise_seed']) * 2 + side) & 0xFFFFFFFFFFFFFFFF
        out = torch.empty((B, 2), dtype=torch.float64, device=dev)
        h.check(h.lib.mp_detector_loss(h.ptr, _lib.ptr(logits), B, Hc, Wc, _lib.ptr(kp), _lib.ptr(valid), 8 * Hc, 8 * Wc,
                                       int(use_ce), _lib.ptr(noise), seed, _lib.ptr(workspace), workspace.numel(),
                                       _lib.ptr(out), stream))
        if state is not None:
            state['det'].append(dict(kp=kp, valid=valid, use_ce=use_ce, noise=noise, seed=seed, out=out))
        return (out[:, 0] / out[:, 1]).mean()           # a zero count gives NaN, as the reference's division does

    def _descriptor_loss(self, pred, data, pred2, data2, valid, workspace, state=None):
        cfg = self.config
        d1, d2 = pred['desc'], pred2['desc']
        if d1 is None or d2 is None:
            raise ValueError('SuperPointLoss: the descriptor loss needs pred["desc"] of both images')
        if tuple(d1.shape) != tuple(d2.shape):
            raise ValueError('SuperPointLoss: descriptor shapes differ: %s vs %s' % (tuple(d1.shape), tuple(d2.shape)))
        hom = [d.get('homography') for d in (data, data2)]
        keep = {} if state is not None else None
        out = _descriptor_sums(d1, d2, hom[0], hom[1], valid[0], valid[1], cfg, workspace, None, keep)
        if state is not None:
            state['desc'] = dict(keep, out=out)
        pos, neg, norm = out[:, 0], out[:, 1], out[:, 3]
        return ((pos + neg) / norm).mean(), (pos / norm).mean(), (neg / norm).mean()


def descriptor_loss_sums(desc1, desc2, homography1, homography2, valid_mask1, valid_mask2, config, workspace=None,
                         warped=None):
    """Per-image sums of the dense descriptor loss (mp_descriptor_loss): a float64 device tensor [B][4] of lambda_d * the
    positive sum, the negative sum, the number of corresponding valid pairs and the normalisation.  desc (B, D, Hc, Wc),
    homography (B, 3, 3) or None, valid_mask (B, [1,] H, W) or None, config the loss keys.  `warped`, a [2][B][Hc*Wc][2]
    fp32 device tensor, receives the warped cell centres (y, x) of side 1 and side 2."""
    return _descriptor_sums(desc1, desc2, homography1, homography2, valid_mask1, valid_mask2, config, workspace, warped)


def _descriptor_sums(desc1, desc2, homography1, homography2, valid_mask1, valid_mask2, config, workspace=None, warped=None,
                     keep=None):
    """descriptor_loss_sums; `keep` (a dict or None) receives the kernel's inputs for the backward."""
    dev = _lib.require_cuda(desc1.device if desc1.device.type == 'cuda' else None)
    if tuple(desc1.shape) != tuple(desc2.shape):
        raise ValueError('SuperPointLoss: descriptor shapes differ: %s vs %s' % (tuple(desc1.shape), tuple(desc2.shape)))
    B, D, Hc, Wc = desc1.shape
    H, W = 8 * Hc, 8 * Wc
    if D not in _DESC_SIZES:
        raise ValueError('SuperPointLoss: descriptor size %d is not one of %s' % (D, _DESC_SIZES))
    d1, d2 = _channels_last(desc1, dev), _channels_last(desc2, dev)
    hom = []
    for m in (homography1, homography2):
        if m is not None:
            if tuple(m.shape) != (B, 3, 3):
                raise ValueError('SuperPointLoss: homography of shape %s, expected %s' % (tuple(m.shape), (B, 3, 3)))
            m = m.to(dev, torch.float32).contiguous()
        hom.append(m)
    valid = []
    for v in (valid_mask1, valid_mask2):
        if v is not None:
            if v.numel() != B * H * W:
                raise ValueError('SuperPointLoss: valid_mask of shape %s does not match %d x %d x %d' % (tuple(v.shape), B, H, W))
            v = _as_flag_map(v.reshape(B, H, W), dev)
        valid.append(v)
    if warped is not None and (warped.dtype != torch.float32 or warped.device != dev or not warped.is_contiguous()
                               or warped.numel() != 2 * B * Hc * Wc * 2):
        raise ValueError('SuperPointLoss: warped must be a contiguous fp32 [2][B][Hc*Wc][2] tensor on %s' % dev)
    h = _lib.get_handle(dev)
    if workspace is None:
        nbytes = ctypes.c_longlong()
        if h.lib.mp_loss_workspace_bytes(B, H, W, ctypes.byref(nbytes)) != _lib.MP_OK:
            raise ValueError('SuperPointLoss: unsupported batch / frame %d x %dx%d' % (B, H, W))
        workspace = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    out = torch.empty((B, 4), dtype=torch.float64, device=dev)
    h.check(h.lib.mp_descriptor_loss(
        h.ptr, _lib.ptr(d1), _lib.ptr(d2), B, Hc, Wc, D, _lib.ptr(hom[0]), _lib.ptr(hom[1]), _lib.ptr(valid[0]),
        _lib.ptr(valid[1]), H, W, float(config['descriptor_loss_threshold']), float(config['positive_margin']),
        float(config['negative_margin']), float(config['lambda_d']), int(bool(config['descriptor_loss_use_mask'])),
        _lib.ptr(workspace), workspace.numel(), _lib.ptr(out), _lib.ptr(warped), _lib.stream_ptr(dev)))
    if keep is not None:
        keep.update(hom=hom, valid=valid, D=D)
    return out


class _LossFunction(torch.autograd.Function):
    """values = SuperPointLoss.evaluate(...) with the HIP backward.  Inputs: the loss module, its (pred, data, pred2,
    data2) and the four differentiable tensors logits1, logits2, desc1, desc2, already fp32 on the device (logits
    [B][65][Hc][Wc], descriptors channels-last [B][Hc][Wc][D]; None where unused).  The backward launches on torch's
    current stream and never synchronises with the host: the upstream coefficients stay on the device."""

    @staticmethod
    def forward(ctx, loss, args, logits1, logits2, desc1, desc2):
        pred, data, pred2, data2 = args
        p = [dict(pred), dict(pred2) if pred2 is not None else None]
        for side, (lg, d) in enumerate(((logits1, desc1), (logits2, desc2))):
            if p[side] is None:
                continue
            if lg is not None:
                p[side]['logits'] = lg
            if d is not None:
                p[side]['desc'] = d.permute(0, 3, 1, 2) if d.dim() == 4 else d
        state = {}
        values, _ = loss._evaluate(p[0], data, p[1], data2, state)
        ctx.state = state
        ctx.config = copy.deepcopy(loss.config)
        ctx.save_for_backward(logits1, logits2, desc1, desc2)      # the kernels' inputs: in-place edits are caught
        return values

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        st, cfg = ctx.state, ctx.config
        logits1, logits2, desc1, desc2 = ctx.saved_tensors
        logits = (logits1, logits2)
        dev, B, Hc, Wc = st['dev'], st['B'], st['Hc'], st['Wc']
        H, W = 8 * Hc, 8 * Wc
        at = {k: i + 1 for i, k in enumerate(st['keys'])}
        g = g.to(dev, torch.float64)
        h = _lib.get_handle(dev)
        stream = _lib.stream_ptr(dev)
        nbytes = ctypes.c_longlong()
        h.lib.mp_loss_workspace_bytes(B, H, W, ctypes.byref(nbytes))
        workspace = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        grads = [None, None, None, None]
        for side, det in enumerate(st['det']):
            if not ctx.needs_input_grad[2 + side]:
                continue
            coef = (g[0] + g[at['detector_loss%d' % (side + 1)]]).reshape(1)          # gamma_k
            grad = torch.empty((B, 65, Hc, Wc), dtype=torch.float32, device=dev)
            h.check(h.lib.mp_detector_loss_backward(
                h.ptr, _lib.ptr(logits[side]), B, Hc, Wc, _lib.ptr(det['kp']), _lib.ptr(det['valid']), H, W,
                int(det['use_ce']), _lib.ptr(det['noise']), det['seed'], _lib.ptr(det['out']), _lib.ptr(coef),
                _lib.ptr(workspace), workspace.numel(), _lib.ptr(grad), stream))
            grads[side] = grad
        desc = st['desc']
        if desc is not None and (ctx.needs_input_grad[4] or ctx.needs_input_grad[5]):
            base = float(cfg['lambda']) * g[0] + g[at['descriptor_loss']]
            coef = torch.stack([base + g[at['positive_dist']], base + g[at['negative_dist']]])     # alpha, beta
            # a side whose gradient is not needed is passed as NULL and not launched
            g1, g2 = [torch.empty((B, Hc, Wc, desc['D']), dtype=torch.float32, device=dev) if ctx.needs_input_grad[k]
                      else None for k in (4, 5)]
            hom, valid = desc['hom'], desc['valid']
            h.check(h.lib.mp_descriptor_loss_backward(
                h.ptr, _lib.ptr(desc1), _lib.ptr(desc2), B, Hc, Wc, desc['D'], _lib.ptr(hom[0]),
                _lib.ptr(hom[1]), _lib.ptr(valid[0]), _lib.ptr(valid[1]), H, W, float(cfg['descriptor_loss_threshold']),
                float(cfg['positive_margin']), float(cfg['negative_margin']), float(cfg['lambda_d']),
                int(bool(cfg['descriptor_loss_use_mask'])), _lib.ptr(desc['out']), _lib.ptr(coef), _lib.ptr(workspace),
                workspace.numel(), _lib.ptr(g1), _lib.ptr(g2), stream))
            grads[2], grads[3] = g1, g2
        return (None, None) + tuple(grads)
