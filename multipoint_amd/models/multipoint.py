"""Host-side mirror of the reference model class (multipoint/models/MultiPoint.py:8-185) for
inference: same constructor config, same state_dict key layout, same forward dict-in/dict-out
contract -- computed by hand-written gfx950 kernels behind libmultipoint_hip.so."""
import collections
import copy
import ctypes

import numpy as np
import torch

from .. import _lib
from ..utils.utils import dict_update


class MultiPoint:
    # multipoint/models/MultiPoint.py:9-23
    default_config = {
        'multispectral': True,
        'descriptor_head': True,
        'intepolation_mode': 'bilinear',
        'descriptor_size': 256,
        'normalize_descriptors': True,
        'final_batchnorm': True,
        'reflection_pad': True,
        'bn_first': False,
        'double_convolution': True,
        'channel_version': 0,
        'verbose': False,
        'mixed_precision': False,
        'force_return_logits': False
    }
    # multipoint_amd only (no reference counterpart, hence not in default_config): optional key model.conv_algorithm, the algorithm of
    # the 3x3 convolutions -- 'auto' | 'winograd43' | 'winograd43_general' | 'direct' (include/multipoint_hip.h:
    # mp_model_config.conv_algorithm)
    CONV_ALGORITHMS = {'auto': 0, 'winograd43': 1, 'winograd43_general': 2, 'direct': 3}
    # ... and optional key model.batch_invariant (bool, default False): forwards of one or two images skip the split small launches
    # of the single-pair latency path, so that their bits equal those of the same images inside a larger batch
    # (mp_model_config.batch_invariant)

    def __init__(self, config=None):
        if config:
            self.config = dict_update(copy.deepcopy(self.default_config), config)
        else:
            self.config = copy.deepcopy(self.default_config)
        if self.config['channel_version'] not in (0, 1, 2):
            raise ValueError('channel_version must be 0, 1 or 2 (MultiPoint.py:38-53)')
        if self.config.get('conv_algorithm', 'auto') not in self.CONV_ALGORITHMS:
            raise ValueError('conv_algorithm must be one of %s' % ', '.join(self.CONV_ALGORITHMS))
        self.training = False
        self.device = None
        self._handle = None
        self._state = None           # OrderedDict name -> CPU tensor (reference state_dict layout)
        self._uploaded = False
        self._fwd_event = None       # last forward's completion, for callers that alternate streams
        self._fwd_stream = None
        self._batch_statistics = False   # set_batch_statistics: the training-mode forward (BatchNorm with batch statistics)
        self._bn_layout = None           # [(state_dict prefix, channels)] of the uploaded model's BatchNorm layers
        self._last_stats = None          # (device fp32 statistics array, names of the layers the last such forward wrote)
        if self.config['verbose']:
            n = sum(int(np.prod(s)) for k, s, d in self.state_dict_spec() if d == torch.float32
                    and not k.endswith(('running_mean', 'running_var')))
            print('MultiPoint number of trainable parameter: ' + str(n))

    # -- state_dict layout (train.py:161-173 saves net.state_dict()) ------------------------------
    def state_dict_spec(self):
        """Ordered (key, shape, dtype) of the reference nn.Module's state_dict for this config
        (nn.Sequential indices of generate_encoder, MultiPoint.py:168-185, and the two heads,
        :62-88)."""
        c = self.config
        spec = []

        def conv(p, co, ci, k):
            spec.append((p + '.weight', (co, ci, k, k), torch.float32))
            spec.append((p + '.bias', (co,), torch.float32))

        def bn(p, ch):
            for leaf in ('weight', 'bias', 'running_mean', 'running_var'):
                spec.append(('%s.%s' % (p, leaf), (ch,), torch.float32))
            spec.append((p + '.num_batches_tracked', (), torch.int64))

        # MultiPoint.py:38-53
        stage = {0: [1, 64, 64, 128, 128], 1: [1, 32, 64, 96, 128], 2: [1, 8, 16, 32, 64]}[c['channel_version']]
        head_channels = 256 if c['channel_version'] == 0 else c['descriptor_size']
        if c['double_convolution']:
            chan = [1, stage[1], stage[1], stage[2], stage[2], stage[3], stage[3], stage[4], stage[4]]
            conv_idx = [1, 5, 10, 14, 19, 23, 28, 32]
        else:       # getConvolutionBlock (MultiPoint.py:147-148): one (pad, conv, X, Y) group per stage, a pool after stages 1-3
            chan = list(stage)
            conv_idx = [1, 6, 11, 16]
        bn_off = 1 if c['bn_first'] else 2
        names = ['encoder_thermal', 'encoder_optical'] if c['multispectral'] else ['encoder']
        for name in names:
            for i, ci in enumerate(conv_idx):
                conv('%s.%d' % (name, ci), chan[i + 1], chan[i], 3)
                bn('%s.%d' % (name, ci + bn_off), chan[i + 1])
        heads = [('detector_head_convolutions', 65)]
        if c['descriptor_head']:
            heads.append(('descriptor_head_convolutions', c['descriptor_size']))
        for name, nout in heads:
            conv(name + '.1', head_channels, stage[4], 3)
            bn('%s.%d' % (name, 1 + bn_off), head_channels)
            conv(name + '.4', nout, head_channels, 1)
            if c['final_batchnorm']:
                bn(name + '.5', nout)
        return spec

    def load_state_dict(self, state_dict, strict=True):
        """nn.Module.load_state_dict semantics (strict by default), predict_align_image_pair.py:58-61."""
        spec = self.state_dict_spec()
        expected = collections.OrderedDict((k, (s, d)) for k, s, d in spec)
        missing = [k for k in expected if k not in state_dict]
        unexpected = [k for k in state_dict if k not in expected]
        errors = []
        if strict and missing:
            errors.append('Missing key(s) in state_dict: %s.' % ', '.join('"%s"' % k for k in missing))
        if strict and unexpected:
            errors.append('Unexpected key(s) in state_dict: %s.' % ', '.join('"%s"' % k for k in unexpected))
        new_state = collections.OrderedDict() if self._state is None else collections.OrderedDict(self._state)
        for k, (shape, dtype) in expected.items():
            if k not in state_dict:
                continue
            v = state_dict[k]
            if not torch.is_tensor(v):
                v = torch.as_tensor(v)
            if tuple(v.shape) != tuple(shape):
                errors.append('size mismatch for %s: copying a param with shape %s from checkpoint, '
                              'the shape in current model is %s.' % (k, tuple(v.shape), tuple(shape)))
                continue
            new_state[k] = v.detach().to('cpu', dtype).contiguous().clone()
        if errors:
            raise RuntimeError('Error(s) in loading state_dict for %s:\n\t' % type(self).__name__ + '\n\t'.join(errors))
        if strict or all(k in new_state for k in expected):
            self._state = collections.OrderedDict((k, new_state[k]) for k in expected)
            self._uploaded = False
            if self.device is not None:
                self._upload()
        return missing, unexpected

    def state_dict(self):
        if self._state is None:
            raise RuntimeError('MultiPoint has no weights: call load_state_dict() or init_random_weights()')
        return collections.OrderedDict((k, v.clone()) for k, v in self._state.items())

    def init_random_weights(self, seed=0):
        """Stand-in for nn.Module's default initialisation when the CLI runs with `-v none`
        (predict_align_image_pair.py:23,58): Kaiming-uniform convs, identity BatchNorm."""
        rng = np.random.default_rng(seed)
        sd = collections.OrderedDict()
        bounds = {}
        for k, shape, dtype in self.state_dict_spec():
            prefix, leaf = k.rsplit('.', 1)
            if dtype == torch.int64:
                sd[k] = torch.zeros((), dtype=torch.int64)
            elif len(shape) == 4:
                bounds[prefix] = 1.0 / np.sqrt(shape[1] * shape[2] * shape[3])
                sd[k] = torch.from_numpy(rng.uniform(-bounds[prefix], bounds[prefix], shape).astype(np.float32))
            elif leaf == 'bias' and prefix in bounds:
                sd[k] = torch.from_numpy(rng.uniform(-bounds[prefix], bounds[prefix], shape).astype(np.float32))
            elif leaf in ('running_var', 'weight'):
                sd[k] = torch.ones(shape)
            else:
                sd[k] = torch.zeros(shape)
        self.load_state_dict(sd)
        return self

    # -- nn.Module-like plumbing ------------------------------------------------------------------
    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError('multipoint_amd implements the inference path only (eval mode)')
        return self.eval()

    def to(self, device):
        device = _lib.require_cuda(device)
        if self.device != device or self._handle is None:
            self.device = device
            self._handle = _lib.Handle(device.index)
            self._uploaded = False
        if self._state is not None and not self._uploaded:
            self._upload()
        return self

    def direct_twin(self):
        """A second model over the SAME weights with `conv_algorithm: direct` (created on first use, on this model's device) --
        the tie-exact algorithm the top-k tie guard re-evaluates flagged images with (utils.tie_robust_redo).  None when this
        model has no other algorithm to offer: it is `direct` itself, or runs the fp16 path (`mixed_precision`)."""
        if self.config.get('conv_algorithm', 'auto') == 'direct' or self.config.get('mixed_precision') or self._state is None \
                or self.device is None:
            return None
        twin = getattr(self, '_direct_twin', None)
        if twin is None or twin._state_of is not self._state or twin.device != self.device:
            cfg = dict(self.config); cfg['conv_algorithm'] = 'direct'
            twin = type(self)(cfg)
            twin._state = self._state                    # shared host tensors (read-only)
            twin._state_of = self._state
            twin._uploaded = False
            twin.to(self.device)
            twin.eval()
            self._direct_twin = twin
        return twin

    def cuda(self, device=None):
        return self.to(torch.device('cuda', torch.cuda.current_device() if device is None else device))

    def set_force_return_logits(self, value):
        # MultiPoint.py:93-97
        if not isinstance(value, bool):
            raise ValueError('set_force_return_logits: The input value needs to be a bool')
        self.config['force_return_logits'] = value

    def set_batch_statistics(self, value):
        """True: `forward` runs the reference's TRAINING-mode forward (train.py never calls net.eval(), so its validation loop
        runs this): every BatchNorm normalises with the statistics of the batch, and the result is the reference's
        {'prob': None, 'logits': (B,65,Hc,Wc), 'desc': (B,D,Hc,Wc)}.  Forward only: `training` stays False, train() still
        raises, and the running statistics are not updated (last_batch_statistics() returns what torch would blend into them).
        fp32 models with BatchNorm only."""
        if not isinstance(value, bool):
            raise ValueError('set_batch_statistics: The input value needs to be a bool')
        self._batch_statistics = value

    def batch_statistics_layout(self):
        """[(state_dict prefix, channels)] of the model's BatchNorm layers, state_dict order (mp_batch_stats_layer)."""
        if self._bn_layout is None:
            h = self._handle
            if h is None or not self._uploaded:
                raise RuntimeError('MultiPoint: move the model to the GPU with weights loaded first')
            n = ctypes.c_int(0)
            h.check(h.lib.mp_batch_stats_count(h.ptr, ctypes.byref(n)))
            layout = []
            for i in range(n.value):
                name, ch = ctypes.c_char_p(), ctypes.c_int(0)
                h.check(h.lib.mp_batch_stats_layer(h.ptr, i, ctypes.byref(name), ctypes.byref(ch)))
                layout.append((name.value.decode(), ch.value))
            self._bn_layout = layout
        return self._bn_layout

    def last_batch_statistics(self):
        """{state_dict prefix: (mean, unbiased variance)} of the BatchNorm layers in the last batch-statistics forward, as
        device tensors -- what torch blends into running_mean / running_var (momentum 0.1).  A multispectral encoder that
        received no images has no entry.  The model's running statistics are not modified."""
        if self._last_stats is None:
            raise RuntimeError('last_batch_statistics: no forward with set_batch_statistics(True) has run yet')
        buf, written = self._last_stats
        out = collections.OrderedDict()
        off = 0
        for name, ch in self.batch_statistics_layout():
            if name in written:
                out[name] = (buf[off:off + ch], buf[off + ch:off + 2 * ch])
            off += 2 * ch
        return out

    def _check_batch_statistics(self, B, H, W, is_opt):
        """The refusals of mp_forward_batch_stats, raised before any launch."""
        if self.config['mixed_precision']:
            raise NotImplementedError('set_batch_statistics: BatchNorm with batch statistics runs on the fp32 path only '
                                      '(mixed_precision models are not supported)')
        if not self._abi_extra['batchnorm']:
            raise NotImplementedError('set_batch_statistics: %s has no BatchNorm layers' % type(self).__name__)
        counts = [B]
        if is_opt is not None:
            n_opt = int(is_opt.sum())
            counts = [n for n in (n_opt, B - n_opt) if n > 0]
        n = min(counts) * (H // 8) * (W // 8)
        if n <= 1:
            raise ValueError('Expected more than 1 value per channel when training, got input size [%d, %d, 1, 1]'
                             % (min(counts), self.config['descriptor_size'] if self.config['final_batchnorm'] and
                                self.config['descriptor_head'] else 65))

    def _encoder_prefixes(self, is_opt, B):
        """State_dict prefixes of the encoders a forward runs."""
        if not self.config['multispectral']:
            return ('encoder.',)
        n_opt = int(is_opt.sum())
        return tuple(p for p, n in (('encoder_thermal.', B - n_opt), ('encoder_optical.', n_opt)) if n > 0)

    # extra mp_model_config fields of this model class (include/multipoint_hip.h)
    _abi_extra = {'batchnorm': 1, 'key_layout': 0, 'softmax_mode': 0}

    def _upload(self):
        c = self.config
        vals = [int(c[k]) if k in ('descriptor_size', 'channel_version') else int(bool(c[k]))
                for k in ('multispectral', 'descriptor_head', 'descriptor_size', 'normalize_descriptors',
                          'final_batchnorm', 'reflection_pad', 'bn_first', 'double_convolution', 'channel_version')]
        vals += [self._abi_extra['batchnorm'], self._abi_extra['key_layout'], self._abi_extra['softmax_mode'],
                 int(bool(c['mixed_precision'])),      # MultiPoint.py:99-103: forward under autocast -> fp16 MFMA path
                 self.CONV_ALGORITHMS[c.get('conv_algorithm', 'auto')], int(bool(c.get('batch_invariant', False)))]
        cfg = _lib.ModelConfig(*vals)
        keep = []
        arr = []
        for k, v in self._state.items():
            if v.dtype != torch.float32:
                continue                       # num_batches_tracked counters are not used in eval mode
            keep.append(v)
            arr.append(_lib.Tensor(k.encode(), ctypes.c_void_p(v.data_ptr()), v.numel()))
        tens = (_lib.Tensor * len(arr))(*arr)
        h = self._handle
        h.check(h.lib.mp_load_weights(h.ptr, ctypes.byref(cfg), tens, len(arr)))
        self._uploaded = True
        self._bn_layout = None
        self._last_stats = None

    # -- forward (MultiPoint.py:99-135) -----------------------------------------------------------
    def forward(self, data):
        if self._state is None:
            raise RuntimeError('MultiPoint has no weights: call load_state_dict() or init_random_weights()')
        if self.training:
            raise NotImplementedError('multipoint_amd implements the inference path only (eval mode)')
        image = data['image']
        if self.device is None:
            self.to(image.device)
        if image.device != self.device:
            raise RuntimeError('input image is on %s but the model is on %s' % (image.device, self.device))
        if image.dim() != 4 or image.shape[1] != 1:
            raise ValueError('image must have shape (B,1,H,W), got %s' % (tuple(image.shape),))
        image = image.to(torch.float32).contiguous()
        B, _, H, W = image.shape
        is_opt = None
        if self.config['multispectral']:
            flags = data['is_optical'][:, 0].to('cpu', torch.uint8).contiguous()
            is_opt = flags
        Hc, Wc = H // 8, W // 8
        if self._batch_statistics:
            self._check_batch_statistics(B, H, W, is_opt)
            return self._forward_batch_statistics(image, is_opt, B, H, W)
        want_logits = bool(self.config['force_return_logits'])
        prob = None if want_logits else torch.empty((B, 1, H, W), dtype=torch.float32, device=self.device)
        logits = torch.empty((B, 65, Hc, Wc), dtype=torch.float32, device=self.device) if want_logits else None
        desc_cl = None
        if self.config['descriptor_head']:
            D = self.config['descriptor_size']
            desc_cl = torch.empty((B, Hc, Wc, D), dtype=torch.float32, device=self.device)
        h = self._handle
        # one workspace per handle: a forward on ANOTHER stream than the previous one is ordered behind it (same stream: in order anyway)
        cur = torch.cuda.current_stream(self.device)
        if self._fwd_event is not None and self._fwd_stream != cur:
            cur.wait_event(self._fwd_event)
        with torch.cuda.device(self.device):
            h.check(h.lib.mp_forward(h.ptr, _lib.ptr(image),
                                     ctypes.c_void_p(is_opt.data_ptr()) if is_opt is not None else None,
                                     B, H, W, _lib.ptr(prob), _lib.ptr(logits), _lib.ptr(desc_cl),
                                     _lib.stream_ptr(self.device)))
        if self._fwd_stream != cur:                  # (the event is only needed across a change of stream: record on change)
            self._fwd_event = torch.cuda.Event()
        if self._fwd_event is not None:
            self._fwd_event.record(cur)
        self._fwd_stream = cur
        out = {'prob': prob, 'logits': logits}
        if desc_cl is not None:
            # logically (B,D,Hc,Wc) like the reference, stored channels-last (values identical)
            out['desc'] = desc_cl.permute(0, 3, 1, 2)
        return out

    __call__ = forward

    def _forward_batch_statistics(self, image, is_opt, B, H, W):
        Hc, Wc = H // 8, W // 8
        logits = torch.empty((B, 65, Hc, Wc), dtype=torch.float32, device=self.device)
        desc_cl = None
        if self.config['descriptor_head']:
            desc_cl = torch.empty((B, Hc, Wc, self.config['descriptor_size']), dtype=torch.float32, device=self.device)
        layout = self.batch_statistics_layout()
        stats = torch.empty((2 * sum(ch for _, ch in layout),), dtype=torch.float32, device=self.device)
        h = self._handle
        cur = torch.cuda.current_stream(self.device)
        if self._fwd_event is not None and self._fwd_stream != cur:
            cur.wait_event(self._fwd_event)
        with torch.cuda.device(self.device):
            h.check(h.lib.mp_forward_batch_stats(h.ptr, _lib.ptr(image),
                                                 ctypes.c_void_p(is_opt.data_ptr()) if is_opt is not None else None,
                                                 B, H, W, _lib.ptr(logits), _lib.ptr(desc_cl), _lib.ptr(stats),
                                                 _lib.stream_ptr(self.device)))
        if self._fwd_stream != cur:
            self._fwd_event = torch.cuda.Event()
        if self._fwd_event is not None:
            self._fwd_event.record(cur)
        self._fwd_stream = cur
        ran = self._encoder_prefixes(is_opt, B)
        self._last_stats = (stats, frozenset(n for n, _ in layout if not n.startswith('encoder') or
                                             any(n.startswith(p) for p in ran)))
        out = {'prob': None, 'logits': logits}
        if desc_cl is not None:
            out['desc'] = desc_cl.permute(0, 3, 1, 2)
        return out

    # profiling hook used by bench.py (per-launch hipEvent timing)
    def profile(self, enable=True):
        h = self._handle
        h.check(h.lib.mp_profile_enable(h.ptr, 1 if enable else 0))

    def profile_read(self):
        h = self._handle
        cap = 4096
        names = (ctypes.c_char_p * cap)()
        ms = (ctypes.c_float * cap)()
        flop = (ctypes.c_double * cap)()
        n = ctypes.c_int(0)
        h.check(h.lib.mp_profile_read(h.ptr, names, ms, flop, cap, ctypes.byref(n)))
        return [(names[i].decode(), float(ms[i]), float(flop[i])) for i in range(n.value)]
