"""TEST INFRASTRUCTURE ONLY (oracle side): weights and images on which every rounding point of the forward is exact.

Every activation of the network is a multiple of a power of two (1/8 in the encoder and the heads' 3x3 blocks, 2^-(3+k) behind the
heads' 1x1 layers) whose count (value / grid step) is bounded by 2048 in magnitude for ANY image of the grid, so fp16 holds it
exactly and no value is subnormal in fp16 or fp32:

  * images: integers 0..8 divided by 8 (one flat image per batch);
  * convolutions: per output channel one +1 tap and one or two -1 taps (two +1 and one -1 on most 3-tap filters; alternating
    signs where a narrow layer needs more taps per filter to be covered), zeros elsewhere, the taps placed round-robin over the seeds so that seeds 0..2 together put a nonzero weight on every (input channel, tap) of every
    layer; biases on the grid;
  * BatchNorm: running_var = 2^38, running_mean = 0, so 1/sqrt(var + 1e-5) is exactly 2^-19 in fp32 and fp64; gamma = s * 2^19
    with s in {+-1, +-2, 0} in EVERY BatchNorm (negative and zero scales everywhere), beta on the grid, chosen so that the next
    layer's input is >= 0;
  * interval arithmetic per channel through convolution, ReLU, BatchNorm and pooling bounds every count (activations by CAP).

The heads' last 1x1 layer and final BatchNorm scale by 2^-k to put the logits into a chosen range (`logit_spread`).  On these inputs
every multiply, sum (in any order), BatchNorm, ReLU, pool and fp16 rounding of the network is exact: a kernel that only multiplies
and adds (no Winograd transform) returns the float64 answer bit for bit.  tests/test_exact_fixture.py checks the premise on the
CPU; tests/test_gpu_exact.py holds the HIP kernels to it.

Only tests/ and tools/ import this file; the product path never does."""
import numpy as np
import torch
import torch.nn.functional as F

from . import mp_oracle as O

CAP = 768                  # bound of every activation count (<= 1024); a 3-tap convolution of it stays within 2 * 768 + 192 < 2048
LIMIT = 2048               # fp16 holds every integer count up to 2^11 exactly
SEEDS = (0, 1, 2)          # the seeds whose filters together cover every (input channel, tap)
INV_STD = 2.0 ** 19        # 1/sqrt(2^38 + 1e-5) == 2^-19 in fp32 and fp64
SPREADS = {'narrow': 30.0, 'wide': 256.0}      # bounds of |logit|: the wide case reaches about 200 on the test shapes

# every MultiPoint configuration the GPU tests run (tests/test_gpu_exact.py)
CONFIGS = {
    'shipped': {},
    'bn_first': {'bn_first': True},
    'zero_pad': {'reflection_pad': False},
    'multispectral': {'multispectral': True},
    'channel_v1': {'channel_version': 1},
    'channel_v2': {'channel_version': 2, 'descriptor_size': 128},
    'single_conv': {'double_convolution': False},
    'desc128': {'descriptor_size': 128},
    'desc256_no_final_bn': {'descriptor_size': 256, 'final_batchnorm': False},
    'raw_desc': {'normalize_descriptors': False},
    'no_desc_head': {'descriptor_head': False},
}


def config(name, **upd):
    cfg = dict(O.SHIPPED_MODEL_CONFIG)
    cfg.update(CONFIGS[name])
    cfg.update(upd)
    return cfg


def exact_images(seed, B, H, W, flat_last=True):
    """(B,1,H,W) fp32: integers 0..8 / 8; image B-1 of the batch is flat (constant) unless flat_last is false (a flat image cannot
    show where a kernel read or wrote: the other images are the same either way)."""
    rng = np.random.default_rng([int(seed), 4242])
    x = rng.integers(0, 9, size=(B, 1, H, W)).astype(np.float32)
    if flat_last:
        x[B - 1] = float(rng.integers(1, 9))
    return torch.from_numpy(x / 8.0)


# ------------------------------------------------------------------------------------------------------------------ weights
def n_taps(cin, cout, k):
    """Nonzero taps per filter: at least 2, and enough for len(SEEDS) seeds to cover all cin * k * k positions."""
    return max(2, -(-(cin * k * k) // (len(SEEDS) * cout)))


def input_cap(cin, cout, k):
    """The activation bound a layer of n_taps filters accepts: its most negative sum stays within LIMIT (up to three taps:
    two -1 taps and a bias of a quarter of the bound, or a bias that puts the sum of two +1 taps below the bound; more taps:
    their signs alternate and the bias puts the +1 taps below the bound)."""
    nt = n_taps(cin, cout, k)
    return CAP if nt <= 3 else min(CAP, LIMIT // nt)


class _Gen:
    """Draws one network's layers; bounds are integer counts (value * 8)."""

    def __init__(self, seed, spread):
        self.seed = int(seed)
        self.rng = np.random.default_rng([self.seed, 31337])
        self.spread = spread

    def taps(self, key, cout, cin, k):
        """[(co, [(ci, ky, kx, sign), ...])]: the nonzero taps of each filter, placed round-robin over the seeds."""
        P = cin * k * k
        nt = n_taps(cin, cout, k)
        perm = np.random.default_rng([sum(map(ord, key)), P, cout]).permutation(P)      # the same order for every seed
        start = (self.seed % len(SEEDS)) * cout * nt
        out = []
        for co in range(cout):
            pos = [int(perm[(start + co * nt + j) % P]) for j in range(nt)]
            if nt == 2 and self.rng.uniform() < 0.3 and P > 2:                          # a second -1 tap on some filters
                extra = int(perm[int(self.rng.integers(0, P))])
                if extra not in pos:
                    pos.append(extra)
            if len(pos) <= 3:
                signs = [1] + [-1] * (len(pos) - 1)
                if len(pos) == 3 and self.rng.uniform() < 0.7:
                    signs = [1, 1, -1]
            else:                                                                       # wide filters of narrow layers: alternate
                signs = [1 if j % 2 == 0 else -1 for j in range(len(pos))]
            out.append([(p // (k * k), (p % (k * k)) // k, p % k, s) for p, s in zip(pos, signs)])
        return out

    def conv(self, key, cout, hi_in, k, weight_shift=0, cap=CAP):
        """weight (cout,cin,k,k) with +-2^-weight_shift taps, bias, and the pre-activation interval [lo, up] in counts of
        2^-(3 + weight_shift)."""
        cin = len(hi_in)
        w = np.zeros((cout, cin, k, k))
        b = np.zeros(cout)
        lo, up = np.zeros(cout, dtype=np.int64), np.zeros(cout, dtype=np.int64)
        for co, taps in enumerate(self.taps(key, cout, cin, k)):
            hpos = sum(int(hi_in[ci]) for ci, _, _, s in taps if s > 0)
            hneg = sum(int(hi_in[ci]) for ci, _, _, s in taps if s < 0)
            for ci, ky, kx, s in taps:
                w[co, ci, ky, kx] = s * 2.0 ** -weight_shift
            top = max(hpos, 1)
            bhi = min(top // 8, cap - hpos)
            blo = min(-(top // 4), bhi)
            bc = int(self.rng.integers(blo, bhi + 1))
            b[co] = bc / 8.0 * 2.0 ** -weight_shift
            lo[co], up[co] = bc - hneg, bc + hpos
        assert max(np.abs(lo).max(), np.abs(up).max()) <= LIMIT, key
        return w, b, lo, up

    def scale(self, allow2):
        u = self.rng.uniform()
        s = 0 if u < 0.08 else (1 if u < 0.7 or not allow2 else 2)
        return s * (1 if self.rng.uniform() < 0.5 else -1)

    def bn_after_relu(self, up, cap=CAP):
        """ReLU -> BN (bn_first false): y = s * relu(z) + beta >= 0.  Returns gamma, beta (values) and the bound of y."""
        co = len(up)
        g, be, hi = np.zeros(co), np.zeros(co), np.zeros(co, dtype=np.int64)
        for c in range(co):
            R = max(int(up[c]), 0)
            R = min(R, cap)                  # (the conv's bias already bounds relu(z) by cap)
            s = self.scale(2 * R <= cap)
            if s < 0:
                beta = -s * R
            else:
                beta = int(self.rng.integers(1 if s == 0 else 0, max(1, min(R // 4, cap - s * R)) + 1))
            g[c], be[c], hi[c] = s * INV_STD, beta / 8.0, s * R + beta if s >= 0 else beta
        return g, be, hi

    def bn_then_relu(self, lo, up, cap=CAP):
        """BN -> ReLU (bn_first): y = relu(s * z + beta), beta near -s * (middle of the interval)."""
        co = len(up)
        g, be, hi = np.zeros(co), np.zeros(co), np.zeros(co, dtype=np.int64)
        for c in range(co):
            mid = (int(lo[c]) + int(up[c])) // 2
            half = (int(up[c]) - int(lo[c])) // 2 + 1
            s = self.scale(2 * half <= cap)
            if s == 0:
                beta = int(self.rng.integers(1, 9))
            else:
                vmax = max(s * int(lo[c]), s * int(up[c]))
                beta = min(-s * mid + int(self.rng.integers(-half // 4, half // 4 + 1)), cap - vmax)
            g[c], be[c], hi[c] = s * INV_STD, beta / 8.0, max(0, max(s * int(lo[c]), s * int(up[c])) + beta) if s else beta
        return g, be, hi

    def spread_shift(self, lo, up, target):
        """The k that puts max|z| * 2^-k at no more than `target` (value)."""
        m = max(np.abs(lo).max(), np.abs(up).max()) / 8.0
        k = 0
        while m * 2.0 ** -k > target:
            k += 1
        return k


def _bn_entries(sd, key, g, be):
    c = len(g)
    sd[key + '.weight'] = torch.tensor(g, dtype=torch.float32)
    sd[key + '.bias'] = torch.tensor(be, dtype=torch.float32)
    sd[key + '.running_mean'] = torch.zeros(c, dtype=torch.float32)
    sd[key + '.running_var'] = torch.full((c,), 2.0 ** 38, dtype=torch.float32)
    sd[key + '.num_batches_tracked'] = torch.tensor(0, dtype=torch.int64)


def _conv_entries(sd, key, w, b):
    sd[key + '.weight'] = torch.tensor(w, dtype=torch.float32)
    sd[key + '.bias'] = torch.tensor(b, dtype=torch.float32)


def exact_weights(seed, cfg=None, logit_spread='narrow', desc_spread=30.0):
    """Reference-layout state_dict for a MultiPoint config (see the module docstring).  logit_spread: 'narrow' (|logit| <= 30),
    'wide' (|logit| <= 256, about 200 reached) or a number."""
    cfg = O.full_config(cfg)
    spread = SPREADS.get(logit_spread, logit_spread)
    G = _Gen(seed, spread)
    sd = {}
    ch, head = O._channels(cfg)
    enc_names = ['encoder_thermal', 'encoder_optical'] if cfg['multispectral'] else ['encoder']
    enc_hi = np.zeros(ch[4], dtype=np.int64)
    layout = O.encoder_layout(cfg)
    consumers = [(l['cin'], l['cout'], 3) for l in layout[1:]] + [(ch[4], head, 3)]
    for name in enc_names:
        hi = np.array([8], dtype=np.int64)
        for l, nxt in zip(layout, consumers):
            key = '%s.%d' % (name, l['conv'])
            cap = input_cap(*nxt)
            w, b, lo, up = G.conv(key, l['cout'], hi, 3, cap=cap)
            _conv_entries(sd, key, w, b)
            g, be, hi = G.bn_then_relu(lo, up, cap) if cfg['bn_first'] else G.bn_after_relu(up, cap)
            _bn_entries(sd, '%s.%d' % (name, l['bn']), g, be)
        enc_hi = np.maximum(enc_hi, hi)
    heads = [('detector_head_convolutions', 65, spread)]
    if cfg['descriptor_head']:
        heads.append(('descriptor_head_convolutions', cfg['descriptor_size'], desc_spread))
    bn_i = 2 if cfg['bn_first'] else 3
    for name, nout, target in heads:
        cap = input_cap(head, nout, 1)
        w, b, lo, up = G.conv(name + '.1', head, enc_hi, 3, cap=cap)
        _conv_entries(sd, name + '.1', w, b)
        g, be, hi = G.bn_then_relu(lo, up, cap) if cfg['bn_first'] else G.bn_after_relu(up, cap)
        _bn_entries(sd, '%s.%d' % (name, bn_i), g, be)
        # the last 1x1 layer: first with unit taps to learn the range, then scaled so that |output| <= target
        state = G.rng.bit_generator.state
        _, _, lo1, up1 = G.conv(name + '.4', nout, hi, 1)
        k = G.spread_shift(lo1, up1, target)
        G.rng.bit_generator.state = state
        if cfg['final_batchnorm']:
            w, b, lo1, up1 = G.conv(name + '.4', nout, hi, 1)
            _conv_entries(sd, name + '.4', w, b)
            # final BN: s = +-2^-k (never 0 on the detector: a constant logit row would make the dustbin trivial), beta on 2^-(3+k)
            s = np.where(G.rng.uniform(size=nout) < 0.5, -1.0, 1.0) * 2.0 ** -k
            if not name.startswith('detector'):
                s[G.rng.uniform(size=nout) < 0.08] = 0.0
            beta = G.rng.integers(-32, 33, size=nout) / 8.0 * 2.0 ** -k
            _bn_entries(sd, name + '.5', s * INV_STD, beta)
        else:
            w, b, _, _ = G.conv(name + '.4', nout, hi, 1, weight_shift=k)
            _conv_entries(sd, name + '.4', w, b)
    spec = O.state_dict_spec(cfg)
    assert [k for k, _, _ in spec] == sorted(sd, key=[k for k, _, _ in spec].index) and len(sd) == len(spec)
    return {k: sd[k] for k, _, _ in spec}


def exact_weights_magicleap(seed, logit_spread='narrow'):
    """SuperPointMagicLeap state_dict (zero padding, ReLU, no BatchNorm) on the same grid."""
    spread = SPREADS.get(logit_spread, logit_spread)
    G = _Gen(seed, spread)
    sd = {}
    his = {'image': np.array([8], dtype=np.int64)}
    src = {'conv1a': 'image', 'conv1b': 'conv1a', 'conv2a': 'conv1b', 'conv2b': 'conv2a', 'conv3a': 'conv2b', 'conv3b': 'conv3a',
           'conv4a': 'conv3b', 'conv4b': 'conv4a', 'convPa': 'conv4b', 'convPb': 'convPa', 'convDa': 'conv4b', 'convDb': 'convDa'}
    for name, co, ci, k in O.MAGICLEAP_LAYERS:
        hi = his[src[name]]
        if name in ('convPb', 'convDb'):
            state = G.rng.bit_generator.state
            _, _, lo1, up1 = G.conv(name, co, hi, 1)
            sh = G.spread_shift(lo1, up1, spread if name == 'convPb' else 30.0)
            G.rng.bit_generator.state = state
            w, b, _, _ = G.conv(name, co, hi, 1, weight_shift=sh)
        else:
            w, b, lo, up = G.conv(name, co, hi, k)
            his[name] = np.maximum(up, 0)                   # ReLU
        _conv_entries(sd, name, w, b)
    return sd


# ------------------------------------------------------------------------------------------------------------------ evaluation
def forward64(sd, img, cfg=None, is_optical=None, return_logits=False):
    """The oracle on double tensors."""
    sd64 = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in sd.items()}
    return O.forward(sd64, img.double(), cfg, is_optical=is_optical, return_logits=return_logits)


def magicleap64(sd, img):
    sd64 = {k: v.double() for k, v in sd.items()}
    return O.forward_magicleap(sd64, img.double())


MUTATIONS = ('corner', 'drop16', 'last_row', 'pool_preact_max', 'last_col', 'block_edge')


def default_block_edge(h, w):
    """Where 'block_edge' lands in an h x w block output when the caller names no place: the first pixel of the last block of
    16 rows x 32 columns (an F(4x4,3x3) item of 4 x 8 tiles)."""
    return (h - 1) // 16 * 16, (w - 1) // 32 * 32


def layer_outputs(sd, img, cfg=None, mixed=None, dtype=torch.float32, mutate=None, encoder_name='encoder'):
    """[(name, output)] of every encoder block (after its pool), the heads' 3x3 blocks, the logits and the raw descriptors, in the
    oracle's arithmetic (fp16 restatement when `mixed`).  mutate = (layer name, mutation) injects one of MUTATIONS into that block,
    the way a kernel bug would: +1/8 at the bottom-right pixel of every channel ('corner'), the last 16 input channels ignored
    ('drop16'), the last output row a copy of the row above ('last_row'), max-pooling BEFORE the activation for every channel
    ('pool_preact_max', the wrong order for negative BatchNorm scales), the last output column a copy of the column to its left
    ('last_col'), +1/8 at ONE pixel of every channel ('block_edge': mutate = (layer, 'block_edge', (y, x)) in the block's output
    frame, the first pixel of a tile block of the launch that computes it; default_block_edge() without a place)."""
    cfg = O.full_config(cfg)
    if mixed is not None:
        cfg['mixed_precision'] = bool(mixed)
    f16 = bool(cfg.get('mixed_precision'))
    rnd = O._h if f16 else (lambda t: t)
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    x = img.to(dtype)
    if f16:
        x = O._h(x)
    outs = []

    def block(x, name, conv_key, bn_key, pool, k3=True):
        mut = mutate[1] if mutate is not None and mutate[0] == name else None
        if mut == 'drop16':
            x = x.clone(); x[:, -min(16, x.shape[1]):] = 0
        w, b = sd[conv_key + '.weight'], sd[conv_key + '.bias']
        xin = O._pad(x, cfg) if k3 else x
        z = rnd(F.conv2d(xin, rnd(w), rnd(b)))

        def act(z):
            if cfg['bn_first']:
                return F.relu(rnd(O._bn_eval(z, sd, bn_key)))
            return rnd(O._bn_eval(F.relu(z), sd, bn_key))
        if pool and mut == 'pool_preact_max':
            y = act(F.max_pool2d(z, 2, 2))
        else:
            y = act(z)
            if pool:
                y = F.max_pool2d(y, 2, 2)
        if mut == 'corner':
            y = y.clone(); y[:, :, -1, -1] += 0.125
        elif mut == 'last_row':
            y = y.clone(); y[:, :, -1, :] = y[:, :, -2, :]
        elif mut == 'last_col':
            y = y.clone(); y[:, :, :, -1] = y[:, :, :, -2]
        elif mut == 'block_edge':
            at = mutate[2] if len(mutate) > 2 else default_block_edge(y.shape[2], y.shape[3])
            y = y.clone(); y[:, :, at[0], at[1]] += 0.125
        return y

    with torch.no_grad():
        for l in O.encoder_layout(cfg):
            name = '%s.%d' % (encoder_name, l['conv'])
            x = block(x, name, name, '%s.%d' % (encoder_name, l['bn']), l['pool'])
            outs.append((name, x))
        bn_i = 2 if cfg['bn_first'] else 3
        heads = ['detector_head_convolutions'] + (['descriptor_head_convolutions'] if cfg['descriptor_head'] else [])
        for hname in heads:
            h = block(x, hname + '.1', hname + '.1', '%s.%d' % (hname, bn_i), False)
            outs.append((hname + '.1', h))
            h = rnd(F.conv2d(h, rnd(sd[hname + '.4.weight']), rnd(sd[hname + '.4.bias'])))
            if cfg['final_batchnorm']:
                h = rnd(O._bn_eval(h, sd, hname + '.5'))
            outs.append(('logits' if hname.startswith('detector') else 'desc_raw', h))
    return outs


def final_outputs(sd, img, cfg=None, **kw):
    """{'logits', 'desc_raw'} of layer_outputs (single-encoder configs)."""
    return {k: v for k, v in layer_outputs(sd, img, cfg, **kw) if k in ('logits', 'desc_raw')}


def truth(sd, img, cfg, is_optical=None, fp32=False):
    """Exact logits and raw descriptors (returned in fp32: every value is an fp32 number), and prob / normalised descriptors as
    float64 functions of them.  fp32=True evaluates the oracle in fp32 (several times faster at large shapes), which
    tests/test_exact_fixture.py shows to be the float64 answer bit for bit on these inputs."""
    c = dict(O.full_config(cfg)); c['mixed_precision'] = False
    raw = dict(c); raw['normalize_descriptors'] = False
    if fp32:
        r = O.forward(sd, img, raw, is_optical=is_optical, return_logits=True)
    else:
        r = forward64(sd, img, raw, is_optical=is_optical, return_logits=True)
    out = {'logits': r['logits'], 'prob': prob64(r['logits'])}
    if c['descriptor_head']:
        out['desc_raw'] = r['desc']
        out['desc'] = normalize64(r['desc'])
    for k in ('logits', 'desc_raw'):
        if k in out:
            f = out[k].float()
            assert torch.equal(f.double(), out[k].double()), k
            out[k] = f
    return out


def prob64(logits):
    return O.depth_to_space(torch.softmax(logits.double(), dim=1)[:, :-1], 8)


def normalize64(d):
    return F.normalize(d.double(), p=2, dim=1)
