"""The cases of tests/golden/batch_statistics.npz and a float64 restatement of MultiPoint's TRAINING-mode forward
(multipoint/models/MultiPoint.py:99-185 without net.eval(): every BatchNorm2d normalises with the mean and biased variance of
the batch, and blends the batch mean / unbiased variance into its running statistics with momentum 0.1).  Written from the
module structure with F.conv2d / F.batch_norm(training=True), independent of the reference code and of the product."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

from oracle import mp_oracle as O

# (name, model config overrides of the shipped params.yaml, B, H, W, is_optical or None)
CASES = [
    ('shipped', {}, 3, 24, 32, None),
    ('bn_first', {'bn_first': True}, 3, 24, 32, None),
    ('no_final_bn', {'final_batchnorm': False}, 3, 24, 32, None),
    ('single_conv', {'double_convolution': False}, 3, 24, 32, None),
    ('channel_v1', {'channel_version': 1, 'descriptor_size': 128}, 2, 24, 32, None),
    ('channel_v2', {'channel_version': 2}, 3, 24, 32, None),
    ('zero_pad', {'reflection_pad': False}, 3, 24, 32, None),
    ('d128', {'descriptor_size': 128}, 2, 24, 32, None),
    ('d256', {'descriptor_size': 256}, 2, 24, 32, None),
    ('bn_first_v2_zero', {'bn_first': True, 'channel_version': 2, 'reflection_pad': False}, 3, 24, 32, None),
    ('ms_mixed', {'multispectral': True}, 4, 24, 32, [1, 0, 0, 1]),
    ('ms_all_optical', {'multispectral': True}, 3, 24, 32, [1, 1, 1]),
]
MOMENTUM = 0.1
EPS = 1e-5


def case_config(case):
    return dict(O.SHIPPED_MODEL_CONFIG, **case[1])


def case_weights(case, seed):
    """Trained-like weights with running statistics that differ clearly from any batch's, and gammas of both signs (the 2x2
    pool follows the affine)."""
    cfg = case_config(case)
    sd = O.make_weights(seed, cfg)
    rng = np.random.default_rng([seed, 7])
    for k in list(sd):
        if k.endswith('.running_mean'):
            p = k[:-len('.running_mean')]
            n = sd[k].numel()
            sd[k] = torch.from_numpy(rng.normal(0.0, 2.0, n).astype(np.float32))
            sd[p + '.running_var'] = torch.from_numpy(rng.uniform(0.2, 5.0, n).astype(np.float32))
            g = rng.uniform(0.5, 2.0, n) * np.where(rng.uniform(size=n) < 0.2, -1.0, 1.0)
            sd[p + '.weight'] = torch.from_numpy(g.astype(np.float32))
            sd[p + '.bias'] = torch.from_numpy(rng.normal(0.0, 0.5, n).astype(np.float32))
    return sd


def case_inputs(case, seed):
    B, H, W = case[2], case[3], case[4]
    img = O.make_images(seed, B, H, W)
    opt = None if case[5] is None else torch.tensor(case[5], dtype=torch.bool).reshape(B, 1)
    return img, opt


def bn_prefixes(cfg):
    """State_dict prefixes of the BatchNorm layers, state_dict order."""
    return [k[:-len('.running_mean')] for k, _, _ in O.state_dict_spec(O.full_config(cfg)) if k.endswith('.running_mean')]


def forward_train64(sd, image, cfg, is_optical=None):
    """float64 training-mode forward: (logits (B,65,Hc,Wc), desc (B,D,Hc,Wc) or None, {prefix: (batch mean, unbiased var)})."""
    cfg = O.full_config(cfg)
    sd = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in sd.items()}
    stats = collections.OrderedDict()

    def pad(x):
        return F.pad(x, (1, 1, 1, 1), mode='reflect' if cfg['reflection_pad'] else 'constant')

    def bn(x, p):
        n = x.shape[0] * x.shape[2] * x.shape[3]
        mean = x.mean(dim=(0, 2, 3))
        var = x.var(dim=(0, 2, 3), unbiased=False)
        stats[p] = (mean, var * n / (n - 1))
        return F.batch_norm(x, None, None, sd[p + '.weight'], sd[p + '.bias'], training=True, eps=EPS)

    def nonlin(x, p):
        return F.relu(bn(x, p)) if cfg['bn_first'] else bn(F.relu(x), p)

    bn_off = 1 if cfg['bn_first'] else 2

    def encoder(x, name):
        for i, (ci, pool) in enumerate(zip(*encoder_layout(cfg))):
            x = F.conv2d(pad(x), sd['%s.%d.weight' % (name, ci)], sd['%s.%d.bias' % (name, ci)])
            x = nonlin(x, '%s.%d' % (name, ci + bn_off))
            if pool:
                x = F.max_pool2d(x, 2, 2)
        return x

    img = image.double()
    if cfg['multispectral']:
        opt = is_optical[:, 0]
        c4 = {0: 128, 1: 128, 2: 64}[cfg['channel_version']]
        x = torch.zeros((img.shape[0], c4, img.shape[2] // 8, img.shape[3] // 8), dtype=torch.float64)
        # state_dict order: encoder_thermal's layers, then encoder_optical's (the statistics dict keeps that order)
        if (~opt).any():
            x[~opt] = encoder(img[~opt], 'encoder_thermal')
        if opt.any():
            x[opt] = encoder(img[opt], 'encoder_optical')
    else:
        x = encoder(img, 'encoder')

    def head(x, name):
        y = nonlin(F.conv2d(pad(x), sd[name + '.1.weight'], sd[name + '.1.bias']), '%s.%d' % (name, 1 + bn_off))
        y = F.conv2d(y, sd[name + '.4.weight'], sd[name + '.4.bias'])
        if cfg['final_batchnorm']:
            y = bn(y, name + '.5')
        return y

    logits = head(x, 'detector_head_convolutions')
    desc = None
    if cfg['descriptor_head']:
        desc = head(x, 'descriptor_head_convolutions')
        if cfg['normalize_descriptors']:
            desc = F.normalize(desc, p=2, dim=1)
    order = bn_prefixes(cfg)
    stats = collections.OrderedDict((p, stats[p]) for p in order if p in stats)
    return logits, desc, stats


def encoder_layout(cfg):
    """(conv Sequential indices, MaxPool2d after the block?) of generate_encoder (MultiPoint.py:168-185)."""
    if cfg['double_convolution']:
        return [1, 5, 10, 14, 19, 23, 28, 32], [False, True, False, True, False, True, False, False]
    return [1, 6, 11, 16], [True, True, True, False]


def blend_running(sd, stats):
    """torch's running-statistics update: (1 - momentum) old + momentum batch."""
    out = {}
    for p, (m, v) in stats.items():
        out[p] = ((1 - MOMENTUM) * sd[p + '.running_mean'].double() + MOMENTUM * m.double(),
                  (1 - MOMENTUM) * sd[p + '.running_var'].double() + MOMENTUM * v.double())
    return out
