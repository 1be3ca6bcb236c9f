"""CPU: the premise of tests/test_gpu_exact.py.  On the weights and images of oracle/exact_fixture.py every rounding point of the
forward is exact, so the oracle's fp32 forward, its float64 forward and its fp16 (autocast) restatement agree bit for bit; the
outputs are far from trivial; the filters of seeds 0..2 together touch every (input channel, tap) of every layer; and the four
bug classes the GPU test is meant to catch (a pixel off by 1/8, a dropped K chunk, a wrong edge row, max-pooling before a
negative-scale activation) reach the exact outputs from every layer."""
import numpy as np
import pytest
import torch

from oracle import exact_fixture as X
from oracle import mp_oracle as O

B, H, W = 3, 32, 48
IS_OPT = torch.tensor([[True], [False], [True]])


def _case(name, seed, spread='narrow'):
    cfg = X.config(name)
    return cfg, X.exact_weights(seed, cfg, spread), X.exact_images(seed, B, H, W)


@pytest.mark.parametrize('spread', ['narrow', 'wide'])
@pytest.mark.parametrize('name', list(X.CONFIGS))
def test_fp32_fp64_fp16_agree_exactly(name, spread):
    for seed in X.SEEDS:
        cfg, sd, img = _case(name, seed, spread)
        raw = dict(cfg, normalize_descriptors=False)
        r32 = O.forward(sd, img, raw, is_optical=IS_OPT, return_logits=True)
        r64 = X.forward64(sd, img, raw, is_optical=IS_OPT, return_logits=True)
        r16 = O.forward(sd, img, dict(raw, mixed_precision=True), is_optical=IS_OPT, return_logits=True)
        assert torch.equal(r32['logits'].double(), r64['logits']), (name, seed)
        assert torch.equal(r16['logits'], r32['logits']), (name, seed)
        if cfg['descriptor_head']:
            assert torch.equal(r32['desc'].double(), r64['desc']), (name, seed)
            assert torch.equal(r16['desc'], r32['desc']), (name, seed)
        t = X.truth(sd, img, cfg, is_optical=IS_OPT)
        assert torch.equal(t['logits'], r32['logits'])
        lg = t['logits']
        assert float((lg != 0).double().mean()) >= 0.8, (name, seed)
        assert lg.unique().numel() >= 100, (name, seed, lg.unique().numel())
        bound = X.SPREADS[spread]
        assert float(lg.abs().max()) <= bound
        if spread == 'wide':
            # the softmax sees arguments far below -30 (the range the __expf comment of head_tail*.hip speaks of)
            assert float((lg - lg.max(1, keepdim=True).values).min()) < -30


@pytest.mark.parametrize('name', list(X.CONFIGS))
def test_every_intermediate_is_an_exact_normal_fp16_value(name):
    """Every block output (and the logits / raw descriptors) holds fp16 numbers, none of them subnormal; every block is dense."""
    for seed in X.SEEDS:
        cfg, sd, img = _case(name, seed)
        encs = ['encoder_optical', 'encoder_thermal'] if cfg['multispectral'] else ['encoder']
        for enc in encs:
            for lname, y in X.layer_outputs(sd, img, cfg, mixed=False, encoder_name=enc):
                assert torch.equal(y.half().float(), y), (name, seed, lname)
                nz = y[y != 0].abs()
                assert nz.numel() == 0 or float(nz.min()) >= 2.0 ** -14, (name, seed, lname)
                dens = float((y != 0).double().mean())
                assert dens >= (0.8 if lname == 'logits' else 0.3), (name, seed, lname, dens)


def test_images_are_on_the_grid_with_one_flat_image():
    img = X.exact_images(5, 4, 24, 40)
    q = img * 8
    assert torch.equal(q, q.round()) and float(q.min()) >= 0 and float(q.max()) <= 8
    assert img[3].unique().numel() == 1 and img[0].unique().numel() == 9


def _conv_keys(sd):
    return [k[:-len('.weight')] for k, v in sd.items() if k.endswith('.weight') and v.dim() == 4]


@pytest.mark.parametrize('name', list(X.CONFIGS))
def test_taps_cover_every_input_channel_and_tap(name):
    """Over seeds 0..2 every (input channel, tap) of every convolution carries a nonzero weight in some filter; every BatchNorm has
    negative, zero and positive scales where it has enough channels."""
    cfg = X.config(name)
    sds = [X.exact_weights(s, cfg) for s in X.SEEDS]
    for key in _conv_keys(sds[0]):
        used = sum((sd[key + '.weight'] != 0).any(dim=0) for sd in sds)
        assert bool(used.all()), (name, key, int((used == 0).sum()))
    for key in [k[:-len('.running_var')] for k in sds[0] if k.endswith('.running_var')]:
        g = torch.cat([sd[key + '.weight'] for sd in sds])
        assert bool((g < 0).any()) and bool((g > 0).any()), (name, key)
        if g.numel() >= 3 * 32 and not key.endswith('.5'):
            assert bool((g == 0).any()), (name, key)
        for sd in sds:
            assert torch.equal(sd[key + '.running_var'], torch.full_like(g[:1], 2.0 ** 38).expand_as(sd[key + '.weight']))
            assert not bool(sd[key + '.running_mean'].any())


def test_magicleap_fixture_is_exact():
    for seed in X.SEEDS:
        sd = X.exact_weights_magicleap(seed)
        img = X.exact_images(seed, B, H, W)
        a, b = O.forward_magicleap(sd, img), X.magicleap64(sd, img)
        assert torch.equal(a['logits'].double(), b['logits'])
        assert float((a['logits'] != 0).double().mean()) >= 0.8 and a['logits'].unique().numel() >= 30
        assert torch.isfinite(b['desc']).all()                  # no all-zero descriptor (the reference divides by the norm)
        sds = [X.exact_weights_magicleap(s) for s in X.SEEDS]
    for name, _, _, _ in O.MAGICLEAP_LAYERS:
        used = sum((sd[name + '.weight'] != 0).any(dim=0) for sd in sds)
        assert bool(used.all()), name


@pytest.mark.parametrize('name', ['shipped', 'bn_first'])
def test_injected_bugs_reach_the_outputs(name):
    """Mutation power: each bug class, injected into one layer of the fp16 restatement, changes the exact logits or raw descriptors
    for at least one seed -- so a GPU kernel with that bug cannot pass tests/test_gpu_exact.py."""
    cfg = O.full_config(X.config(name, mixed_precision=True))
    layers = ['encoder.%d' % l['conv'] for l in O.encoder_layout(cfg)] + \
        ['detector_head_convolutions.1', 'descriptor_head_convolutions.1']
    pooled = {'encoder.%d' % l['conv'] for l in O.encoder_layout(cfg) if l['pool']}
    cases = {s: (X.exact_weights(s, cfg), X.exact_images(s, B, H, W)) for s in X.SEEDS}
    clean = {s: X.final_outputs(sd, img, cfg) for s, (sd, img) in cases.items()}
    missed = []
    for layer in layers:
        for mut in X.MUTATIONS:
            if mut == 'pool_preact_max' and layer not in pooled:
                continue
            hit = False
            for s, (sd, img) in cases.items():
                got = X.final_outputs(sd, img, cfg, mutate=(layer, mut))
                if any(not torch.equal(got[k], clean[s][k]) for k in got):
                    hit = True
                    break
            if not hit:
                missed.append((layer, mut))
    assert not missed, missed


def test_layer_outputs_end_in_the_forward():
    cfg, sd, img = _case('shipped', 1)
    outs = dict(X.layer_outputs(sd, img, cfg))
    r = O.forward(sd, img, dict(cfg, normalize_descriptors=False), return_logits=True)
    assert torch.equal(outs['logits'], r['logits']) and torch.equal(outs['desc_raw'], r['desc'])
    last = 'encoder.%d' % O.encoder_layout(O.full_config(cfg))[-1]['conv']
    assert np.array_equal(outs[last].shape, (B, 128, H // 8, W // 8))
