"""GPU (MI355X): the HIP path, called through the C ABI via the product's Python mirror of the
reference interface, against the oracle on the same seeded inputs, against the committed golden
vectors, and -- at BASELINE.json's full size -- through size-independent properties.

Tolerances: north_star asks for descriptors within 1e-4 (fp32); asserted here: descriptors within 1e-5, prob within 3e-5 abs
(softmax of fp32 logits whose summation order differs from ATen's: observed <= 2e-5 / 4e-6); keypoint indices BIT-EXACT given the
same probability map, tie-break (score desc, row-major index asc)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'

# north_star's bar: descriptors within 1e-4 of the CPU reference (fp32); it gives no number for the heat map.  Round 6 holds the
# benign-weights cases of this file to 10x / 3x tighter bars -- desc 1e-5, prob 3e-5 -- after measuring that every forward test passes at
# 4e-6 / 2e-5 (MP_TEST_DESC_TOL / MP_TEST_PROB_TOL tighten them for such probes, and can only tighten: a stray setting must not loosen
# the suite); trained-like statistics have their own test and bound (tests/test_gpu_trained_like.py), the fp16 path its own
# (tests/test_gpu_f16.py).
DESC_TOL = min(float(os.environ.get('MP_TEST_DESC_TOL', 1e-5)), 1e-5)
PROB_TOL = min(float(os.environ.get('MP_TEST_PROB_TOL', 3e-5)), 3e-5)


@pytest.fixture(scope='module')
def U():
    import multipoint_amd.utils as utils
    return utils


def _net(oracle, cfg, seed=0):
    import multipoint_amd.models as M
    sd = oracle.make_weights(seed, cfg)
    net = M.MultiPoint(dict(cfg)); net.load_state_dict(sd); net.to('cuda'); net.eval()
    return net, sd


@pytest.fixture(scope='module')
def shipped(oracle):
    return _net(oracle, oracle.SHIPPED_MODEL_CONFIG)


# ------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize('B,H,W', [(2, 64, 64), (1, 240, 320), (3, 72, 104), (1, 16, 16), (2, 480, 640), (5, 40, 264),
                                   (1, 1024, 1280), (2, 24, 2048), (1, 1032, 16), (3, 88, 48)])
def test_forward_matches_oracle(oracle, shipped, B, H, W):
    net, sd = shipped
    img = oracle.make_images(100 + H, B, H, W)
    ref = oracle.forward(sd, img, oracle.SHIPPED_MODEL_CONFIG)
    out = net({'image': img.cuda()})
    assert out['logits'] is None
    assert out['prob'].shape == (B, 1, H, W) and out['desc'].shape == (B, 64, H // 8, W // 8)
    assert (out['prob'].cpu() - ref['prob']).abs().max().item() <= PROB_TOL
    assert (out['desc'].cpu() - ref['desc']).abs().max().item() <= DESC_TOL


@pytest.mark.parametrize('env', [{'MP_DEBUG': v} for v in (
    'persist_min_items=1', 'no_persist', 'no_fuse', 'no_winograd', 'no_winograd,no_fuse', 'no_head_fuse', 'wino43=0',
    'no_planar', 'no_fuse43', 'wino43_gen=2', 'wino43_gen=2,no_planar', 'wino43_gen=1', 'no_vin')])
@pytest.mark.parametrize('B,H,W', [(6, 120, 160), (3, 200, 328), (3, 240, 320), (4, 64, 96)])
def test_forward_kernel_variants(oracle, monkeypatch, env, B, H, W):
    """Every convolution kernel variant against the oracle on the same inputs: the persistent one-workgroup-per-CU
    kernel forced onto small launches (all tile shapes, partial tiles at the right/bottom edge), the per-tile kernel
    only, the unfused first block in front of the direct second convolution, the first block fused into the direct kernel, the four separate head-tail launches instead of the fused
    head_tail kernel, no Winograd kernel at all (MP_DEBUG=wino43=0), the any-frame-size F(4x4,3x3) kernel on EVERY 3x3 layer
    (MP_DEBUG=wino43_gen=2: conv_wino43b.hip) or on none (=1: the direct kernels take the frames conv_wino43.hip does not), NHWC everywhere
    (MP_DEBUG=no_planar) instead of channel-quad-planar tensors behind conv1 and the pooled layers.  (Round 6 retired the switch values no
    routing selects: wino43=1, planar=2.)  The default -- standalone first block writing
    planar, conv_wino43.hip on every 3x3 layer whose frame is a multiple of 4 (conv_wino43b.hip otherwise), LDS-DMA staging -- is
    what every other test of this file runs.  (240x320: conv1-5 are multiples of 4 and run F(4x4,3x3), conv6-8 and the heads
    at 60x80 too, ... 30x40 is not: the deep layers take the any-frame-size kernel inside the SAME forward -- the mixed case the frame-size rule
    produces; 64x96: every layer F(4x4,3x3) down to 8x12.)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    net, sd = _net(oracle, oracle.SHIPPED_MODEL_CONFIG, seed=4)          # new handle: reads the environment
    img = oracle.make_images(300 + W, B, H, W)
    ref = oracle.forward(sd, img, oracle.SHIPPED_MODEL_CONFIG)
    out = net({'image': img.cuda()})
    assert (out['prob'].cpu() - ref['prob']).abs().max().item() <= PROB_TOL
    assert (out['desc'].cpu() - ref['desc']).abs().max().item() <= DESC_TOL


@pytest.mark.parametrize('B,H,W,gen', [(2, 480, 640, ''), (2, 240, 320, ''), (1, 128, 96, ''), (3, 64, 64, ''),
                                       (1, 88, 120, '2'), (2, 72, 104, '2'), (2, 240, 320, '2')])
def test_split_input_channels_on_small_launches(oracle, monkeypatch, B, H, W, gen):
    """Single-pair latency path (forwards of one or two images): an F(4x4,3x3) launch with fewer items than half the CUs runs the input channels of an item as
    2 / 4 / 8 separate items whose pre-bias output tiles split_reduce_kernel (conv_split.hip) sums in range order (conv_wino43.hip and -- gen '2':
    every layer; default routing: the layers whose frame is no multiple of 4 -- conv_wino43b.hip, SPLIT).
    Against the oracle, against the unsplit launch (MP_DEBUG=splitk_max=1: another summation order, same tolerance class as any two
    kernel variants), and bit-identical from run to run."""
    if gen:
        monkeypatch.setenv('MP_DEBUG', 'wino43_gen=' + gen)
    img = oracle.make_images(77 + W, B, H, W)
    net, sd = _net(oracle, oracle.SHIPPED_MODEL_CONFIG, seed=9)
    a = net({'image': img.cuda()})
    a2 = net({'image': img.cuda()})
    for _ in range(3):
        a3 = net({'image': img.cuda()})
        assert torch.equal(a['prob'], a3['prob']) and torch.equal(a['desc'], a3['desc'])
    assert torch.equal(a['prob'], a2['prob']) and torch.equal(a['desc'], a2['desc'])
    monkeypatch.setenv('MP_DEBUG', ('wino43_gen=' + gen + ',' if gen else '') + 'splitk_max=1')
    net1, _ = _net(oracle, oracle.SHIPPED_MODEL_CONFIG, seed=9)
    b = net1({'image': img.cuda()})
    monkeypatch.setenv('MP_DEBUG', ('wino43_gen=' + gen + ',' if gen else '') + 'splitk_max=2')
    net2, _ = _net(oracle, oracle.SHIPPED_MODEL_CONFIG, seed=9)
    c = net2({'image': img.cuda()})
    monkeypatch.setenv('MP_DEBUG', ('wino43_gen=' + gen + ',' if gen else '') + 'splitk_max=4')
    net4, _ = _net(oracle, oracle.SHIPPED_MODEL_CONFIG, seed=9)
    d = net4({'image': img.cuda()})
    ref = oracle.forward(sd, img, oracle.SHIPPED_MODEL_CONFIG)
    for o in (a, b, c, d):
        assert (o['prob'].cpu() - ref['prob']).abs().max().item() <= PROB_TOL
        assert (o['desc'].cpu() - ref['desc']).abs().max().item() <= DESC_TOL
    if B <= 2:
        assert not torch.equal(a['desc'], b['desc'])        # the split really ran
    else:       # forwards of more than two images never split: their bits must not depend on the batch size
        assert torch.equal(a['desc'], b['desc']) and torch.equal(a['prob'], b['prob'])
    assert (a['prob'] - b['prob']).abs().max().item() <= 3e-5 and (a['desc'] - b['desc']).abs().max().item() <= 3e-6


def test_reload_restores_auto_algorithm(oracle):
    """mp_load_weights starts every load from the switches mp_create read (round-4 advisor): a handle that held a `direct` (or
    `winograd43_general`) model and is reloaded with `auto` must run what a fresh `auto` handle runs, bit for bit."""
    cfg = dict(oracle.SHIPPED_MODEL_CONFIG)
    fresh, sd = _net(oracle, cfg, seed=4)
    img = oracle.make_images(77, 3, 120, 160).cuda()
    want = fresh({'image': img})
    for first in ('direct', 'winograd43_general'):
        net, _ = _net(oracle, dict(cfg, conv_algorithm=first), seed=4)
        other = net({'image': img})
        assert not torch.equal(other['desc'], want['desc'])           # the first load really ran another algorithm
        net.config['conv_algorithm'] = 'auto'
        net.load_state_dict(sd)                                       # same handle, reloaded
        got = net({'image': img})
        assert torch.equal(got['prob'], want['prob']) and torch.equal(got['desc'], want['desc']), first


def test_split_launch_gate_is_the_whole_forward(oracle):
    """The split small launches are gated on the forward's image count, not on one encoder's share of it (round-4 advisor):
    a multispectral forward of 4 interleaved images (2 per encoder) or of 6 images with ONE thermal image has the bits of the same
    images inside a larger batch, without `batch_invariant`."""
    cfg = dict(oracle.SHIPPED_MODEL_CONFIG, multispectral=True)
    net, _ = _net(oracle, cfg, seed=6)
    img = oracle.make_images(31, 8, 240, 320).cuda()
    opt = torch.tensor([[True], [False]] * 4).cuda()
    big = net({'image': img, 'is_optical': opt})
    part = net({'image': img[:4], 'is_optical': opt[:4]})
    assert torch.equal(part['prob'], big['prob'][:4]) and torch.equal(part['desc'], big['desc'][:4])
    opt1 = torch.tensor([[True]] * 5 + [[False]]).cuda()
    six = net({'image': img[:6], 'is_optical': opt1})
    opt2 = torch.tensor([[True]] * 5 + [[False]] + [[False], [True]]).cuda()
    eight = net({'image': img, 'is_optical': opt2})
    assert torch.equal(six['prob'], eight['prob'][:6]) and torch.equal(six['desc'], eight['desc'][:6])


@pytest.mark.parametrize('H,W', [(480, 640), (240, 320)])
def test_batch_invariant_setting(oracle, H, W):
    """model.batch_invariant (mp_model_config.batch_invariant): forwards of one or two images leave the split small launches out,
    so a shard of two images has the bits of the same images inside a larger batch; without it they differ (and stay inside
    the tolerance)."""
    img = oracle.make_images(5 + H, 6, H, W).cuda()
    cfg = dict(oracle.SHIPPED_MODEL_CONFIG)
    fast, _ = _net(oracle, cfg, seed=9)
    cfg['batch_invariant'] = True
    inv, _ = _net(oracle, cfg, seed=9)
    big = inv({'image': img})
    big_fast = fast({'image': img})
    assert torch.equal(big['prob'], big_fast['prob']) and torch.equal(big['desc'], big_fast['desc'])      # batched forwards: one path
    for lo in (0, 2, 4):
        part = inv({'image': img[lo:lo + 2]})
        assert torch.equal(part['prob'], big['prob'][lo:lo + 2]) and torch.equal(part['desc'], big['desc'][lo:lo + 2])
    one = inv({'image': img[3:4]})
    assert torch.equal(one['prob'], big['prob'][3:4]) and torch.equal(one['desc'], big['desc'][3:4])
    part = fast({'image': img[0:2]})
    assert not torch.equal(part['desc'], big['desc'][0:2])
    assert (part['prob'] - big['prob'][0:2]).abs().max().item() <= 3e-5 and (part['desc'] - big['desc'][0:2]).abs().max().item() <= 3e-6


@pytest.mark.parametrize('env', [{}, {'MP_DEBUG': 'wino43=0'}, {'MP_DEBUG': 'no_winograd'}])
@pytest.mark.parametrize('upd', [{}, {'multispectral': True, 'bn_first': True}, {'reflection_pad': False},
                                 {'channel_version': 1, 'descriptor_size': 128}])
@pytest.mark.parametrize('B,H,W', [(3, 72, 104), (2, 240, 320), (1, 16, 16)])
def test_single_convolution_per_stage(oracle, monkeypatch, env, upd, B, H, W):
    """`double_convolution: false` (MultiPoint.py:144-148): one 3x3 convolution per stage, MaxPool2d(2,2) directly behind the first
    block (conv_first_pool_kernel) and behind stages 2 and 3; state_dict keys encoder.{1,6,11,16} / BN {3,8,13,18} -- the three
    convolution families against the oracle (itself pinned on this layout by tests/golden/forward_variants.npz)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = dict(oracle.SHIPPED_MODEL_CONFIG); cfg['double_convolution'] = False; cfg.update(upd)
    net, sd = _net(oracle, cfg, seed=8)
    assert 'encoder.16.weight' in sd or 'encoder_thermal.16.weight' in sd
    img = oracle.make_images(61 + W, B, H, W)
    flags = torch.tensor([[i % 2 == 0] for i in range(B)])
    ref = oracle.forward(sd, img, cfg, is_optical=flags)
    out = net({'image': img.cuda(), 'is_optical': flags})
    assert out['desc'].shape == (B, cfg['descriptor_size'], H // 8, W // 8)
    assert (out['prob'].cpu() - ref['prob']).abs().max().item() <= PROB_TOL
    assert (out['desc'].cpu() - ref['desc']).abs().max().item() <= DESC_TOL


@pytest.mark.parametrize('upd', [{}, {'multispectral': True}, {'bn_first': True}])
@pytest.mark.parametrize('B,H,W', [(3, 72, 104), (2, 16, 16), (1, 240, 320), (5, 40, 264), (2, 480, 640)])
def test_first_block_inside_f43_equals_standalone(oracle, monkeypatch, upd, B, H, W):
    """The first encoder block evaluated inside the F(4x4,3x3) conv2 kernel (default; round 3: per unit, straight into the raw LDS
    ring, nine rank-1 v_mfma_f32_4x4x1 updates per pixel with the bias as the accumulator's initial value) against the standalone
    first-block launch (MP_DEBUG=no_fuse43: a k-ordered multiply-add chain, bias added last): the same nine products and the bias summed
    in another order, so the block's outputs differ by an ulp here and there and the network outputs by what that becomes
    downstream (measured: prob <= 1.0e-5, desc <= 6e-7 between the two; each of them 6.5e-6 .. 9.9e-6 from an fp64 evaluation,
    the fp32 CPU oracle 7e-6 .. 1.2e-5) -- borders (two nested reflections), partial items, two encoders, bn_first."""
    cfg = dict(oracle.SHIPPED_MODEL_CONFIG); cfg.update(upd)
    img = oracle.make_images(31 + W, B, H, W)
    flags = torch.tensor([[i % 2 == 0] for i in range(B)])
    net, sd = _net(oracle, cfg, seed=6)
    a = net({'image': img.cuda(), 'is_optical': flags})
    monkeypatch.setenv('MP_DEBUG', 'no_fuse43')
    net2, _ = _net(oracle, cfg, seed=6)
    b = net2({'image': img.cuda(), 'is_optical': flags})
    ref = oracle.forward(sd, img, cfg, is_optical=flags)
    assert (a['prob'].cpu() - ref['prob']).abs().max().item() <= PROB_TOL and (a['desc'].cpu() - ref['desc']).abs().max().item() <= DESC_TOL
    assert (b['prob'].cpu() - ref['prob']).abs().max().item() <= PROB_TOL and (b['desc'].cpu() - ref['desc']).abs().max().item() <= DESC_TOL
    assert (a['prob'] - b['prob']).abs().max().item() <= 3e-5 and (a['desc'] - b['desc']).abs().max().item() <= 3e-6


@pytest.mark.parametrize('upd', [{}, {'multispectral': True}, {'bn_first': True}, {'descriptor_size': 128}, {'descriptor_head': False}])
@pytest.mark.parametrize('B,H,W', [(3, 72, 104), (2, 16, 16), (1, 240, 320), (5, 120, 160), (2, 480, 640)])
def test_pretransformed_head_input_is_bit_identical(oracle, monkeypatch, upd, B, H, W):
    """The 3x3 head convolutions (512 couts = 8 output slices over ONE input, MultiPoint.py:62-65,78-81) run with their input
    transform V = B^T d B as a pass of its own (conv_wino43.hip: wino43_vprod_kernel + the VIN instantiation that DMAs V) instead of
    transforming the same windows once per slice (MP_DEBUG=no_vin).  The producer runs the same column-pass / row-pass chains, so the
    outputs are EQUAL -- reflected borders, phantom tiles of partial tile blocks, both item shapes (60x80: 8x4 tiles; 9x13: 4x8)."""
    cfg = dict(oracle.SHIPPED_MODEL_CONFIG); cfg.update(upd)
    img = oracle.make_images(13 + W, B, H, W)
    flags = torch.tensor([[i % 2 == 0] for i in range(B)])
    net, sd = _net(oracle, cfg, seed=8)
    a = net({'image': img.cuda(), 'is_optical': flags})
    monkeypatch.setenv('MP_DEBUG', 'no_vin')
    net2, _ = _net(oracle, cfg, seed=8)
    b = net2({'image': img.cuda(), 'is_optical': flags})
    assert torch.equal(a['prob'], b['prob'])
    assert (a.get('desc') is None and b.get('desc') is None) or torch.equal(a['desc'], b['desc'])
    ref = oracle.forward(sd, img, cfg, is_optical=flags)
    assert (a['prob'].cpu() - ref['prob']).abs().max().item() <= PROB_TOL


@pytest.mark.parametrize('upd', [{}, {'multispectral': True}, {'bn_first': True}])
@pytest.mark.parametrize('B,H,W', [(3, 72, 104), (2, 16, 16), (1, 240, 320), (2, 88, 48)])
def test_planar_layout_is_bit_identical(oracle, monkeypatch, upd, B, H, W):
    """Channel-quad-planar tensors [B][C/4][H][W][4] between conv1 and the F(4x4,3x3) layers (default) against NHWC everywhere
    (MP_DEBUG=no_planar): the layout changes which bytes a DMA fetches, not one multiply-add, so the outputs are EQUAL -- partial
    items, reflected borders, two encoders with image lists."""
    cfg = dict(oracle.SHIPPED_MODEL_CONFIG); cfg.update(upd)
    img = oracle.make_images(23 + W, B, H, W)
    flags = torch.tensor([[i % 2 == 0] for i in range(B)])
    net, sd = _net(oracle, cfg, seed=5)
    a = net({'image': img.cuda(), 'is_optical': flags})
    monkeypatch.setenv('MP_DEBUG', 'no_planar')
    net2, _ = _net(oracle, cfg, seed=5)
    b = net2({'image': img.cuda(), 'is_optical': flags})
    assert torch.equal(a['prob'], b['prob']) and torch.equal(a['desc'], b['desc'])


@pytest.mark.parametrize('bn_first', [False, True])
@pytest.mark.parametrize('B,H,W', [(2, 64, 64), (1, 240, 320), (2, 104, 72)])
def test_pooled_epilogue_with_negative_batchnorm_scales(oracle, bn_first, B, H, W):
    """The pooled F(4x4,3x3) epilogue pools BEFORE it activates, with the sign of the channel's BatchNorm scale folded into the
    bias multiply-add (conv_wino43.hip; tests/test_host_logic.py holds the identity): a third of every encoder BatchNorm's
    gammas negative, one exactly zero -- the synthetic generator only draws positive ones."""
    import multipoint_amd.models as M
    cfg = dict(oracle.SHIPPED_MODEL_CONFIG); cfg['bn_first'] = bn_first
    sd = oracle.make_weights(3, cfg)
    for k in list(sd):
        if k.startswith('encoder.') and k.endswith('.weight') and sd[k].dim() == 1:
            g = sd[k].clone(); g[::3] *= -1.0; g[1] = 0.0
            sd[k] = g
    net = M.MultiPoint(dict(cfg)); net.load_state_dict(sd); net.to('cuda'); net.eval()
    img = oracle.make_images(50 + H, B, H, W)
    ref = oracle.forward(sd, img, cfg)
    out = net({'image': img.cuda()})
    assert (out['prob'].cpu() - ref['prob']).abs().max().item() <= PROB_TOL
    assert (out['desc'].cpu() - ref['desc']).abs().max().item() <= DESC_TOL


@pytest.mark.parametrize('upd', [{'channel_version': 1}, {'channel_version': 2}, {'channel_version': 1, 'descriptor_size': 128},
                                 {'channel_version': 2, 'multispectral': True, 'reflection_pad': False}])
def test_forward_channel_versions(oracle, upd):
    """channel_version 1 ([1,32,64,96,128]) and 2 ([1,8,16,32,64]) with head width = descriptor_size (MultiPoint.py:38-53):
    the same kernels on tensors zero-padded to multiples of 32 channels."""
    cfg = dict(oracle.SHIPPED_MODEL_CONFIG); cfg.update(upd)
    net, sd = _net(oracle, cfg, seed=9)
    B, H, W = 3, 72, 104
    img = oracle.make_images(17, B, H, W)
    is_opt = torch.tensor([[True], [False], [True]])
    ref = oracle.forward(sd, img, cfg, is_optical=is_opt)
    out = net({'image': img.cuda(), 'is_optical': is_opt.cuda()})
    assert out['desc'].shape == (B, cfg['descriptor_size'], H // 8, W // 8)
    assert (out['prob'].cpu() - ref['prob']).abs().max().item() <= PROB_TOL
    assert (out['desc'].cpu() - ref['desc']).abs().max().item() <= DESC_TOL
    big = oracle.make_images(18, 8, 240, 320)                               # large enough for the persistent kernel
    refb = oracle.forward(sd, big, cfg, is_optical=torch.ones(8, 1, dtype=torch.bool))
    outb = net({'image': big.cuda(), 'is_optical': torch.ones(8, 1, dtype=torch.bool).cuda()})
    assert (outb['prob'].cpu() - refb['prob']).abs().max().item() <= PROB_TOL
    assert (outb['desc'].cpu() - refb['desc']).abs().max().item() <= DESC_TOL


def test_forward_matches_reference_golden(oracle, shipped, golden_dir):
    """Directly against outputs of the imported reference (no oracle in between)."""
    net, _ = shipped
    g = np.load(os.path.join(golden_dir, 'forward_64x64.npz'))
    img = oracle.make_images(int(g['image_seed']), 2, 64, 64)
    out = net({'image': img.cuda()})
    assert np.abs(out['prob'].cpu().numpy() - g['prob']).max() <= PROB_TOL
    assert np.abs(out['desc'].cpu().numpy() - g['desc']).max() <= DESC_TOL
    g = np.load(os.path.join(golden_dir, 'forward_240x320.npz'))          # BASELINE configs[0] shape
    out = net({'image': oracle.make_images(int(g['image_seed']), 1, 240, 320).cuda()})
    p = out['prob'].cpu().numpy().ravel(); d = out['desc'].cpu().numpy().ravel()
    assert np.abs(p[g['prob_idx']] - g['prob_val']).max() <= PROB_TOL
    assert np.abs(d[g['desc_idx']] - g['desc_val']).max() <= DESC_TOL


@pytest.mark.parametrize('name,upd', [('multispectral', {'multispectral': True}), ('zero_pad', {'reflection_pad': False}),
                                      ('bn_first', {'bn_first': True}), ('desc256', {'descriptor_size': 256}),
                                      ('no_final_bn', {'final_batchnorm': False}),
                                      ('single_conv', {'double_convolution': False}),
                                      ('single_conv_ms_zero_pad', {'double_convolution': False, 'multispectral': True,
                                                                   'reflection_pad': False, 'bn_first': True}),
                                      ('no_normalize', {'normalize_descriptors': False})])
def test_forward_variants_match_reference_golden(oracle, golden_dir, name, upd):
    g = np.load(os.path.join(golden_dir, 'forward_variants.npz'))
    cfg = dict(oracle.SHIPPED_MODEL_CONFIG); cfg.update(upd)
    net, _ = _net(oracle, cfg, int(g['weight_seed']))
    img = oracle.make_images(int(g['image_seed']), 3, 32, 48)
    flags = torch.tensor([[True], [False], [True]])
    out = net({'image': img.cuda(), 'is_optical': flags.cuda()})
    scale = max(1.0, float(np.abs(g[name + '_desc']).max()))
    assert np.abs(out['prob'].cpu().numpy() - g[name + '_prob']).max() <= PROB_TOL
    assert np.abs(out['desc'].cpu().numpy() - g[name + '_desc']).max() <= DESC_TOL * scale


def test_forwards_on_alternating_streams_share_the_workspace_safely(oracle, shipped):
    """One workspace per handle: a forward enqueued on another stream than the previous one is ordered behind it by the model
    (PairPipeline runs its forwards on a stream of its own while callers keep using theirs) -- no host synchronisation needed."""
    net, sd = shipped
    a = oracle.make_images(71, 6, 240, 320).cuda()
    b = oracle.make_images(72, 6, 240, 320).cuda()
    ra = net({'image': a}); rb = net({'image': b})
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for _ in range(3):
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            oa = net({'image': a})
        ob = net({'image': b})                        # the caller's stream, right behind it, same workspace
        with torch.cuda.stream(side):
            oa2 = net({'image': a})
        torch.cuda.synchronize()
        assert torch.equal(oa['prob'], ra['prob']) and torch.equal(oa['desc'], ra['desc'])
        assert torch.equal(ob['prob'], rb['prob']) and torch.equal(ob['desc'], rb['desc'])
        assert torch.equal(oa2['prob'], ra['prob']) and torch.equal(oa2['desc'], ra['desc'])


def test_force_return_logits(oracle, shipped, golden_dir):
    net, _ = shipped
    g = np.load(os.path.join(golden_dir, 'forward_variants.npz'))
    net.set_force_return_logits(True)
    try:
        out = net({'image': oracle.make_images(int(g['image_seed']), 3, 32, 48).cuda()})
    finally:
        net.set_force_return_logits(False)
    assert out['prob'] is None
    assert np.abs(out['logits'].cpu().numpy() - g['logits']).max() <= 1e-4


def test_superpoint_magicleap_model(oracle, golden_dir):
    """model.type 'SuperPointMagicLeap' (zero pad, no BatchNorm, D = 256, exp/(sum+1e-5) heat map) against the
    reference's own output and the oracle at a larger size."""
    import multipoint_amd.models as M
    g = np.load(os.path.join(golden_dir, 'forward_magicleap.npz'))
    sd = oracle.make_weights_magicleap(int(g['weight_seed']))
    net = M.SuperPointMagicLeap(); net.load_state_dict(sd); net.to('cuda'); net.eval()
    out = net({'image': oracle.make_images(int(g['image_seed']), 2, 32, 48).cuda()})
    assert set(out) == {'logits', 'desc', 'prob'}
    assert np.abs(out['logits'].cpu().numpy() - g['logits']).max() <= 1e-4
    assert np.abs(out['desc'].cpu().numpy() - g['desc']).max() <= DESC_TOL
    assert np.abs(out['prob'].cpu().numpy() - g['prob']).max() <= PROB_TOL
    img = oracle.make_images(3, 2, 240, 320)
    ref = oracle.forward_magicleap(sd, img)
    out = net({'image': img.cuda()})
    assert (out['prob'].cpu() - ref['prob']).abs().max().item() <= PROB_TOL
    assert (out['desc'].cpu() - ref['desc']).abs().max().item() <= DESC_TOL
    with pytest.raises(RuntimeError, match='Missing key'):
        M.SuperPointMagicLeap().load_state_dict({k: v for k, v in sd.items() if k != 'convDb.bias'})


def test_retired_switch_names_are_reported(oracle):
    """Rounds 1-4 selected kernels with ~20 MP_* variables; round 5 folded them into MP_DEBUG=key[=value],...  A script that still
    sets an old name would silently compare the default against itself: mp_create says so once on stderr (round-5 advisor)."""
    import subprocess, sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from multipoint_amd import _lib\n_lib.get_handle('cuda:0'); _lib.Handle(0)\nprint('created')\n" % ROOT)
    env = dict(os.environ); env['MP_NO_WINOGRAD'] = '1'
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'created' in r.stdout, r.stderr[-1500:]
    assert r.stderr.count('MP_NO_WINOGRAD is no longer read') == 1 and 'MP_DEBUG=key' in r.stderr
    env.pop('MP_NO_WINOGRAD')
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'no longer read' not in r.stderr


def test_forward_errors(oracle, shipped):
    net, _ = shipped
    with pytest.raises(ValueError, match='divisible by 8'):
        net({'image': torch.rand(1, 1, 60, 64, device='cuda')})
    with pytest.raises(ValueError):
        net({'image': torch.rand(1, 3, 64, 64, device='cuda')})
    import multipoint_amd.models as M
    with pytest.raises(RuntimeError, match='no weights'):
        M.MultiPoint(dict(oracle.SHIPPED_MODEL_CONFIG))({'image': torch.rand(1, 1, 64, 64, device='cuda')})


# ------------------------------------------------------------------------------------------ box NMS
def _heat(rng, B, H, W, density, levels=0):
    p = rng.random((B, 1, H, W), dtype=np.float32)
    p = np.where(rng.random((B, 1, H, W)) < density, p, 0).astype(np.float32)
    if levels:
        p = (np.floor(p * levels) / levels).astype(np.float32)
    return p


@pytest.mark.parametrize('seed,density,levels,size,iou,topk', [
    (0, 0.07, 0, 4, 0.1, 0), (1, 0.5, 0, 4, 0.1, 50), (2, 1.0, 0, 4, 0.1, 0), (3, 0.6, 6, 4, 0.1, 40),
    (4, 0.3, 0, 2, 0.1, 0), (5, 0.3, 3, 8, 0.1, 25), (6, 0.4, 0, 4, 0.3, 0), (7, 0.9, 2, 3, 0.05, 10),
    (8, 0.2, 0, 1, 0.1, 0), (9, 1.0, 1, 4, 0.1, 7)])
def test_box_nms_bit_exact(oracle, U, seed, density, levels, size, iou, topk):
    rng = np.random.default_rng(seed)
    p = _heat(rng, 3, 72, 104, density, levels)
    ref = oracle.box_nms(p, size, 0.015, iou=iou, keep_top_k=topk)
    out = U.box_nms(torch.from_numpy(p).cuda(), size, 0.015, iou=iou, keep_top_k=topk)
    assert out.shape == p.shape and out.is_cuda
    assert np.array_equal(out.cpu().numpy(), ref)
    # 2-D form (utils.py:90-91) and CPU tensors (result returned on the input's device)
    out2 = U.box_nms(torch.from_numpy(p[1, 0]), size, 0.015, iou=iou, keep_top_k=topk)
    assert not out2.is_cuda and np.array_equal(out2.numpy(), oracle.box_nms(p[1, 0], size, 0.015, iou=iou, keep_top_k=topk))


def test_box_nms_on_network_output_and_mask(oracle, U, shipped):
    net, sd = shipped
    img = oracle.make_images(5, 2, 240, 320)
    rp = oracle.forward(sd, img, oracle.SHIPPED_MODEL_CONFIG)['prob'].numpy()
    mask = np.ones_like(rp, dtype=bool); mask[:, :, :40] = False; mask[:, :, :, 300:] = False
    for topk in (0, 300):
        ref = oracle.box_nms(rp * mask, 4, 0.015, keep_top_k=topk)
        out = U.box_nms(torch.from_numpy(rp).cuda(), 4, 0.015, keep_top_k=topk, valid_mask=torch.from_numpy(mask).cuda())
        assert np.array_equal(out.cpu().numpy(), ref)
        kp, sc, cnt = U.detect_keypoints(torch.from_numpy(rp).cuda(), 4, 0.015, keep_top_k=topk, capacity=4096,
                                         valid_mask=torch.from_numpy(mask).cuda())
        for b in range(2):
            okp = oracle.keypoints_from_map(ref[b, 0], 0.015)
            n = int(cnt[b])
            assert n == len(okp)
            assert np.array_equal(kp[b, :n].cpu().numpy().astype(np.int64), okp)       # torch.nonzero order
            assert np.array_equal(sc[b, :n].cpu().numpy(), ref[b, 0][okp[:, 0], okp[:, 1]])


def test_box_nms_edge_cases(oracle, U):
    z = torch.zeros(2, 1, 32, 40, device='cuda')
    assert not U.box_nms(z, 4, 0.015, keep_top_k=5).any()
    kp, sc, cnt = U.detect_keypoints(z, 4, 0.015, keep_top_k=5)
    assert cnt.tolist() == [0, 0]
    c = np.full((16, 24), 0.3, dtype=np.float32)                              # all ties
    assert np.array_equal(U.box_nms(torch.from_numpy(c).cuda(), 4, 0.015).cpu().numpy(), oracle.box_nms(c, 4, 0.015))
    ramp = np.linspace(0.02, 0.9, 64 * 200, dtype=np.float32).reshape(64, 200)   # long dependency chain
    assert np.array_equal(U.box_nms(torch.from_numpy(ramp).cuda(), 4, 0.015).cpu().numpy(), oracle.box_nms(ramp, 4, 0.015))
    with pytest.raises(ValueError):
        U.box_nms(torch.rand(16, 24, device='cuda'), 40, 0.015)               # footprint radius unsupported (stated deviation: size <= 16)
    m = U.extract_keypoints(torch.from_numpy(ramp).cuda(), 0.5)
    assert np.array_equal(m[0][0, :int(m[2][0])].cpu().numpy(), np.argwhere(ramp > 0.5))
    vm = np.random.default_rng(0).random(ramp.shape) < 0.5                     # nonzero((prob > thr) * valid_mask)
    m = U.extract_keypoints(torch.from_numpy(ramp).cuda(), 0.5, valid_mask=torch.from_numpy(vm).cuda())
    assert np.array_equal(m[0][0, :int(m[2][0])].cpu().numpy(), np.argwhere((ramp > 0.5) & vm))


@pytest.mark.parametrize('B,H,W', [(1, 37, 45), (3, 33, 131), (2, 5, 3), (2, 1, 1), (3, 129, 257), (2, 64, 66)])
def test_extract_keypoints_any_frame(U, B, H, W):
    """torch.nonzero((prob > thr) * valid_mask) (evaluation.py:156-157) takes any map: pixel counts that are no multiple of 4 (every
    image of a batch then starts at an unaligned address), with and without a mask, row-major order, counts beyond the capacity."""
    rng = np.random.default_rng(B * 100000 + H * 1000 + W)
    p = rng.random((B, 1, H, W), dtype=np.float32)
    vm = rng.random((B, 1, H, W)) < 0.6
    for mask in (None, vm):
        kp, sc, cnt = U.extract_keypoints(torch.from_numpy(p).cuda(), 0.5, capacity=H * W,
                                          valid_mask=None if mask is None else torch.from_numpy(mask).cuda())
        for b in range(B):
            keep = p[b, 0] > 0.5 if mask is None else (p[b, 0] > 0.5) & mask[b, 0]
            ref = np.argwhere(keep)
            n = int(cnt[b])
            assert n == len(ref)
            assert np.array_equal(kp[b, :n].cpu().numpy().astype(np.int64), ref)
            assert np.array_equal(sc[b, :n].cpu().numpy(), p[b, 0][keep])
    K = max(1, (H * W) // 8)                                                   # capacity smaller than the count: first K in order, true count
    kp, sc, cnt = U.extract_keypoints(torch.from_numpy(p).cuda(), 0.5, capacity=K)
    for b in range(B):
        ref = np.argwhere(p[b, 0] > 0.5)
        assert int(cnt[b]) == len(ref)
        m = min(K, len(ref))
        assert np.array_equal(kp[b, :m].cpu().numpy().astype(np.int64), ref[:m])


@pytest.mark.parametrize('H,W,size,iou,topk', [(37, 45, 4, 0.1, 0), (33, 131, 4, 0.1, 60), (40, 50, 11, 0.1, 0), (17, 23, 3, 0.05, 9),
                                                (64, 101, 12, 0.1, 0), (48, 66, 16, 0.2, 5), (5, 3, 4, 0.1, 0), (31, 1, 2, 0.1, 0)])
def test_box_nms_any_frame_and_large_boxes(oracle, U, H, W, size, iou, topk):
    """utils.box_nms takes any H x W and any box size (utils.py:78-122): widths that are no multiple of 4 (the work map's rows are
    padded internally), sizes up to 16, the threshold compared in double (size 11 / iou 0.1: offset 9 overlaps by exactly 0.1f)."""
    rng = np.random.default_rng(H * 1000 + W)
    p = _heat(rng, 2, H, W, 0.5, 5)
    mask = rng.random((2, 1, H, W)) < 0.8
    ref = oracle.box_nms(p * mask, size, 0.015, iou=iou, keep_top_k=topk)
    out = U.box_nms(torch.from_numpy(p).cuda(), size, 0.015, iou=iou, keep_top_k=topk, valid_mask=torch.from_numpy(mask).cuda())
    assert out.shape == p.shape and np.array_equal(out.cpu().numpy(), ref)
    assert np.array_equal(U.box_nms(torch.from_numpy(p[0, 0]).cuda(), size, 0.015, iou=iou, keep_top_k=topk).cpu().numpy(),
                          oracle.box_nms(p[0, 0], size, 0.015, iou=iou, keep_top_k=topk))
    kp, sc, cnt = U.detect_keypoints(torch.from_numpy(p).cuda(), size, 0.015, iou=iou, keep_top_k=topk, capacity=H * W,
                                     valid_mask=torch.from_numpy(mask).cuda())
    for b in range(2):
        okp = oracle.keypoints_from_map(ref[b, 0], 0.015)
        assert int(cnt[b]) == len(okp) and np.array_equal(kp[b, :len(okp)].cpu().numpy().astype(np.int64), okp)
        assert np.array_equal(sc[b, :len(okp)].cpu().numpy(), ref[b, 0][okp[:, 0], okp[:, 1]])


def test_box_nms_threshold_compared_in_double(oracle, U):
    """oracle/nms_greedy.c: torchvision compares the fp32 overlap ratio with the DOUBLE threshold -- 22 / 220 = 0.1f > 0.1."""
    p = np.zeros((8, 40), dtype=np.float32)
    p[4, 10] = 0.9; p[4, 19] = 0.5
    out = U.box_nms(torch.from_numpy(p).cuda(), 11, 0.015, iou=0.1).cpu().numpy()
    assert out[4, 10] == np.float32(0.9) and out[4, 19] == 0 and np.array_equal(out, oracle.box_nms(p, 11, 0.015, iou=0.1))
    out = U.box_nms(torch.from_numpy(p).cuda(), 11, 0.015, iou=float(np.float32(0.1))).cpu().numpy()
    assert out[4, 19] == np.float32(0.5)


def test_tie_guards_flag_plateaus_only(oracle, U):
    """Footprint tie guard (any keep_top_k) and the exact-tie split of the top-k cut (include/multipoint_hip.h)."""
    rng = np.random.default_rng(3)
    H, W = 96, 128
    noise = _heat(rng, 1, H, W, 0.05)[0, 0]                  # independent scores: next to no near-ties inside a footprint
    plateau = np.zeros((H, W), dtype=np.float32)
    plateau[8:88:2, 8:120:2] = 0.25                          # equal scores two pixels apart: every suppression is a tie
    near = plateau.copy(); near[plateau > 0] += (rng.random(int((plateau > 0).sum())).astype(np.float32) * 4e-5)
    p = np.stack([noise, plateau, near, noise])[:, None]
    U.topk_ambiguous(None, 0)                                # (drain what earlier calls on this handle left in the running total)
    for topk in (0, 50):
        out = U.box_nms(torch.from_numpy(p).cuda(), 4, 0.015, keep_top_k=topk)
        assert np.array_equal(out.cpu().numpy(), oracle.box_nms(p, 4, 0.015, keep_top_k=topk))      # (the guard only reports)
        flags, total = U.topk_ambiguous(None, 4)
        assert flags == [False, True, True, False] and total == 2
    assert U.topk_ambiguous(None, 4)[1] == 0                 # the read drained the running total
    U.nms_tie_guard(None, 0)                                 # footprint guard off: topk 0 flags nothing ...
    try:
        U.box_nms(torch.from_numpy(p).cuda(), 4, 0.015, keep_top_k=0)
        assert U.topk_ambiguous(None, 4) == ([False] * 4, 0)
        # ... and with a top-k cut only what the CUT sees: 4 survivors of one score around rank 3 split an exact tie -- flagged
        # although fewer than min_each_side (4) sit on either side
        q = np.zeros((2, 1, 32, 64), dtype=np.float32)
        q[0, 0, 4, 4:64:8] = [0.9, 0.8, 0.5, 0.5, 0.5, 0.5, 0.2, 0.1]
        q[1, 0, 4, 4:64:8] = [0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.2, 0.1]
        out = U.box_nms(torch.from_numpy(q).cuda(), 4, 0.015, keep_top_k=3)
        assert np.array_equal(out.cpu().numpy(), oracle.box_nms(q, 4, 0.015, keep_top_k=3))
        assert U.topk_ambiguous(None, 2) == ([True, False], 1)
    finally:
        U.nms_tie_guard(None, 16)


def test_box_nms_async_rounds_and_overflow(oracle, U):
    """The pipeline enqueues a fixed number of fixed-point rounds without synchronising; convergence is
    checked afterwards.  A monotone ramp forces a dependency chain across many 32x32 tiles."""
    ramp = np.linspace(0.02, 0.9, 64 * 640, dtype=np.float32).reshape(1, 1, 64, 640)
    t = torch.from_numpy(ramp).cuda()
    kp, sc, cnt = U.detect_keypoints(t, 4, 0.015, keep_top_k=0, capacity=4096, max_rounds=1)
    assert U.nms_unresolved() > 0                              # one round is not enough for this input
    kp, sc, cnt = U.detect_keypoints(t, 4, 0.015, keep_top_k=0, capacity=4096, max_rounds=64)
    assert U.nms_unresolved() == 0
    ref = oracle.keypoints_from_map(oracle.box_nms(ramp[0, 0], 4, 0.015), 0.015)
    assert int(cnt[0]) == len(ref) and np.array_equal(kp[0, :len(ref)].cpu().numpy(), ref)
    # capacity overflow with keep_top_k == 0: the count reports all survivors, the list holds the first K
    kp2, sc2, cnt2 = U.detect_keypoints(t, 4, 0.015, keep_top_k=0, capacity=16)
    assert int(cnt2[0]) == len(ref) and np.array_equal(kp2[0].cpu().numpy(), ref[:16])
    # top-k larger than the number of survivors
    kp3, sc3, cnt3 = U.detect_keypoints(t, 4, 0.015, keep_top_k=100000, capacity=8192)
    assert int(cnt3[0]) == len(ref)


def test_box_nms_more_than_64_rounds(oracle, U):
    """A strictly increasing ramp along a 4096-pixel row is one chain of dependent decisions across 128 tiles: the
    synchronising NMS keeps iterating (counter slots recycled after 64 rounds) and still equals the greedy algorithm."""
    W = 4096
    ramp = np.broadcast_to(np.linspace(0.02, 0.9, W, dtype=np.float32), (8, W)).copy()
    ramp += (np.arange(8, dtype=np.float32) * 1e-4)[:, None]
    got = U.box_nms(torch.from_numpy(ramp).cuda(), 4, 0.015).cpu().numpy()
    assert np.array_equal(got, oracle.box_nms(ramp, 4, 0.015)) and (got > 0).sum() > W // 8
    kp, sc, cnt = U.detect_keypoints(torch.from_numpy(ramp[None, None]).cuda(), 4, 0.015, capacity=8192, max_rounds=64)
    assert U.nms_unresolved() > 0                              # 64 fixed rounds are not enough here ...
    kp, sc, cnt = U.detect_keypoints(torch.from_numpy(ramp[None, None]).cuda(), 4, 0.015, capacity=8192)
    assert U.nms_unresolved() == 0                             # ... the converging form is
    ref = oracle.keypoints_from_map(got, 0.015)
    assert int(cnt[0]) == len(ref) and np.array_equal(kp[0, :len(ref)].cpu().numpy(), ref)


def test_pipeline_falls_back_to_converging_nms(oracle, shipped):
    """PairPipeline.__call__ (the entry of the evaluation drivers) stays exact when the fixed asynchronous rounds are
    too few: same keypoints and matches as a pipeline with plenty of rounds."""
    from multipoint_amd.pipeline import PairPipeline
    net, sd = shipped
    img = oracle.make_images(3, 4, 120, 160).cuda()
    pred = {'nms': 4, 'detection_threshold': 0.0005, 'topk': 0,
            'matching': {'method': 'bfmatcher', 'method_kwargs': {'crossCheck': True}, 'knn_matches': False}}
    few = PairPipeline(net, pred, capacity=4096, nms_rounds=1)
    many = PairPipeline(net, pred, capacity=4096, nms_rounds=32)
    a = few(img[0::2], img[1::2])
    few.check_converged()
    b = many(img[0::2], img[1::2])
    many.check_converged()
    assert torch.equal(a.kp_count, b.kp_count) and torch.equal(a.match_count, b.match_count)
    for i in range(4):
        n = int(a.kp_count[i])
        assert n > 100 and torch.equal(a.kp_yx[i, :n], b.kp_yx[i, :n])
    for p in range(2):
        n = int(a.kp_count[2 * p])
        assert torch.equal(a.match_idx[p, :n], b.match_idx[p, :n])
    r = few.run_interleaved(PairPipeline.interleave(img[0::2], img[1::2]))
    with pytest.raises(RuntimeError, match='undecided'):        # the throughput entry reports instead of repeating
        few.check_converged()


class _MapNet:
    """Stand-in for a model inside PairPipeline.run_converged: returns prepared heat maps (image b's id is its first pixel) -- the
    default algorithm's maps, or the tie-exact twin's."""

    def __init__(self, maps, twin_maps=None, desc=None):
        self.maps, self.twin_maps, self.desc, self.calls = maps, twin_maps, desc, []

    def __call__(self, data):
        ids = data['image'][:, 0, 0, 0].round().long()
        self.calls.append(ids.tolist())
        return {'prob': self.maps.index_select(0, ids).clone(), 'logits': None, 'desc': self.desc.index_select(0, ids).clone()}

    def direct_twin(self):
        return _MapNet(self.twin_maps, None, self.desc) if self.twin_maps is not None else None


@pytest.mark.parametrize('topk', [0, 40])
def test_run_converged_reads_the_tie_guards_on_the_converged_pass(oracle, U, topk):
    """PairPipeline.run_converged (evaluation.py:224-285's loop head): the tie guards are read from the pass whose lists are
    returned -- after the NMS / capacity loop -- flagged images are redone with the tie-exact twin and settled again, and the
    running total a later check_converged() reports is drained.  Also with `topk: 0` (the shipped configs): the footprint guard."""
    from multipoint_amd.pipeline import PairPipeline
    rng = np.random.default_rng(5)
    H, W = 64, 640
    noise = _heat(rng, 1, H, W, 0.03)[0, 0]
    exact = np.zeros((H, W), dtype=np.float32); exact[8:56:2, 8:632:2] = 0.25                     # the reference's map: exact ties
    noisy = exact.copy(); noisy[exact > 0] += rng.random(int((exact > 0).sum())).astype(np.float32) * 4e-5     # ... seen through rounding noise
    # one round of NMS is not enough for this one (a chain of dependent decisions across 20 tiles; neighbours differ by >= 1e-4: no near-ties)
    ramp = (0.02 + 1e-3 * np.arange(W, dtype=np.float32)[None, :] + 1e-4 * np.arange(H, dtype=np.float32)[:, None]).astype(np.float32)
    auto = torch.from_numpy(np.stack([noise, noisy, ramp, noise])[:, None]).cuda()
    twin = torch.from_numpy(np.stack([noise, exact, ramp, noise])[:, None]).cuda()
    desc = torch.nn.functional.normalize(torch.rand(4, 64, H // 8, W // 8, device='cuda'), dim=1)
    img = torch.zeros(4, 1, H, W, device='cuda'); img[:, 0, 0, 0] = torch.arange(4, device='cuda')
    pred = {'nms': 4, 'detection_threshold': 0.015, 'topk': topk,
            'matching': {'method': 'bfmatcher', 'method_kwargs': {'crossCheck': True}, 'knn_matches': False}}
    net = _MapNet(auto, twin, desc)
    pipe = PairPipeline(net, pred, capacity=64 if topk == 0 else None, nms_rounds=1)      # (topk 0: the lists overflow and are regrown too)
    res = pipe.run_converged(img)
    assert pipe.tie_redone == 1 and net.calls == [[0, 1, 2, 3]]
    want = oracle.box_nms(twin.cpu().numpy(), 4, 0.015, keep_top_k=topk)
    for b in range(4):
        okp = oracle.keypoints_from_map(want[b, 0], 0.015)
        assert int(res.kp_count[b]) == len(okp) and np.array_equal(res.kp_yx[b, :len(okp)].cpu().numpy().astype(np.int64), okp)
    pipe.check_converged()
    assert pipe.tie_flagged == 0                               # nothing left over from the passes that were redone
    # the sensitivity is the caller's (PairPipeline.set_tie_guard): with both thresholds out of reach nothing is flagged -- the noisy
    # plateau holds near-ties, no exact ones for the cut to split -- and the defaults come back afterwards
    try:
        pipe.set_tie_guard(None, min_each_side=100000, min_pairs=10 ** 9)
        loose = PairPipeline(_MapNet(auto, twin, desc), pred, capacity=64 if topk == 0 else None, nms_rounds=1)
        loose.run_converged(img)
        # (top-k 40: among the plateau's ~1800 survivors in a window of 1300 float steps some are EXACTLY equal, and a cut that splits
        # such a pair is flagged whatever the thresholds)
        assert loose.tie_redone == 0 or topk > 0
    finally:
        pipe.set_tie_guard(None)
    again = PairPipeline(_MapNet(auto, twin, desc), pred, capacity=64 if topk == 0 else None, nms_rounds=1)
    again.run_converged(img)
    assert again.tie_redone == 1
    plain = PairPipeline(_MapNet(auto, None, desc), pred, capacity=64 if topk == 0 else None, nms_rounds=1, tie_robust=False)
    res = plain.run_converged(img)                             # without the guard: the noisy map's own lists
    want = oracle.box_nms(auto.cpu().numpy(), 4, 0.015, keep_top_k=topk)
    okp = oracle.keypoints_from_map(want[1, 0], 0.015)
    assert plain.tie_redone == 0 and np.array_equal(res.kp_yx[1, :len(okp)].cpu().numpy().astype(np.int64), okp)


def test_inputs_may_be_overwritten_after_run_interleaved(oracle, shipped):
    """The forward of run_interleaved runs on the pipeline's own stream; the caller's stream is ordered behind its reads of the
    input (PairResults.inputs_consumed is the same event for other streams): overwriting `images` in place right after the call
    must not change the results."""
    from multipoint_amd.pipeline import PairPipeline
    net, _ = shipped
    pred = {'nms': 4, 'detection_threshold': 0.015, 'topk': 300,
            'matching': {'method': 'bfmatcher', 'method_kwargs': {'crossCheck': True}, 'knn_matches': False}}
    pipe = PairPipeline(net, pred, capacity=512)
    clean = oracle.make_images(31, 8, 240, 320).cuda()
    ref = pipe.run_interleaved(clean.clone())
    pipe.check_converged()
    ref = (ref.kp_count.clone(), ref.kp_yx.clone(), ref.match_count.clone(), ref.match_idx.clone())
    side = torch.cuda.Stream()
    for trial in range(4):
        images = clean.clone()
        res = pipe.run_interleaved(images)
        assert res.inputs_consumed is not None
        if trial % 2 == 0:
            images.normal_()                                   # caller's stream: ordered behind the forward's reads
        else:
            with torch.cuda.stream(side):                      # another stream: waits for the event
                side.wait_event(res.inputs_consumed)
                images.zero_()
        pipe.check_converged()
        torch.cuda.synchronize()
        assert torch.equal(res.kp_count, ref[0]) and torch.equal(res.kp_yx, ref[1])
        assert torch.equal(res.match_count, ref[2]) and torch.equal(res.match_idx, ref[3])


# ------------------------------------------------------------------------------- sampling / matching
def test_interpolate_descriptors(oracle, U, golden_dir):
    g = np.load(os.path.join(golden_dir, 'sampling.npz'))                     # rows from the reference itself
    kp = torch.from_numpy(g['keypoints']).cuda()
    kp_before = kp.clone()
    rows = U.interpolate_descriptors(kp, torch.from_numpy(g['desc']).cuda(), int(g['H']), int(g['W']))
    assert torch.equal(kp, kp_before)
    assert rows.shape == g['rows'].shape
    assert np.abs(rows.cpu().numpy() - g['rows']).max() <= 1e-5
    rng = np.random.default_rng(3)
    d = rng.standard_normal((256, 12, 20)).astype(np.float32)                 # D = 256, odd map size
    kp = np.stack([rng.integers(0, 96, 77), rng.integers(0, 160, 77)], 1)
    out = U.interpolate_descriptors(torch.from_numpy(kp), torch.from_numpy(d), 96, 160)
    assert not out.is_cuda
    assert np.abs(out.numpy() - oracle.interpolate_descriptors(kp, d, 96, 160)).max() <= 1e-5
    assert U.interpolate_descriptors(torch.zeros(0, 2, dtype=torch.int64).cuda(), torch.from_numpy(d).cuda(), 96, 160).shape == (0, 256)


def _check_matches(oracle, m, d1, d2, thr):
    """Exact parity with the oracle except where the two best distances of a row/column are closer than
    fp32 summation noise (then either choice is a valid nearest neighbour)."""
    q, t, dist = oracle.nn_match(d1, d2, thr)
    gq = np.array([x.queryIdx for x in m], dtype=np.int64); gt = np.array([x.trainIdx for x in m], dtype=np.int64)
    gd = np.array([x.distance for x in m], dtype=np.float32)
    if np.array_equal(gq, q) and np.array_equal(gt, t):
        # d = sqrt(2 - 2 s): compare d^2 (near s = 1 the sqrt amplifies 1-ulp differences of s)
        assert np.abs(gd * gd - dist * dist).max(initial=0) <= 2e-6
        return 0
    dm = oracle.distance_matrix(d1, d2)
    srt_r = np.sort(dm, axis=1); srt_c = np.sort(dm, axis=0)
    amb_r = (srt_r[:, 1] - srt_r[:, 0]) < 1e-5 if dm.shape[1] > 1 else np.zeros(dm.shape[0], bool)
    amb_c = (srt_c[1] - srt_c[0]) < 1e-5 if dm.shape[0] > 1 else np.zeros(dm.shape[1], bool)
    a = set(zip(q.tolist(), t.tolist())); b = set(zip(gq.tolist(), gt.tolist()))
    for i, j in a ^ b:
        assert amb_r[i] or amb_c[j] or abs(dm[i, j] - (thr or 1e9)) < 1e-5, 'match (%d,%d) differs without a near-tie' % (i, j)
    return len(a ^ b)


def test_get_matches(oracle, U, golden_dir):
    g = np.load(os.path.join(golden_dir, 'matcher.npz'))                      # NNMatcher output of the reference
    m = U.get_matches(g['d1'], g['d2'], 'nnmatcher', False, threshold=float(g['threshold']))
    assert [x.queryIdx for x in m] == g['query'].tolist() and [x.trainIdx for x in m] == g['train'].tolist()
    assert np.abs(np.array([x.distance for x in m]) ** 2 - g['distance'] ** 2).max() <= 2e-6
    rng = np.random.default_rng(9)
    for n, k, D in [(1000, 1000, 64), (37, 513, 64), (300, 120, 256), (1, 1, 64), (64, 65, 128)]:
        d1 = rng.standard_normal((n, D)).astype(np.float32); d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
        d2 = rng.standard_normal((k, D)).astype(np.float32); d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
        d2[: min(n, k) // 2] = d1[: min(n, k) // 2]                           # exact duplicates: distance 0 ties
        _check_matches(oracle, U.get_matches(d1, d2, 'bfmatcher', False, crossCheck=True), d1, d2, None)
        _check_matches(oracle, U.get_matches(torch.from_numpy(d1).cuda(), torch.from_numpy(d2).cuda(), 'nnmatcher', False, threshold=0.9), d1, d2, 0.9)
    # cross-check restatement of cv2.BFMatcher agrees with the NNMatcher formula on unit descriptors
    q1, t1, _ = oracle.bf_match_crosscheck(d1, d2); q2, t2, _ = oracle.nn_match(d1, d2, None)
    assert len(set(zip(q1, t1)) ^ set(zip(q2, t2))) <= 2


# ------------------------------------------------------------------------------------ whole pipeline
def test_pipeline_matches_oracle_config1_shape(oracle, shipped):
    """BASELINE configs[0]: a single 240x320 pair through the whole path (+ a second pair)."""
    from multipoint_amd.pipeline import PairPipeline
    net, sd = shipped
    img = oracle.make_images(77, 4, 240, 320)
    pred = {'nms': 4, 'detection_threshold': 0.015, 'topk': 500,
            'matching': {'method': 'bfmatcher', 'method_kwargs': {'crossCheck': True}, 'knn_matches': False}}
    pipe = PairPipeline(net, pred, capacity=500)
    res = pipe(img[0::2].cuda(), img[1::2].cuda())
    pipe.check_converged()
    host = res.to_host()
    ref = oracle.process_pairs(sd, oracle.SHIPPED_MODEL_CONFIG, img[0::2], img[1::2], nms=4, detection_threshold=0.015, topk=500)
    for a, b in zip(ref, host):
        # end to end the GPU prob differs from the CPU prob by ~1e-5, so a keypoint may flip only where its
        # score is within that noise of a neighbour / the top-k boundary; on these seeds none flips
        assert np.array_equal(a['kp_optical'], b['kp_optical']) and np.array_equal(a['kp_thermal'], b['kp_thermal'])
        assert np.abs(a['desc_optical'] - b['desc_optical']).max() <= DESC_TOL
        assert np.abs(a['desc_thermal'] - b['desc_thermal']).max() <= DESC_TOL
        assert np.abs(np.linalg.norm(b['desc_optical'], axis=1) - 1).max() <= 1e-5

        class M:                                    # adapt to _check_matches
            def __init__(s, q, t, d): s.queryIdx, s.trainIdx, s.distance = q, t, d
        ms = [M(q, t, d) for q, t, d in zip(b['match_query'], b['match_train'], b['match_dist'])]
        _check_matches(oracle, ms, b['desc_optical'], b['desc_thermal'], None)


def test_full_size_properties(oracle, shipped, U):
    """BASELINE configs[2] size (32 pairs = 64 images 480x640, top-k 1000): properties that do not need
    the CPU oracle at this size."""
    from multipoint_amd.pipeline import PairPipeline
    from multipoint_amd.datasets import SyntheticPairs
    net, sd = shipped
    P = 32
    imgs = np.empty((2 * P, 1, 480, 640), dtype=np.float32)
    for p in range(P):
        imgs[2 * p], imgs[2 * p + 1] = SyntheticPairs.make_pair(0, p, 480, 640)
    images = torch.from_numpy(imgs).cuda()
    pred = {'nms': 4, 'detection_threshold': 0.015, 'topk': 1000,
            'matching': {'method': 'bfmatcher', 'method_kwargs': {'crossCheck': True}, 'knn_matches': False}}
    pipe = PairPipeline(net, pred, capacity=1000)
    res = pipe.run_interleaved(images)
    pipe.check_converged()
    out = net({'image': images})
    prob = out['prob']
    assert torch.isfinite(prob).all() and torch.isfinite(out['desc']).all()
    # softmax: 64 cell probabilities + dustbin sum to 1  =>  every 8x8 block sums to < 1
    blocks = prob.reshape(2 * P, 60, 8, 80, 8).sum(dim=(2, 4))
    assert (blocks <= 1 + 1e-5).all() and (prob >= 0).all()
    assert (out['desc'].pow(2).sum(1).sqrt() - 1).abs().max().item() <= 1e-5          # unit descriptors
    # NMS: idempotent, survivors keep their score, no two survivors inside each other's footprint, top-k exact
    nms1 = U.box_nms(prob, 4, 0.015, keep_top_k=1000)
    nms2 = U.box_nms(nms1, 4, 0.015, keep_top_k=1000)
    assert torch.equal(nms1, nms2)
    kept = nms1 > 0
    assert torch.equal(nms1[kept], prob[kept])
    assert (kept.flatten(1).sum(1) <= 1000).all()
    full = U.box_nms(prob, 4, 0.015)                                                     # without top-k
    k = (full > 0).float()
    foot = torch.zeros(1, 1, 7, 7, device='cuda')
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            if (4 - abs(dy)) * (4 - abs(dx)) >= 3 and (dy or dx):
                foot[0, 0, dy + 3, dx + 3] = 1
    neigh = torch.nn.functional.conv2d(k, foot, padding=3)
    assert ((neigh > 0) & (k > 0)).sum().item() == 0
    for b in (0, 17, 63):                                                                 # top-k = the k best survivors
        s_full = torch.sort(full[b][full[b] > 0], descending=True).values
        s_top = torch.sort(nms1[b][nms1[b] > 0], descending=True).values
        assert torch.equal(s_top, s_full[:1000])
    # keypoint lists == nonzero of the dense map, in row-major order
    K = res.kp_yx.shape[1]
    for b in (0, 33):
        n = min(int(res.kp_count[b]), K)
        nz = torch.nonzero(nms1[b, 0] > 0.015)
        assert torch.equal(res.kp_yx[b, :n].long(), nz)
    # matching: mutual + symmetric (swapping A and B gives the transposed match set)
    mi = res.match_idx
    cntA, cntB = res.kp_count[0::2].clamp(max=K), res.kp_count[1::2].clamp(max=K)
    swapped = U.match_pairs(res.desc[1::2].contiguous(), cntB.contiguous(), res.desc[0::2].contiguous(), cntA.contiguous())[0]
    for p in (0, 5, 31):
        fwd = {(i, int(j)) for i, j in enumerate(mi[p].tolist()) if j >= 0}
        bwd = {(int(i), j) for j, i in enumerate(swapped[p].tolist()) if i >= 0}
        assert fwd == bwd and len(fwd) == int(res.match_count[p])
        assert len({j for _, j in fwd}) == len(fwd)                                       # one-to-one


@pytest.mark.parametrize('mixed', [False, True])
def test_large_batch_index_range(oracle, mixed):
    """40 images 1024x1280: the 64-channel activation tensors hold 3.4e9 elements (> 2^31), so every kernel's
    addressing is exercised beyond 32 bits; images are independent, so the outputs of the last and the first image
    must equal the outputs of the same images run as a batch of two -- bit for bit."""
    cfg = dict(oracle.SHIPPED_MODEL_CONFIG); cfg['mixed_precision'] = mixed
    net, _ = _net(oracle, cfg)
    B = 40
    g = torch.Generator(device='cpu').manual_seed(9)
    two = torch.rand((2, 1, 1024, 1280), generator=g)
    images = torch.rand((B, 1, 1024, 1280), generator=g)
    images[0], images[B - 1] = two[0], two[1]
    ref = net({'image': two.cuda()})
    ref_prob, ref_desc = ref['prob'].clone(), ref['desc'].clone()
    out = net({'image': images.cuda()})
    assert torch.equal(out['prob'][0], ref_prob[0]) and torch.equal(out['prob'][B - 1], ref_prob[1])
    assert torch.equal(out['desc'][0], ref_desc[0]) and torch.equal(out['desc'][B - 1], ref_desc[1])
    assert torch.isfinite(out['prob']).all() and torch.isfinite(out['desc']).all()


# ----------------------------------------------------------------------------------------------------------------------
# the remaining get_matches modes (mp_match_knn2, mp_match_threshold; multipoint/utils/matching.py:4-33, 74-99)
# ----------------------------------------------------------------------------------------------------------------------
def _unit_rows(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@pytest.mark.parametrize('N,M,D', [(300, 257, 64), (1000, 1000, 64), (130, 77, 128), (65, 400, 256), (5, 1, 64)])
def test_bf_knn_and_ratio_test(oracle, N, M, D):
    import multipoint_amd.utils as U
    rng = np.random.default_rng(N + M + D)
    d1 = _unit_rows(rng, N, D)
    d2 = _unit_rows(rng, M, D)
    k = min(N, M) // 2
    d2[:k] = d1[:k] + 0.1 * rng.standard_normal((k, D)).astype(np.float32)         # true correspondences
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    if M >= 3:
        d2[2] = d2[1]                                                                 # an exact duplicate: index tie
    idx, dist = oracle.bf_knn(d1, d2, 2)
    nn = U.get_matches(torch.from_numpy(d1).to(DEV), d2, 'bfmatcher', crossCheck=False)
    assert [m.queryIdx for m in nn] == list(range(N))
    got = np.array([m.trainIdx for m in nn]); gd = np.array([m.distance for m in nn], np.float32)
    diff = d1[:, None, :] - d2[None, :, :]
    dm = np.sqrt((diff * diff).sum(-1))
    # nearest: same index unless the oracle's own best two are within fp32 noise of each other
    close = (np.partition(dm, 1, axis=1)[:, 1] - dm.min(1) < 1e-5) if M > 1 else np.zeros(N, bool)
    assert np.array_equal(got[~close], idx[~close, 0]) and np.abs(gd - dm[np.arange(N), got]).max() < 1e-5
    if M >= 3:
        assert not (got == 2).any()                                                   # the duplicate never beats index 1
    if M == 1:
        with pytest.raises(ValueError):                                               # `for m, n in all_matches` of the reference
            U.get_matches(d1, d2, 'bfmatcher', True)
        return
    m = U.get_matches(d1, d2, 'bfmatcher', True)
    q, t, d = oracle.bf_ratio_match(d1, d2)
    margin = np.abs(dist[:, 0] - 0.9 * dist[:, 1]) < 1e-5                              # ratio test on the fence
    sg = {(x.queryIdx, x.trainIdx) for x in m if not margin[x.queryIdx] and not close[x.queryIdx]}
    so = {(int(a), int(b)) for a, b in zip(q, t) if not margin[a] and not close[a]}
    assert sg == so and len(so) >= (1 if k else 0)
    assert [x.queryIdx for x in m] == sorted(x.queryIdx for x in m)


@pytest.mark.parametrize('N,M,D,thr', [(300, 257, 64, 0.7), (1000, 1000, 64, 0.5), (130, 77, 128, 1.2), (40, 90, 256, 0.9)])
def test_threshold_matcher(oracle, N, M, D, thr):
    import multipoint_amd.utils as U
    rng = np.random.default_rng(N * 7 + M)
    d1 = _unit_rows(rng, N, D)
    d2 = _unit_rows(rng, M, D)
    k = min(N, M) // 2
    d2[:k] = d1[:k] + 0.04 * rng.standard_normal((k, D)).astype(np.float32)
    d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    m = U.get_matches(d1, torch.from_numpy(d2).to(DEV), 'thresholdmatcher', threshold=thr)
    q, t, d = oracle.threshold_match(d1, d2, thr)
    dm = oracle.distance_matrix(d1, d2)
    fence = np.abs(dm - thr) < 1e-5
    sg = {(x.queryIdx, x.trainIdx) for x in m if not fence[x.queryIdx, x.trainIdx]}
    so = {(int(a), int(b)) for a, b in zip(q, t) if not fence[a, b]}
    assert sg == so and len(so) >= k // 2
    pairs = [(x.queryIdx, x.trainIdx) for x in m]
    assert pairs == sorted(pairs)                                                     # np.argwhere order
    # sqrt(2 - 2ab) amplifies the fp32 noise of the dot product as 1/d near d = 0
    assert max(abs(x.distance - dm[x.queryIdx, x.trainIdx]) * max(dm[x.queryIdx, x.trainIdx], 1e-3) for x in m) < 1e-6
    # a list larger than the first capacity guess: threshold 2.1 keeps every pair
    if N * M <= 40000:
        allm = U.get_matches(d1, d2, 'thresholdmatcher', threshold=2.1)
        assert len(allm) == N * M


# ------------------------------------------------------------------------------------------ machine shape
def test_machine_shape_is_derived_from_the_device():
    """mp_create sizes every persistent grid and the XCD split from the device (round-2 verdict, weak 8): the handle reports
    what it derived, and it equals what PyTorch reports for the same device -- no 256 / 8 constants."""
    from multipoint_amd import _lib
    h = _lib.Handle(0)
    ncu, nxcd, grid = h.device_shape()
    assert ncu == torch.cuda.get_device_properties(0).multi_processor_count
    assert nxcd >= 1 and nxcd & (nxcd - 1) == 0 and ncu % nxcd == 0
    assert grid == ncu // nxcd * nxcd


@pytest.mark.parametrize('shape', [('64', '2'), ('32', '1'), ('200', '8'), ('128', '4')])
@pytest.mark.parametrize('upd', [{}, {'mixed_precision': True}])
def test_smaller_machine_shapes_give_the_same_results(oracle, monkeypatch, shape, upd):
    """A partitioned or CU-masked device (MP_DEBUG=ncu= / nxcd= emulate one on the full chip): fewer persistent workgroups and
    another XCD split of the work items, bit-identical outputs -- every persistent kernel family (F(4x4,3x3) with the fused
    first block, the any-frame-size kernel on the deep 240x320 layers, the fused head tail, the fp16 kernels)."""
    from multipoint_amd import _lib
    cfg = dict(oracle.SHIPPED_MODEL_CONFIG); cfg.update(upd)
    img = oracle.make_images(77, 6, 240, 320).cuda()
    net, sd = _net(oracle, cfg, seed=3)
    full = net({'image': img})
    monkeypatch.setenv('MP_DEBUG', 'ncu=%s,nxcd=%s' % shape)
    assert _lib.Handle(0).device_shape()[:2] == (int(shape[0]), int(shape[1]))
    net2, _ = _net(oracle, cfg, seed=3)
    part = net2({'image': img})
    assert torch.equal(full['prob'], part['prob']) and torch.equal(full['desc'], part['desc'])


def test_unsupported_machine_shape_is_refused(monkeypatch):
    from multipoint_amd import _lib
    monkeypatch.setenv('MP_DEBUG', 'nxcd=3')
    with pytest.raises(_lib.MultiPointHipError, match='unsupported machine shape'):
        _lib.Handle(0)
