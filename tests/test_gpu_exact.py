"""GPU (MI355X): the HIP forward on weights and images where every rounding point is exact (oracle/exact_fixture.py; the premise is
checked on the CPU by tests/test_exact_fixture.py).  Every kernel that only multiplies and adds -- the direct fp32 family
(conv_mfma.hip: per-tile, persistent and fused-first-block launches; head_tail.hip) and the whole fp16 family (conv_first f16,
conv_f16.hip, conv_f16_res.hip, head_tail_f16.hip) -- must return the float64 logits and raw descriptors BIT FOR BIT, whatever its
summation order, with negative and zero BatchNorm scales in every layer.  A difference is a bug, reported with its coordinates.

prob and normalised descriptors are float64 functions of the exact logits / raw map, so they are held to fp32 rounding of the tails
alone (softmax with __expf in head_tail*.hip, expf in heads_post.hip; L2 normalisation), stated at PROB_REL / PROB_ABS / DESC_ABS.
The fp32 Winograd routings round inside their transforms: they keep the bars of tests/test_gpu_parity.py, measured against the
exact truth here."""
import numpy as np
import pytest
import torch

from oracle import exact_fixture as X

pytestmark = pytest.mark.gpu

# prob: relative error where the truth is >= 1e-6, absolute error elsewhere.  The softmax argument x - max is exact here; __expf is
# v_exp_f32(x * log2(e)), whose product rounds to half an ulp of |x| * log2(e) (2^-20 for prob >= 1e-6, |x| <= 14), a relative error
# of ln(2) * 2^-20 = 6.6e-7 in exp, plus the sum of 65 terms, the reciprocal and the product.  Observed on the MI355X, fused tails
# (head_tail*.hip, __expf): 1.3e-6 relative, 1.2e-12 absolute; separate launches (heads_post.hip, expf): 3.9e-7 / 3.6e-13.
PROB_REL = 2e-6
PROB_ABS = 2e-12
# normalised descriptors (components <= 1): the fp32 sum of squares, sqrt and division; one fp32 ulp of 1.0.  Observed: 7.1e-8.
DESC_ABS = 2.0 ** -23
# the bars of tests/test_gpu_parity.py for the Winograd routings (logits: test_force_return_logits)
PROB_TOL, DESC_TOL, LOGITS_TOL = 3e-5, 1e-5, 1e-4

DIRECT = [{'conv_algorithm': 'direct'}, ['', 'no_fuse', 'persist_min_items=1', 'no_persist', 'no_head_fuse']]
F16 = [{'mixed_precision': True}, ['', 'f16_no_fuse1', 'f16_no_res', 'f16_res_groups=2', 'no_head_fuse']]
MACHINE = ['ncu=32,nxcd=1', 'ncu=200,nxcd=8']
ROUTINGS = [('direct', DIRECT[0], e) for e in DIRECT[1] + MACHINE] + [('f16', F16[0], e) for e in F16[1] + MACHINE]

# (B, H, W, config): B = 1 and B > 2, partial tiles, a 1x1 deepest frame (zero padding: reflection needs 2 pixels), and frames on
# which pick_mbw (forward.hip) chooses each tile width 32 / 16 / 8 at the full-resolution layers (test_shapes_cover_every_tile_width)
SHAPES = [(2, 16, 16, 'shipped'), (1, 8, 8, 'zero_pad'), (3, 72, 104, 'shipped'), (5, 40, 264, 'shipped'), (1, 240, 320, 'shipped'),
          (2, 480, 640, 'shipped'), (2, 24, 2048, 'shipped'), (2, 64, 72, 'shipped'), (3, 48, 80, 'bn_first')]

_TRUTH = {}
_STATS = {}


def pick_mbw(H, W):
    """forward.hip pick_mbw: the tile width (tiles mbw x 256/mbw) with the least padded area, 32 on ties."""
    best, arg = None, 32
    for mbw in (32, 16, 8):
        th = 256 // mbw
        area = -(-H // th) * th * (-(-W // mbw) * mbw)
        if best is None or area < best:
            best, arg = area, mbw
    return arg


def _iso(B):
    return torch.tensor([[b % 2 == 0] for b in range(B)])


def _case(name, seed, B, H, W, spread='narrow', flat_last=True):
    """(cfg, sd, img, is_optical, truth), the truth computed once per (config, seed, shape, spread).  flat_last false: no flat image
    in the batch (exact_images makes image B - 1 flat, so a B = 1 case is ONE constant image, which cannot see where a kernel reads)."""
    key = (name, seed, B, H, W, spread, flat_last)
    if key not in _TRUTH:
        cfg = X.config(name)
        sd = X.exact_weights(seed, cfg, spread)
        img = X.exact_images(seed + 10 * H + W, B, H, W, flat_last=flat_last)
        iso = _iso(B) if cfg['multispectral'] else None
        t = X.truth(sd, img, cfg, is_optical=iso, fp32=B * H * W > 3 * 72 * 104)
        _TRUTH[key] = (cfg, sd, img, iso, t)
    return _TRUTH[key]


def _run(monkeypatch, cfg, sd, img, iso, env, upd):
    """logits + raw descriptors (force_return_logits, normalize_descriptors false) and prob + descriptors of a new handle."""
    import multipoint_amd.models as M
    if env:
        monkeypatch.setenv('MP_DEBUG', env)
    else:
        monkeypatch.delenv('MP_DEBUG', raising=False)
    data = {'image': img.cuda()}
    if iso is not None:
        data['is_optical'] = iso.cuda()
    out = {}
    for extra in ({'force_return_logits': True, 'normalize_descriptors': False}, {}):
        c = dict(cfg); c.update(upd); c.update(extra)
        net = M.MultiPoint(c); net.load_state_dict(sd); net.to('cuda'); net.eval()
        o = net(data)
        for k, v in o.items():
            if v is not None:
                out[k + ('_raw' if k == 'desc' and extra else '')] = v.cpu()
    monkeypatch.delenv('MP_DEBUG', raising=False)
    return out


def _where(got, want, n=6):
    """Count and first coordinates of the elements that differ."""
    bad = (got != want).nonzero()
    pts = [(tuple(int(i) for i in p), float(got[tuple(p)]), float(want[tuple(p)])) for p in bad[:n]]
    return '%d of %d differ; first (index, got, want): %s' % (bad.shape[0], got.numel(), pts)


def _check_exact(got, t, ctx):
    assert torch.equal(got['logits'], t['logits']), (ctx, 'logits', _where(got['logits'], t['logits']))
    if 'desc_raw' in t:
        assert torch.equal(got['desc_raw'], t['desc_raw']), (ctx, 'desc_raw', _where(got['desc_raw'], t['desc_raw']))


def _check_tails(got, t, ctx, tag, raw_desc=False):
    p, tp = got['prob'].double(), t['prob']
    big = tp >= 1e-6
    rel = float(((p - tp).abs() / tp.clamp_min(1e-300))[big].max()) if bool(big.any()) else 0.0
    ab = float((p - tp).abs()[~big].max()) if bool((~big).any()) else 0.0
    st = _STATS.setdefault(tag, {'prob_rel': 0.0, 'prob_abs_small': 0.0, 'desc_abs': 0.0})
    st['prob_rel'], st['prob_abs_small'] = max(st['prob_rel'], rel), max(st['prob_abs_small'], ab)
    assert rel <= PROB_REL and ab <= PROB_ABS, (ctx, 'prob', rel, ab)
    if 'desc' in t and not raw_desc:
        de = float((got['desc'].double() - t['desc']).abs().max())
        st['desc_abs'] = max(st['desc_abs'], de)
        assert de <= DESC_ABS, (ctx, 'desc', de)


def _tag(upd, env):
    return ('f16' if upd.get('mixed_precision') else 'fp32') + (' heads_post' if 'no_head_fuse' in env else ' head_tail')


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for k, v in sorted(_STATS.items()):
        print('\n[exact tails %s] max prob rel (truth >= 1e-6) %.3g, max prob abs (truth < 1e-6) %.3g, max desc abs %.3g'
              % (k, v['prob_rel'], v['prob_abs_small'], v['desc_abs']))


def test_shapes_cover_every_tile_width():
    assert {pick_mbw(H, W) for _, H, W, _ in SHAPES} == {32, 16, 8}
    assert {B for B, _, _, _ in SHAPES} >= {1, 2, 3, 5}


@pytest.mark.parametrize('B,H,W,name', SHAPES)
@pytest.mark.parametrize('fam,upd,env', ROUTINGS, ids=['%s:%s' % (f, e or 'default') for f, _, e in ROUTINGS])
def test_routings_are_bit_exact(monkeypatch, fam, upd, env, B, H, W, name):
    """Every direct fp32 and every fp16 launch (and two emulated machine shapes) on every shape: logits and raw descriptors
    equal the float64 forward; prob and descriptors within PROB_REL / PROB_ABS / DESC_ABS of float64 tails."""
    seed = (H + W) % 3
    for flat_last in ((True, False) if B == 1 else (True,)):            # B = 1: the flat image, and a non-flat one
        cfg, sd, img, iso, t = _case(name, seed, B, H, W, flat_last=flat_last)
        got = _run(monkeypatch, cfg, sd, img, iso, env, upd)
        ctx = (fam, env, name, seed, B, H, W, flat_last)
        _check_exact(got, t, ctx)
        _check_tails(got, t, ctx, _tag(upd, env))


@pytest.mark.parametrize('name', list(X.CONFIGS))
@pytest.mark.parametrize('fam', ['direct', 'f16'])
def test_model_configs_are_bit_exact(monkeypatch, name, fam):
    """Every model variant (multispectral with mixed is_optical) on the three seeds whose filters cover every (channel, tap)."""
    upd = DIRECT[0] if fam == 'direct' else F16[0]
    for seed in X.SEEDS:
        cfg, sd, img, iso, t = _case(name, seed, 3, 40, 56)
        got = _run(monkeypatch, cfg, sd, img, iso, '', upd)
        ctx = (fam, name, seed)
        _check_exact(got, t, ctx)
        raw = not cfg['normalize_descriptors']
        if raw:
            assert torch.equal(got['desc'], t['desc_raw']), ctx
        _check_tails(got, t, ctx, _tag(upd, ''), raw_desc=raw)


@pytest.mark.parametrize('env', ['', 'no_head_fuse'])
@pytest.mark.parametrize('fam', ['direct', 'f16'])
def test_wide_logits(monkeypatch, fam, env):
    """Logits up to about 200 (softmax arguments far below -30): the fused tail's __expf and heads_post's expf against float64."""
    upd = DIRECT[0] if fam == 'direct' else F16[0]
    reach = 0.0
    for seed in X.SEEDS:
        cfg, sd, img, iso, t = _case('shipped', seed, 2, 120, 160, spread='wide')
        lg = t['logits']
        reach = max(reach, float(lg.abs().max()))
        got = _run(monkeypatch, cfg, sd, img, iso, env, upd)
        ctx = (fam, env, seed)
        _check_exact(got, t, ctx)
        _check_tails(got, t, ctx, _tag(upd, env) + ' wide')
    assert reach >= 100


def test_superpoint_magicleap_direct():
    """SuperPointMagicLeap (zero padding, no BatchNorm, exp / (sum + 1e-5)) with conv_algorithm direct: logits bit for bit, prob and
    descriptors (divided by their norm) within the tails' bounds of float64."""
    import multipoint_amd.models as M
    for seed in X.SEEDS:
        sd = X.exact_weights_magicleap(seed)
        img = X.exact_images(seed + 5, 2, 64, 96)
        t = X.magicleap64(sd, img)
        net = M.SuperPointMagicLeap({'conv_algorithm': 'direct'}); net.load_state_dict(sd); net.to('cuda'); net.eval()
        out = net({'image': img.cuda()})
        lg = out['logits'].cpu()
        assert torch.equal(lg.double(), t['logits']), (seed, _where(lg.double(), t['logits']))
        got = {'prob': out['prob'].cpu(), 'desc': out['desc'].cpu()}
        want = {'prob': t['prob'].double(), 'desc': t['desc']}
        # an all-zero descriptor divides 0 by 0 in the reference: NaN on both sides
        nan = torch.isnan(want['desc'])
        assert torch.equal(torch.isnan(got['desc']), nan), seed
        got['desc'][nan], want['desc'][nan] = 0, 0
        _check_tails(got, want, ('magicleap', seed), 'fp32 magicleap')


@pytest.mark.parametrize('fam', ['direct', 'f16'])
def test_large_batch_index_range_is_exact(monkeypatch, fam):
    """40 images 1024x1280 (activation tensors past 2^31 elements): the first and the last image equal the exact truth bit for bit."""
    upd = DIRECT[0] if fam == 'direct' else F16[0]
    key = ('large',)
    cfg = X.config('shipped')
    if key not in _TRUTH:
        sd = X.exact_weights(1, cfg)
        two = X.exact_images(21, 2, 1024, 1280)
        _TRUTH[key] = (sd, two, X.truth(sd, two, cfg, fp32=True))
    sd, two, t = _TRUTH[key]
    B = 40
    images = (torch.from_numpy(np.random.default_rng(22).integers(0, 9, size=(B, 1, 1024, 1280)).astype(np.float32)) / 8.0)
    images[0], images[B - 1] = two[0], two[1]
    monkeypatch.delenv('MP_DEBUG', raising=False)
    import multipoint_amd.models as M
    c = dict(cfg); c.update(upd); c.update({'force_return_logits': True, 'normalize_descriptors': False})
    net = M.MultiPoint(c); net.load_state_dict(sd); net.to('cuda'); net.eval()
    out = net({'image': images.cuda()})
    for i, j in ((0, 0), (B - 1, 1)):
        lg, d = out['logits'][i].cpu(), out['desc'][i].cpu()
        assert torch.equal(lg, t['logits'][j]), (fam, i, _where(lg, t['logits'][j]))
        assert torch.equal(d, t['desc_raw'][j]), (fam, i, _where(d, t['desc_raw'][j]))
    del out, images


@pytest.mark.parametrize('env,B,H,W', [('', 2, 240, 320), ('', 1, 88, 120), ('', 3, 72, 104), ('wino43_gen=2', 2, 240, 320),
                                       ('wino43_gen=2', 1, 88, 120), ('wino43_gen=2', 3, 40, 56)])
def test_winograd_routings_against_exact_truth(monkeypatch, env, B, H, W):
    """The fp32 Winograd routings (default, the any-frame kernel everywhere, split input channels at B <= 2) round inside their
    transforms: the existing bars of tests/test_gpu_parity.py, measured against the exact truth."""
    seed = W % 3
    for flat_last in ((True, False) if B == 1 else (True,)):            # B = 1: the flat image, and a non-flat one
        cfg, sd, img, iso, t = _case('shipped', seed, B, H, W, flat_last=flat_last)
        got = _run(monkeypatch, cfg, sd, img, iso, env, {})
        assert float((got['logits'] - t['logits']).abs().max()) <= LOGITS_TOL, flat_last
        assert float((got['prob'].double() - t['prob']).abs().max()) <= PROB_TOL, flat_last
        assert float((got['desc'].double() - t['desc']).abs().max()) <= DESC_TOL, flat_last
