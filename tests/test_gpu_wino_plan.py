"""GPU (MI355X): the fp32 Winograd forward on every launch class its plan can take (tests/wino_plan_restatement.py lists the
classes and the cases, tests/test_wino_plan_host.py proves the coverage on the CPU).  The library's own plan (mp_forward_plan) must
equal the restatement; every case is held to the float64 truth of the exact fixture at the bars of tests/test_gpu_exact.py;
handles whose plans differ only in layouts, the pre-transformed input, workgroups or the XCD split must agree bit for bit."""
import pytest
import torch

import wino_plan_restatement as R
from oracle import exact_fixture as X
from oracle import mp_oracle as O
from test_gpu_exact import DESC_TOL, LOGITS_TOL, PROB_TOL
from test_wino_plan_host import all_cases

pytestmark = pytest.mark.gpu

_TRUTH = {}
_STATS = {}
IDS = ['%s:%dx%dx%d:gen%d' % ((n,) + c) for n, c in all_cases()]
SHIPPED3 = [c for c in R.CASES if c[0] >= 3]


def _case(name, case, seed=None):
    """(cfg, sd, img, is_optical, truth) of a case, the truth computed once."""
    B, H, W, _ = case
    seed = (H + W) % 3 if seed is None else seed
    key = (name, case, seed)
    if key not in _TRUTH:
        cfg = X.config(name)
        sd = R.case_weights(seed, name, case)
        img = R.case_images(seed, name, case)
        iso = R.is_optical(O.full_config(cfg), B)
        _TRUTH[key] = (cfg, sd, img, iso, R.case_truth(sd, img, name, case, iso))
    return _TRUTH[key]


def _env(case, extra=''):
    return ','.join(t for t in (R.ROUTINGS[case[3]], extra) if t)


def _net(monkeypatch, cfg, sd, env, **upd):
    import multipoint_amd.models as M
    if env:
        monkeypatch.setenv('MP_DEBUG', env)
    else:
        monkeypatch.delenv('MP_DEBUG', raising=False)
    c = dict(cfg); c.update(upd)
    net = M.MultiPoint(c); net.load_state_dict(sd); net.to('cuda'); net.eval()
    monkeypatch.delenv('MP_DEBUG', raising=False)
    return net


def _fwd(net, img, iso):
    data = {'image': img.cuda()}
    if iso is not None:
        data['is_optical'] = iso.cuda()
    return {k: v.cpu() for k, v in net(data).items() if v is not None}


def _where(name, case, env, err):
    """The worst element of an error map (B, C, h, w) at H/8 or (B, 1, H, W), and the tile block of each launch it lies in."""
    B, H, W, _ = case
    idx = [int(i) for i in (err == err.max()).nonzero()[0]]
    y, x = idx[-2], idx[-1]
    scale = 8 if err.shape[-2] == H // 8 and err.shape[-2] != H else 1
    out = []
    for r in R.case_plan(name, case, env):
        if r['kernel'] in R.WINO:
            f = max(1, H // r['H'])
            out.append((r['name'], r['kernel'], r['tc4']) + R.block_of(r, y * scale // f, x * scale // f))
    return 'worst %.3g at %s; (launch, kernel, tc4, block row, block column, tile row, tile column): %s' % (float(err.max()), idx, out)


def _check_truth(got, t, name, case, env, tag):
    st = _STATS.setdefault(tag, {'logits': 0.0, 'prob': 0.0, 'desc': 0.0})
    bars = {'logits': LOGITS_TOL, 'prob': PROB_TOL, 'desc': DESC_TOL}
    errs = {k: (got[k].double() - t[k].double()).abs() for k in bars if k in got and k in t}
    for k, e in errs.items():
        assert not bool(torch.isnan(got[k]).any()), (name, case, env, k, 'NaN')
        st[k] = max(st[k], float(e.max()))
        print('[wino plan %s %s %s] %s err %.3g' % (name, case, env or 'default', k, float(e.max())))
    for k, e in errs.items():
        assert float(e.max()) <= bars[k], (name, case, env, k, _where(name, case, env, e))


def _both(monkeypatch, cfg, sd, img, iso, env):
    """logits (force_return_logits) and prob + descriptors of new handles."""
    out = _fwd(_net(monkeypatch, cfg, sd, env, force_return_logits=True), img, iso)
    got = {'logits': out['logits']}
    net = _net(monkeypatch, cfg, sd, env)
    o = _fwd(net, img, iso)
    got['prob'], got['desc'] = o['prob'], o.get('desc')
    if got['desc'] is None:
        del got['desc']
    return got, net


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for k, v in sorted(_STATS.items()):
        print('\n[wino plan %s] max logits err %.3g, max prob err %.3g, max desc err %.3g' % (k, v['logits'], v['prob'], v['desc']))


_DEVICE = []


def _device_shape(net):
    ncu, nxcd, _ = net._handle.device_shape()
    return ncu, nxcd


def _device(monkeypatch):
    """(compute units, XCDs) of the device, without MP_DEBUG overrides."""
    if not _DEVICE:
        cfg = X.config('shipped')
        _DEVICE.append(_device_shape(_net(monkeypatch, cfg, X.exact_weights(0, cfg), '')))
    return _DEVICE[0]


@pytest.mark.parametrize('name,case', all_cases(), ids=IDS)
def test_plan_equals_the_restatement(monkeypatch, name, case):
    """mp_forward_plan against the restated planner for the case's routing, the layout / VIN switches and the emulated machines,
    with the CU / XCD counts the handle reports."""
    cfg, sd, img, iso, _ = _case(name, case)
    B, H, W, _ = case
    full = O.full_config(cfg)
    for extra in ('', 'no_planar', 'no_xplanar', 'no_vin') + R.EMULATED:
        env = _env(case, extra)
        net = _net(monkeypatch, cfg, sd, env)
        real = net._handle.forward_plan(B, H, W, R.n_optical(full, B))
        want = R.plan(full, B, H, W, env, R.n_optical(full, B), device=_device(monkeypatch))
        assert _device_shape(net) == R.machine(env, _device(monkeypatch)), env
        assert real == want, (name, case, env, [(a, b) for a, b in zip(real, want) if a != b])


def test_real_plans_cover_the_universe(monkeypatch):
    """The coverage assertion of tests/test_wino_plan_host.py on the library's own plans."""
    cfg = X.config('shipped')
    sd = X.exact_weights(0, cfg)
    full = O.full_config(cfg)
    got, walks = set(), set()
    for case in R.CASES + R.IDENTITY_CASES:
        B, H, W, _ = case
        got |= R.classes(_net(monkeypatch, cfg, sd, _env(case))._handle.forward_plan(B, H, W), full)
        if B >= 3:
            for e in R.EMULATED:
                walks |= R.walk_classes(_net(monkeypatch, cfg, sd, _env(case, e))._handle.forward_plan(B, H, W), R.machine(e)[1])
    zcfg = X.config('zero_pad')
    zsd = X.exact_weights(0, zcfg)
    for case in R.CONFIG_CASES['zero_pad']:
        B, H, W, _ = case
        real = _net(monkeypatch, zcfg, zsd, _env(case))._handle.forward_plan(B, H, W)
        got |= {c for c in R.classes(real, O.full_config(zcfg)) if c == ('f', 'direct_1x1_zero_pad')}
    from test_wino_plan_host import UNREACHABLE_WALKS
    u = R.universe()
    assert not [c for c in u if c not in got], [c for c in u if c not in got]
    assert not (R.walk_universe() - UNREACHABLE_WALKS - walks)


@pytest.mark.parametrize('name,case', all_cases(), ids=IDS)
def test_cases_against_the_exact_truth(monkeypatch, name, case):
    """Logits, prob and descriptors of every case within the bars of tests/test_gpu_exact.py of the float64 truth, on every seed of
    X.SEEDS (tests/test_wino_plan_host.py shows each geometric error on SOME seed); three runs of one handle are bit-identical."""
    env = _env(case)
    for seed in X.SEEDS:
        cfg, sd, img, iso, t = _case(name, case, seed)
        got, net = _both(monkeypatch, cfg, sd, img, iso, env)
        _check_truth(got, t, name, case, env, '%s %s' % (name, env or 'default'))
    for _ in range(2):
        again = _fwd(net, img, iso)
        assert torch.equal(again['prob'], got['prob']), (name, case, 'prob differs between runs of one handle')
        if 'desc' in got:
            assert torch.equal(again['desc'], got['desc']), (name, case, 'desc differs between runs of one handle')


@pytest.mark.parametrize('name,case', all_cases(), ids=IDS)
def test_layouts_vin_and_machines_change_no_bit(monkeypatch, name, case):
    """no_planar, no_xplanar and no_vin change layouts and the input transform's place, never a bit.  The emulated machines change
    workgroups and the XCD split alone at B >= 3 (bit-identical); at B <= 2 they change the split of the input channels too, and
    those results are held to the truth at the bars."""
    cfg, sd, img, iso, t = _case(name, case)
    base = _fwd(_net(monkeypatch, cfg, sd, _env(case)), img, iso)
    exact = ['no_planar', 'no_xplanar', 'no_vin'] + (list(R.EMULATED) if case[0] >= 3 else [])
    for extra in exact:
        o = _fwd(_net(monkeypatch, cfg, sd, _env(case, extra)), img, iso)
        for k in ('prob', 'desc'):
            if k in base:
                assert torch.equal(o[k], base[k]), (name, case, extra, k, int((o[k] != base[k]).sum()))
    if case[0] <= 2:
        for extra in R.EMULATED:
            env = _env(case, extra)
            got, _ = _both(monkeypatch, cfg, sd, img, iso, env)
            _check_truth(got, t, name, case, env, '%s %s emulated' % (name, R.ROUTINGS[case[3]] or 'default'))


@pytest.mark.parametrize('name,case', [('shipped', c) for c in SHIPPED3] + [('multispectral', (3, 32, 32, 0))])
def test_batch_invariance(monkeypatch, name, case):
    """Permuting the images permutes the outputs bit for bit, and an image has the same bits in a batch of 3 and of 5 (B >= 3
    never splits the input channels), also with two encoders."""
    cfg, sd, img, iso, _ = _case(name, case)
    net = _net(monkeypatch, cfg, sd, _env(case))
    base = _fwd(net, img, iso)
    perm = [2, 0, 1]
    o = _fwd(net, img[perm], None if iso is None else iso[perm])
    for k in ('prob', 'desc'):
        assert torch.equal(o[k], base[k][perm]), (name, case, 'permutation', k)
    B, H, W, _ = case
    more = X.exact_images(77, 2, H, W, flat_last=False)
    img5 = torch.cat([img[:1], more[:1], img[1:], more[1:]])
    iso5 = None if iso is None else torch.cat([iso[:1], torch.tensor([[True]]), iso[1:], torch.tensor([[False]])])
    o5 = _fwd(net, img5, iso5)
    for k in ('prob', 'desc'):
        assert torch.equal(o5[k][[0, 2, 3]], base[k]), (name, case, 'batch of 5', k)


# a split case (B = 1, input channels in ranges), a pre-transformed-input case (B = 3, conv_wino43.hip heads) and a partial-block
# any-frame case
STALE = [(1, 96, 32, 0), (3, 32, 96, 0), (1, 104, 184, 2)]


@pytest.mark.parametrize('case', STALE)
def test_stale_workspace_cannot_reach_an_output(monkeypatch, case):
    """A handle that ran a LARGER frame of NaN images, then of large finite images, returns a fresh handle's bits on the case: no
    launch reads what an earlier forward left in the activation, split or pre-transformed-input workspaces."""
    assert case in R.CASES
    p = R.case_plan('shipped', case)
    assert {(1, 96, 32, 0): any(r['ks_shift'] for r in p), (3, 32, 96, 0): bool(p[-1]['vin']),
            (1, 104, 184, 2): any(R.last_partial_block(r) for r in p if r['kernel'] == 'wino43b')}[case]
    cfg, sd, img, iso, _ = _case('shipped', case)
    B, H, W, _ = case
    fresh = _fwd(_net(monkeypatch, cfg, sd, _env(case)), img, iso)
    net = _net(monkeypatch, cfg, sd, _env(case))
    big = (B, 1, H + 16, W + 24)
    for fill, dirty in (('NaN', torch.full(big, float('nan'))), ('large', 2e3 * torch.rand(big, generator=torch.Generator().manual_seed(5)) - 1e3)):
        _fwd(net, dirty, None)
        o = _fwd(net, img, iso)
        for k in ('prob', 'desc'):
            assert bool(torch.isfinite(o[k]).all()), (case, fill, k)
            assert torch.equal(o[k], fresh[k]), (case, fill, k, int((o[k] != fresh[k]).sum()))
