"""Batch-statistics (training-mode) forward on the GPU, on every launch and tile shape it can take: mp_forward_batch_stats /
MultiPoint.set_batch_statistics(True) against the float64 restatement (tests/batch_stats_restatement.py) with the bars of
tests/test_gpu_batch_stats.py, unchanged.

What the shapes and routings below reach, and tests/test_gpu_batch_stats.py (one 24 x 32 frame, no MP_DEBUG) does not:
  * every tile width (32 / 16 / 8) of the direct kernels at every encoder resolution and at the heads, with partial tiles at the
    right and bottom edges (test_shapes_reach_every_tile_width_at_every_level);
  * the persistent kernels -- identity epilogue and, for bn_first models, LINEAR -- at every tile width, on two emulated machine
    shapes whose workgroups walk several items and a tail (test_routings_sit_on_their_side_of_the_persistence_gate);
  * a second trip through bn_apply_kernel's row loop and a capped, uneven split of the pixels over the statistics partials
    (test_more_than_65535_rows);
  * the optional outputs of the C ABI on accepted calls (test_optional_outputs_of_the_c_abi);
  * workspace memory that is read but never written (test_stale_workspace_cannot_reach_an_output).

Per-tile against persistent: conv_mfma_persist_kernel multiplies a chunk's k-steps in the per-tile kernel's order and both add
the bias to the finished sum in the epilogue, so every routing must return the same bits; the tests assert torch.equal between
all routings of a case, not only between the two machine shapes."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import batch_stats_restatement as R  # noqa: E402
from test_gpu_batch_stats import DEV, TOL_DESC, TOL_LOGITS, TOL_STATS, _data, _net  # noqa: E402
from test_gpu_exact import pick_mbw  # noqa: E402

pytestmark = pytest.mark.gpu

# (B, H, W): together they reach tile widths 32, 16 and 8 at each of the four encoder resolutions and at the heads, and each has
# a partial tile on some level (test_shapes_reach_every_tile_width_at_every_level)
SHAPES = [(3, 72, 104), (3, 136, 40), (2, 264, 40), (5, 40, 264), (3, 200, 24)]
EXPECTED_MBW = {(3, 72, 104): (16, 32, 32, 16, 16), (3, 136, 40): (8, 32, 16, 8, 8), (2, 264, 40): (8, 8, 16, 8, 8),
                (5, 40, 264): (32, 32, 16, 32, 32), (3, 200, 24): (8, 16, 8, 8, 8)}
ROUTES = {2: [1, 0], 3: [1, 0, 1], 5: [1, 0, 0, 1, 0]}          # uneven: the encoders see different numbers of images

CONFIGS = {
    'shipped': {},
    'bn_first': {'bn_first': True},                                  # the LINEAR kernels
    'ms_bn_first': {'multispectral': True, 'bn_first': True},        # gather, scatter through out_list, statistics of a subset
    'bn_first_v2_zero': {'bn_first': True, 'channel_version': 2, 'reflection_pad': False},    # padding channels in every tensor
    'many_rows': {'reflection_pad': False, 'bn_first': True},
    'd256': {'descriptor_size': 256},
    'channel_v1': {'channel_version': 1, 'descriptor_size': 128},
    'channel_v2_bn_first': {'channel_version': 2, 'bn_first': True},
}
CASES = [(name, shape) for shape in SHAPES for name in ('shipped', 'bn_first', 'ms_bn_first')] + [('bn_first_v2_zero', (3, 136, 40))]
MANY_ROWS = (33, 2048, 8)
MANY_ROWS_SEED = 5

# routings: MP_DEBUG of a new handle.  The default launches every 3x3 layer of SHAPES per tile; the two emulated machine shapes
# make every one of them persistent, four (six, in two XCD ranges) workgroups walking several items and a tail each.
PER_TILE = ''
MACHINE = ['persist_min_items=1,ncu=4,nxcd=1', 'persist_min_items=1,ncu=6,nxcd=2']
# an encoder of the multispectral model that received ONE image has 2 items at its deepest level, and the 64-channel deepest
# level of channel version 2 has 3 for the whole batch, fewer than 4 or 6 workgroups: two-workgroup machines put those launches
# on the persistent side as well
FEW_ITEMS = ('ms_bn_first', 'bn_first_v2_zero')
MACHINE_SMALL = ['persist_min_items=1,ncu=2,nxcd=1', 'persist_min_items=1,ncu=2,nxcd=2']
PERSIST_DEFAULT = 8                                                  # host.h DebugSwitches::persist

STAGE_CHANNELS = {0: (64, 64, 128, 128), 1: (32, 64, 96, 128), 2: (8, 16, 32, 64)}     # MultiPoint.py:38-53

_REF = {}
_ERRORS = {}


def _seed(name, shape):
    return MANY_ROWS_SEED if name == 'many_rows' else 3 + sum(shape) % 7


def _case(name, shape):
    """(cfg, sd, img, is_optical, (logits64, desc64, stats64)): weights, input and the float64 restatement, once per case."""
    key = (name, shape)
    if key not in _REF:
        B, H, W = shape
        case = (name, CONFIGS[name], B, H, W, ROUTES[B] if CONFIGS[name].get('multispectral') else None)
        cfg, seed = R.case_config(case), _seed(name, shape)
        sd = R.case_weights(case, seed)
        img, opt = R.case_inputs(case, seed)
        torch.set_num_threads(min(16, torch.get_num_threads()))
        _REF[key] = (cfg, sd, img, opt, R.forward_train64(sd, img, cfg, opt))
    return _REF[key]


def _levels(H, W):
    """(h, w) of the four encoder resolutions and of the heads."""
    return [(H >> l, W >> l) for l in range(4)] + [(H // 8, W // 8)]


def _debug(env):
    out = {}
    for tok in env.split(','):
        k, eq, v = tok.partition('=')
        if k:
            out[k] = int(v) if eq else 1
    return out


def conv3x3_launches(cfg, B, H, W, route=None):
    """[(name, images, h, w, slices)] of the 3x3 MFMA launches of the batch-statistics forward (forward.hip
    run_forward_batch_stats): enc.conv2 .. enc.conv8 of every encoder that received images, and both heads' 3x3 convolutions in
    one launch.  (enc.conv1 has one input channel and its own kernel.)"""
    cfg = R.O.full_config(cfg)
    assert cfg['double_convolution']
    st = STAGE_CHANNELS[cfg['channel_version']]
    couts = [st[0], st[1], st[1], st[2], st[2], st[3], st[3]]
    level = [0, 1, 1, 2, 2, 3, 3]
    if cfg.get('multispectral'):
        encoders = [('thermal.', len(route) - sum(route)), ('optical.', sum(route))]
    else:
        encoders = [('', B)]
    out = []
    for tag, nb in encoders:
        if nb:
            out += [('%senc.conv%d' % (tag, i + 2), nb, H >> level[i], W >> level[i], -(-couts[i] // 64)) for i in range(7)]
    hc = 256 if cfg['channel_version'] == 0 else cfg['descriptor_size']
    out.append(('heads.conv3x3', B, H // 8, W // 8, -(-(hc * (2 if cfg['descriptor_head'] else 1)) // 64)))
    return out


def persistent_launches(cfg, B, H, W, route, ncu, persist):
    """conv_mfma.hip launch_t: {launch: persistent?}, persistent when persist > 0 and nblk >= ncu * persist,
    nblk = images * tiles_x * tiles_y * slices."""
    out = {}
    for name, nb, h, w, slices in conv3x3_launches(cfg, B, H, W, route):
        mbw = pick_mbw(h, w)
        nblk = nb * -(-w // mbw) * -(-h // (256 // mbw)) * slices
        out[name] = bool(persist) and nblk >= ncu * persist
    return out


def _gate(cfg, shape, route, env, device_cus):
    """persistent_launches() of a handle created under MP_DEBUG=env on a device of device_cus compute units (api.hip mp_create:
    ncu=N is taken when 0 < N <= the device's)."""
    d = _debug(env)
    ncu = d['ncu'] if 0 < d.get('ncu', 0) <= device_cus else device_cus
    persist = 0 if 'no_persist' in d else d.get('persist_min_items', PERSIST_DEFAULT)
    return ncu, persistent_launches(cfg, *shape, route, ncu, persist)


def _routings(name):
    return [PER_TILE] + MACHINE + (MACHINE_SMALL if name in FEW_ITEMS else [])


def _check_gate(name, cfg, shape, route, env, device_cus):
    """Every 3x3 launch of the case is on the side of the persistence gate that routing `env` is there to test."""
    ncu, sides = _gate(cfg, shape, route, env, device_cus)
    if env == PER_TILE or 'no_persist' in env:
        assert not any(sides.values()), (name, shape, env, ncu, sides)
    elif name not in FEW_ITEMS or env in MACHINE_SMALL:
        assert all(sides.values()), (name, shape, env, ncu, sides)
    else:
        # at least the heads' launch over the whole batch and the full-resolution launch of each encoder
        assert all(v for k, v in sides.items() if k == 'heads.conv3x3' or k.endswith('enc.conv2')), (name, shape, env, ncu, sides)
    return ncu


def test_shapes_reach_every_tile_width_at_every_level():
    """Runs without a GPU.  pick_mbw (forward.hip) over the shape list: tile widths {32, 16, 8} at each of the four encoder
    resolutions and at the heads; every shape has a partial tile on some level; more than one block everywhere."""
    for shape in SHAPES:
        assert tuple(pick_mbw(h, w) for h, w in _levels(*shape[1:])) == EXPECTED_MBW[shape], shape
    for l in range(5):
        assert {EXPECTED_MBW[s][l] for s in SHAPES} == {32, 16, 8}, l
    for B, H, W in SHAPES:
        partial = [(h, w) for h, w in _levels(H, W) if w % pick_mbw(h, w) or h % (256 // pick_mbw(h, w))]
        assert partial, (B, H, W)
    # the LINEAR case with padding channels takes the 8-wide tile at full resolution and at the heads
    assert EXPECTED_MBW[(3, 136, 40)][0] == 8 and EXPECTED_MBW[(3, 136, 40)][4] == 8
    assert {B for B, _, _ in SHAPES} == {2, 3, 5}


@pytest.mark.parametrize('device_cus', [32, 64, 128, 256])
def test_routings_sit_on_their_side_of_the_persistence_gate(device_cus):
    """Runs without a GPU, for the compute-unit counts of an MI355X and its partitions (the GPU tests repeat the check with the
    handle's own device_shape()): the default handle launches every 3x3 layer of every case per tile, the emulated machines
    launch every one persistently, each workgroup walking more than one item somewhere."""
    for name, shape in CASES:
        cfg = R.case_config((name, CONFIGS[name]))
        route = ROUTES[shape[0]] if cfg.get('multispectral') else None
        for env in _routings(name):
            ncu = _check_gate(name, cfg, shape, route, env, device_cus)
            if env != PER_TILE:
                items = [nb * -(-w // pick_mbw(h, w)) * -(-h // (256 // pick_mbw(h, w))) * s
                         for _, nb, h, w, s in conv3x3_launches(cfg, *shape, route)]
                assert max(items) >= 3 * ncu and any(i % ncu for i in items), (name, shape, env, items)
    cfg = R.case_config(('many_rows', CONFIGS['many_rows']))
    for env in ['no_persist'] + MACHINE:
        _check_gate('many_rows', cfg, MANY_ROWS, None, env, device_cus)


def _run(monkeypatch, cfg, sd, img, opt, env):
    """Outputs and statistics of a new model (a new handle reads MP_DEBUG) on the host, and the handle's compute units."""
    if env:
        monkeypatch.setenv('MP_DEBUG', env)
    else:
        monkeypatch.delenv('MP_DEBUG', raising=False)
    net = _net(cfg, sd)
    monkeypatch.delenv('MP_DEBUG', raising=False)
    net.set_batch_statistics(True)
    with torch.no_grad():
        out = net(_data(img, opt))
    stats = {p: (m.cpu(), v.cpu()) for p, (m, v) in net.last_batch_statistics().items()}
    return {'logits': out['logits'].cpu(), 'desc': out['desc'].cpu(), 'stats': stats, 'ncu': net._handle.device_shape()[0]}


def _device_cus():
    from multipoint_amd import _lib
    return _lib.Handle(torch.device(DEV).index).device_shape()[0]


def _check_restatement(got, ref, ctx, tag):
    """The bars of tests/test_gpu_batch_stats.py; the statistics first (the per-layer probe), the first layer out of bounds named
    by its state_dict prefix."""
    l64, d64, st64 = ref
    assert list(got['stats']) == list(st64), ctx
    worst = 0.0
    for p, (m64, v64) in st64.items():
        m, v = (t.double() for t in got['stats'][p])
        scale = 1 + max(float(m64.abs().max()), float(v64.abs().max()))
        em, ev = float((m - m64).abs().max()), float((v - v64).abs().max())
        worst = max(worst, em / scale, ev / scale)
        assert em < TOL_STATS * scale and ev < TOL_STATS * scale, \
            (ctx, 'first layer out of bounds: ' + p, 'mean err %.3g var err %.3g bound %.3g' % (em, ev, TOL_STATS * scale))
    reach = float(l64.abs().max())
    tol_logits = TOL_LOGITS * max(1.0, reach / 9.0)          # TOL_LOGITS was set for |logit| <= 9
    el = float((got['logits'].double() - l64).abs().max())
    ed = float((got['desc'].double() - d64).abs().max())
    e = _ERRORS.setdefault(tag, {'logits': 0.0, 'logits_over_bar': 0.0, 'desc': 0.0, 'stats_rel': 0.0})
    e['logits'], e['desc'], e['stats_rel'] = max(e['logits'], el), max(e['desc'], ed), max(e['stats_rel'], worst)
    e['logits_over_bar'] = max(e['logits_over_bar'], el / tol_logits)
    print('\n[batch stats %s] %s: max |logit| %.3g (bar x %.3g), logits err %.3g, desc err %.3g, statistics err / scale %.3g'
          % (tag, ctx, reach, max(1.0, reach / 9.0), el, ed, worst))
    assert el < tol_logits, (ctx, 'logits', el, tol_logits)
    assert ed < TOL_DESC, (ctx, 'desc', ed)


def _where(a, b):
    bad = (a != b).nonzero()
    return '%d of %d differ; first (index, got, want): %s' % (
        bad.shape[0], a.numel(), [(tuple(int(i) for i in p), float(a[tuple(p)]), float(b[tuple(p)])) for p in bad[:4]])


def _check_identical(a, b, ctx):
    for p in a['stats']:
        for i, what in enumerate(('mean', 'var')):
            assert torch.equal(a['stats'][p][i], b['stats'][p][i]), (ctx, p, what, _where(a['stats'][p][i], b['stats'][p][i]))
    assert torch.equal(a['logits'], b['logits']), (ctx, 'logits', _where(a['logits'], b['logits']))
    assert torch.equal(a['desc'], b['desc']), (ctx, 'desc', _where(a['desc'], b['desc']))


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    for tag, e in _ERRORS.items():
        print('\n[batch stats routes] %-40s max logits err %.3g (%.2f of its bar), desc err %.3g, statistics err / scale %.3g'
              % (tag or 'default (per tile)', e['logits'], e['logits_over_bar'], e['desc'], e['stats_rel']))


def _routes_case(monkeypatch, name, shape, routings):
    cfg, sd, img, opt, ref = _case(name, shape)
    route = ROUTES[shape[0]] if cfg.get('multispectral') else None
    runs = []
    for env in routings:
        got = _run(monkeypatch, cfg, sd, img, opt, env)
        # the handle took the machine shape and every 3x3 launch is on the side of the gate this routing is meant to test
        ncu = _check_gate(name, cfg, shape, route, env, got['ncu'])
        assert ncu == got['ncu'] and ncu == _debug(env).get('ncu', ncu), (env, ncu, got['ncu'])
        _check_restatement(got, ref, (name, shape, env), env)
        runs.append((env, got))
    for env, got in runs[1:]:
        _check_identical(got, runs[0][1], (name, shape, env, 'against', runs[0][0] or 'default'))
    return runs


@pytest.mark.parametrize('name,shape', CASES, ids=['%s-%dx%dx%d' % ((n,) + s) for n, s in CASES])
def test_routes(monkeypatch, name, shape):
    """Per-tile launches (default handle) and persistent launches on two emulated machine shapes (four where a launch has fewer than 6 items):
    logits, descriptors and every layer's batch mean and unbiased variance within the bars of the float64 restatement, and
    bit-identical between all routings -- the machine shape only changes the grid, and the persistent kernels multiply and add in
    the per-tile kernels' order."""
    _routes_case(monkeypatch, name, shape, _routings(name))


def test_more_than_65535_rows(monkeypatch):
    """33 frames 2048 x 8 (zero padding: the deepest frame is 256 x 1): 67584 rows, more than bn_apply_kernel's 65535 grid rows, so
    its row loop makes a second trip; 540672 full-resolution pixels, more than MP_BN_MAX_PARTS * 256, so the statistics partials
    are capped and a partial's chunk is no multiple of the kernel's rows per pass.  On a whole MI355X the default handle already
    launches enc.conv2 persistently here (2112 items), so the per-tile routing is no_persist and the default runs besides."""
    assert MANY_ROWS[0] * MANY_ROWS[1] > 65535
    runs = _routes_case(monkeypatch, 'many_rows', MANY_ROWS, ['no_persist'] + MACHINE)
    # the default handle: whatever side of the gate its launches fall on, the same bits
    cfg, sd, img, opt, ref = _case('many_rows', MANY_ROWS)
    got = _run(monkeypatch, cfg, sd, img, opt, '')
    _check_restatement(got, ref, ('many_rows', MANY_ROWS, 'default'), 'default, 67584 rows')
    _check_identical(got, runs[0][1], ('many_rows', 'default against no_persist'))


def _abi_call(net, img, want_desc, want_stats):
    """mp_forward_batch_stats with optional outputs left NULL; the outputs it was given are pre-filled with NaN."""
    h = net._handle
    B, _, H, W = img.shape
    n = sum(ch for _, ch in net.batch_statistics_layout())
    logits = torch.full((B, 65, H // 8, W // 8), float('nan'), device=DEV)
    desc = torch.full((B, H // 8, W // 8, net.config['descriptor_size']), float('nan'), device=DEV) if want_desc else None
    stats = torch.full((2 * n,), float('nan'), device=DEV) if want_stats else None
    x = img.to(DEV).contiguous()
    rc = h.lib.mp_forward_batch_stats(h.ptr, ctypes.c_void_p(x.data_ptr()), None, B, H, W, ctypes.c_void_p(logits.data_ptr()),
                                      ctypes.c_void_p(desc.data_ptr()) if want_desc else None,
                                      ctypes.c_void_p(stats.data_ptr()) if want_stats else None, None)
    assert rc == 0, h.lib.mp_last_error(h.ptr).decode()
    torch.cuda.synchronize()
    return logits.cpu(), None if desc is None else desc.cpu(), None if stats is None else stats.cpu()


@pytest.mark.parametrize('name', ['shipped', 'd256'])
def test_optional_outputs_of_the_c_abi(name):
    """desc == NULL on a model with a descriptor head (the raw descriptors go to the workspace behind the logits, and their layers'
    statistics are still reported) and stats == NULL: what the call does return is bit-identical to the full call's."""
    shape = (3, 72, 104)
    cfg, sd, img, _, ref = _case(name, shape)
    net = _net(cfg, sd)
    logits, desc, stats = _abi_call(net, img, True, True)
    assert not torch.isnan(logits).any() and not torch.isnan(desc).any() and not torch.isnan(stats).any()
    # the full call is the one the restatement bars hold for
    layout = net.batch_statistics_layout()
    off, st = 0, {}
    for p, ch in layout:
        st[p] = (stats[off:off + ch], stats[off + ch:off + 2 * ch])
        off += 2 * ch
    _check_restatement({'logits': logits, 'desc': desc.permute(0, 3, 1, 2), 'stats': st}, ref, (name, shape, 'C ABI'), 'C ABI, all outputs')
    assert any(p.startswith('descriptor_head') for p, _ in layout)
    l2, d2, s2 = _abi_call(net, img, False, True)
    assert d2 is None
    assert torch.equal(l2, logits), ('desc NULL: logits', _where(l2, logits))
    assert torch.equal(s2, stats), ('desc NULL: statistics (descriptor layers included)', _where(s2, stats))
    l3, d3, s3 = _abi_call(net, img, True, False)
    assert s3 is None
    assert torch.equal(l3, logits), ('stats NULL: logits', _where(l3, logits))
    assert torch.equal(d3, desc), ('stats NULL: desc', _where(d3, desc))
    l4, _, _ = _abi_call(net, img, False, False)
    assert torch.equal(l4, logits), ('desc and stats NULL: logits', _where(l4, logits))


@pytest.mark.parametrize('name', ['shipped', 'channel_v1', 'channel_v2_bn_first'])
def test_stale_workspace_cannot_reach_an_output(monkeypatch, name):
    """A forward on NaN images leaves NaN in the workspace tensors of the handle (nothing faults); a clean input of the same shape
    on that handle must then give the bits of a fresh handle, without a NaN.  The detector's logits tensor has 80 channels per
    pixel of which the 1x1 convolution writes 65, and channel versions 1 / 2 carry padding channels: what is read there must never
    reach an output.  The maxima of the forward (ReLU, fmax in bn_finalize_kernel) return their other operand for a NaN, so NaN
    stops at the first of them; a second fill with large finite images reaches the tensors behind it."""
    shape = (3, 72, 104)
    cfg, sd, img, opt, ref = _case(name, shape)
    fresh = _run(monkeypatch, cfg, sd, img, opt, '')
    _check_restatement(fresh, ref, (name, shape, 'fresh handle'), 'default')
    net = _net(cfg, sd)
    net.set_batch_statistics(True)
    fills = {'NaN': torch.full_like(img, float('nan')), 'large': 2e3 * R.O.make_images(99, *shape) - 1e3}
    for fill, dirty in fills.items():
        with torch.no_grad():
            net(_data(dirty, opt))
            out = net(_data(img, opt))
        got = {'logits': out['logits'].cpu(), 'desc': out['desc'].cpu(),
               'stats': {p: (m.cpu(), v.cpu()) for p, (m, v) in net.last_batch_statistics().items()}}
        for p, (m, v) in got['stats'].items():
            assert bool(torch.isfinite(m).all()) and bool(torch.isfinite(v).all()), (name, fill, p)
        assert bool(torch.isfinite(got['logits']).all()) and bool(torch.isfinite(got['desc']).all()), (name, fill)
        _check_identical(got, fresh, (name, shape, 'after a forward on %s images, against a fresh handle' % fill))
