"""GPU: the loss kernels (csrc/losses.hip through SuperPointLoss, descriptor_loss_sums and the C ABI) at every cell count
where a tile begins or ends, against the float64 restatements.  tests/loss_shape_cases.py builds the inputs and the answers
(once per process); tests/test_loss_shapes_host.py asserts their premises on the CPU -- above all that every sum the
descriptor kernels form on these inputs is exact in fp32, so that the comparisons here are np.array_equal against float64.

What each test reaches that tests/test_gpu_loss.py and tests/test_gpu_loss_grad.py do not:

  test_descriptor_forward[HcxWc-D]   N = 1, 31 .. 33, 63 .. 65, 95, 97, 127 .. 129, 255 .. 257, 385, 513 at D = 64, 128, 256:
                                     desc_loss_tile_kernel's clamped rows (min(i0 + row, N - 1)) with one live row, a full
                                     last tile, one row in the last tile; 1 to 5 x 5 tiles; desc_prologue_kernel with one live
                                     thread, 255 .. 257 cells, a third workgroup of one cell; Wc = 1 and Hc = 1 in its n / Wc
                                     decode; the positive, negative and pair sums bit for bit (a dropped, doubled or wrongly
                                     weighted pair changes them), warped centres bit for bit, hinge ties, the five mask
                                     layouts, an image without valid cells, a row alone against the row in its batch
  test_descriptor_backward[HcxWc-D]  desc_loss_grad_kernel's own-cell workgroups (one live lane, 127 .. 129 cells, a fifth
                                     workgroup of one cell), its other-side walk in tiles of 64 rows (32 at D = 256) with 1,
                                     TI - 1, TI and TI + 1 rows, the `i0 + TI < N` prefetch guard and the `jj < N` store guard:
                                     both gradients for every cell and channel bit for bit, NaN for the empty image only
  test_random_homographies           the general warp path at N = 33, 129, 513 for each D, sums AND gradients bit for bit on the
                                     kernel's own centres
  test_thresholds                    corr_bound at 0, -1, inf, 8, float32(sqrt(128)) and the float below it, on pairs at
                                     squared distance 0, 64 and 128
  test_stale_memory_backward         mp_descriptor_loss_backward into NaN-filled gradients with a 0xFF workspace
  test_detector[...]                 detector_loss_kernel / detector_loss_backward_kernel on the same grids, CE with host and
                                     with device noise and BCE; the pixel-position sweep; the BCE clamps
"""
import ctypes

import numpy as np
import pytest
import torch

import loss_restatement as R
import loss_shape_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _gpu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _bits(x):
    """a float array as integers: equal bits, NaN included"""
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def _sides(case, images=None, grad=(False, False)):
    """(pred, data) of the two sides, for all images or for the listed ones"""
    sel = slice(None) if images is None else list(images)
    pred, data = [], []
    for s in (1, 2):
        desc = _gpu(case['inputs']['desc%d' % s][sel])
        pred.append({'logits': None, 'desc': desc.requires_grad_() if grad[s - 1] else desc})
        d = {'valid_mask': _gpu(case['inputs']['valid_mask%d' % s][sel])}
        if 'homography%d' % s in case['inputs']:
            d['homography'] = _gpu(case['inputs']['homography%d' % s][sel])
        data.append(d)
    return pred, data


def forward(case, images=None, config=None, workspace=None):
    """(sums (B, 4) float64, warped (2, B, N, 2) fp32) of descriptor_loss_sums, host arrays"""
    from multipoint_amd.utils.losses import descriptor_loss_sums
    pred, data = _sides(case, images)
    B = pred[0]['desc'].shape[0]
    warped = torch.full((2, B, case['N'], 2), float('nan'), dtype=torch.float32, device=DEV)
    out = descriptor_loss_sums(pred[0]['desc'], pred[1]['desc'], data[0].get('homography'), data[1].get('homography'),
                               data[0]['valid_mask'], data[1]['valid_mask'], dict(R.DEFAULTS, **dict(case['config'], **(config or {}))),
                               workspace=workspace, warped=warped)
    return out.cpu().numpy(), warped.cpu().numpy()


def backward(case, grad=(True, True)):
    """(values (4,), g1, g2) of SuperPointLoss.evaluate and values.backward(C.upstream): float64 host arrays, None for a
    side that does not require grad"""
    from multipoint_amd.utils.losses import SuperPointLoss
    pred, data = _sides(case, grad=grad)
    values, keys = SuperPointLoss(case['config']).evaluate(pred[0], data[0], pred[1], data[1])
    assert keys == C.KEYS and values.dtype == torch.float64
    values.backward(gradient=_gpu(C.upstream(case)))
    g = [None if p['desc'].grad is None else p['desc'].grad.cpu().numpy() for p in pred]
    for p, x in zip(pred, g):
        assert x is None or (x.dtype == np.float32 and x.shape == tuple(p['desc'].shape))
    return values.detach().cpu().numpy(), g[0], g[1]


def _workspace(case, fill):
    from multipoint_amd import _lib
    Hc, Wc = case['grid']
    n = ctypes.c_longlong()
    assert _lib.get_handle(DEV).lib.mp_loss_workspace_bytes(case['B'], 8 * Hc, 8 * Wc, ctypes.byref(n)) == 0
    return torch.full((n.value,), fill, dtype=torch.uint8, device=DEV)


def _assert_forward(got, warped, ref, name):
    for k, col in enumerate(('positive', 'negative', 'pairs', 'norm')):
        assert np.array_equal(got[:, k], ref['sums'][:, k]), (name, col, got[:, k].tolist(), ref['sums'][:, k].tolist())
    assert np.array_equal(warped, ref['warped']), name


def _assert_gradients(g1, g2, ref, name):
    for k, g in (('g1', g1), ('g2', g2)):
        bad = ~((g.astype(np.float64) == ref[k]) | (np.isnan(g) & np.isnan(ref[k])))
        assert not bad.any(), (name, k, int(bad.sum()), np.argwhere(bad)[:4].tolist(),
                               g[bad][:4].tolist(), ref[k][bad][:4].tolist())


@pytest.mark.parametrize('name', C.descriptor_names())
def test_descriptor_forward(name):
    """All four columns of the sums and the warped centres equal float64's; a second run, a run with a workspace of 0xFF bytes
    and each image run alone give the same bits."""
    case, ref = C.descriptor_case(name), C.descriptor_reference(name)
    got, warped = forward(case)
    _assert_forward(got, warped, ref, name)
    again, warped2 = forward(case)
    assert np.array_equal(_bits(got), _bits(again)) and np.array_equal(_bits(warped), _bits(warped2))
    stale, warped3 = forward(case, workspace=_workspace(case, 0xFF))
    assert np.array_equal(_bits(got), _bits(stale)) and np.array_equal(_bits(warped), _bits(warped3))
    for b in range(case['B']):
        alone, w = forward(case, images=[b])
        assert np.array_equal(_bits(alone[0]), _bits(got[b])), (name, b)
        assert np.array_equal(_bits(w[:, 0]), _bits(warped[:, b])), (name, b)


@pytest.mark.parametrize('name', C.descriptor_names())
def test_descriptor_backward(name):
    """Both gradients equal float64's for every cell and channel (NaN where the reference's is: the image without valid
    cells); a second run gives the same bits, and so does each side when the other does not require grad."""
    case, ref = C.descriptor_case(name), C.descriptor_reference(name)
    values, g1, g2 = backward(case)
    _assert_gradients(g1, g2, ref, name)
    s = ref['sums']
    with np.errstate(invalid='ignore'):
        want = [((s[:, 0] + s[:, 1]) / s[:, 3]).mean(), (s[:, 0] / s[:, 3]).mean(), (s[:, 1] / s[:, 3]).mean()]
    assert np.allclose(values[1:], want, rtol=1e-14, atol=0, equal_nan=True), (values, want)
    assert np.allclose(values[0], R.DEFAULTS['lambda'] * want[0], rtol=1e-14, atol=0, equal_nan=True)
    v2, h1, h2 = backward(case)
    assert np.array_equal(_bits(values), _bits(v2))
    assert np.array_equal(_bits(g1), _bits(h1)) and np.array_equal(_bits(g2), _bits(h2))
    _, a1, a2 = backward(case, grad=(True, False))
    assert a2 is None and np.array_equal(_bits(a1), _bits(g1))
    _, b1, b2 = backward(case, grad=(False, True))
    assert b1 is None and np.array_equal(_bits(b2), _bits(g2))


@pytest.mark.parametrize('name', C.random_names())
def test_random_homographies(name):
    """The general warp path at these N: the kernel's fp32 centres lie within 1e-4 px of float64's, and on those centres
    the sums and both gradients equal float64's bit for bit."""
    case = C.random_case(name)
    got, warped = forward(case)
    Hc, Wc = case['grid']
    for s in (1, 2):
        centres = R.warp_centres(case['inputs']['homography%d' % s], case['B'], Hc, Wc)
        assert np.abs(warped[s - 1] - centres).max() < 1e-4
    ref = dict(C.descriptor_answers(case, warped[0], warped[1]), warped=warped)
    assert ref['sums'][:, 2].min() > 0 and ref['sums'][:, :2].min() > 0
    _assert_forward(got, warped, ref, name)
    _, g1, g2 = backward(case)
    _assert_gradients(g1, g2, ref, name)


@pytest.mark.parametrize('i', range(len(C.THRESHOLD_CASES)))
def test_thresholds(i):
    """descriptor_loss_threshold 0, -1, inf, 8, float32(sqrt(128)) and the float below: the pair count and the sums are those
    of `sqrt_rn(s) <= threshold` on fp32 distances."""
    case = C.threshold_case(i)
    for t, thr in enumerate(C.THRESHOLDS):
        got, _ = forward(case, config={'descriptor_loss_threshold': thr})
        ref = C.threshold_reference(i, t)
        print('N = %d threshold %r: pairs %s' % (case['N'], thr, got[:, 2].tolist()))
        assert np.array_equal(got, ref), (thr, got.tolist(), ref.tolist())


@pytest.mark.parametrize('i', range(len(C.STALE_CASES)))
def test_stale_memory_backward(i):
    """One direct mp_descriptor_loss_backward per tile class into gradient buffers filled with NaN, with a workspace of 0xFF
    bytes: the wrapper's bits, float64's values, and no NaN -- an unwritten cell or a stale partial would be one."""
    from multipoint_amd import _lib
    from multipoint_amd.utils.losses import descriptor_loss_sums
    case, ref = C.stale_case(i), C.stale_reference(i)
    B, D, N, (Hc, Wc) = case['B'], case['D'], case['N'], case['grid']
    _, w1, w2 = backward(case)
    _assert_gradients(w1, w2, ref, i)
    pred, data = _sides(case)
    cfg = dict(R.DEFAULTS, **case['config'])
    fwd = descriptor_loss_sums(pred[0]['desc'], pred[1]['desc'], data[0].get('homography'), data[1].get('homography'),
                               data[0]['valid_mask'], data[1]['valid_mask'], cfg, workspace=_workspace(case, 0xFF))
    assert np.array_equal(fwd.cpu().numpy(), ref['sums'])
    d = [p['desc'].permute(0, 2, 3, 1).contiguous() for p in pred]              # [B][Hc][Wc][D]
    hom = [x.get('homography') for x in data]
    hom = [None if m is None else m.contiguous() for m in hom]
    valid = [x['valid_mask'].reshape(B, 8 * Hc, 8 * Wc).view(torch.uint8).contiguous() for x in data]
    coef = _gpu(np.array([case['alpha'], case['beta']]))
    g = [torch.full((B, Hc, Wc, D), float('nan'), dtype=torch.float32, device=DEV) for _ in (1, 2)]
    ws = _workspace(case, 0xFF)
    h = _lib.get_handle(DEV)
    P = _lib.ptr
    rc = h.lib.mp_descriptor_loss_backward(
        h.ptr, P(d[0]), P(d[1]), B, Hc, Wc, D, P(hom[0]), P(hom[1]), P(valid[0]), P(valid[1]), 8 * Hc, 8 * Wc,
        float(cfg['descriptor_loss_threshold']), float(cfg['positive_margin']), float(cfg['negative_margin']),
        float(cfg['lambda_d']), 1, P(fwd), P(coef), P(ws), ws.numel(), P(g[0]), P(g[1]), _lib.stream_ptr(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    for got, want in zip(g, (w1, w2)):
        got = got.permute(0, 3, 1, 2).cpu().numpy()
        assert not np.isnan(got).any()
        assert np.array_equal(_bits(got), _bits(want))


# ---- detector ----
def _error(got, ref):
    """largest difference over the finite entries; the NaN entries must be the reference's"""
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    ok = np.isfinite(ref)
    return float(np.abs(got[ok] - ref[ok]).max()) if ok.any() else 0.0


@pytest.mark.parametrize('name', C.detector_names())
def test_detector(name):
    """mp_detector_loss's valid-cell counts exactly, its sums and the per-cell dlogits of loss.backward() within
    C.detector_tolerance: max(4 x the float32 restatement's own error, 8 fp32 ulps) of the largest reference value."""
    from multipoint_amd import _lib
    from multipoint_amd.utils.losses import SuperPointLoss
    case, ref = C.detector_case(name), C.detector_reference(name)
    B, (Hc, Wc), inp = case['B'], case['grid'], case['inputs']
    h = _lib.get_handle(DEV)
    P, S = _lib.ptr, _lib.stream_ptr(torch.device(DEV))
    ws = _workspace(case, 0xFF)
    pred, data = [], []
    for s in (1, 2):
        lg = _gpu(inp['logits%d' % s])
        kp = _gpu(inp['keypoints%d' % s]).view(torch.uint8)
        vm = _gpu(inp['valid_mask%d' % s])
        noise = _gpu(case['noise'][s - 1]) if case['mode'] == 'ce_host' else None
        out = torch.full((B, 2), float('nan'), dtype=torch.float64, device=DEV)
        rc = h.lib.mp_detector_loss(h.ptr, P(lg), B, Hc, Wc, P(kp), P(vm.reshape(B, 8 * Hc, 8 * Wc).view(torch.uint8)), 8 * Hc,
                                    8 * Wc, int(case['use_ce']), P(noise), 2 * C.DEVICE_SEED + s - 1, P(ws), ws.numel(), P(out), S)
        assert rc == 0
        out = out.cpu().numpy()
        tol = C.detector_tolerance('sum', ref['sum%d' % s])
        err = _error(out[:, 0], ref['sum%d' % s])
        print('%s side %d: counts %s, sum error %.3g, tolerance %.3g' % (name, s, out[:, 1].tolist(), err, tol))
        assert np.array_equal(out[:, 1], ref['count%d' % s])
        assert err <= tol, (name, s, err, tol)
        pred.append({'logits': lg.requires_grad_(), 'desc': None})
        data.append({'keypoints': _gpu(inp['keypoints%d' % s]), 'valid_mask': vm})
    cfg = {'descriptor_loss': False, 'detector_use_cross_entropy': case['use_ce'],
           'label_noise': 'device' if case['mode'] == 'ce_device' else 'host', 'label_noise_seed': C.DEVICE_SEED}
    torch.manual_seed(case['seed'])
    loss, comp = SuperPointLoss(cfg)(pred[0], data[0], pred[1], data[1])
    loss.backward()
    for s in (1, 2):
        with np.errstate(invalid='ignore'):
            want = float(np.mean(ref['sum%d' % s] / ref['count%d' % s]))
        tol = C.detector_tolerance('sum', ref['sum%d' % s]) / max(ref['count%d' % s].min(), 1.0)
        assert np.isnan(want) == np.isnan(comp['detector_loss%d' % s])
        assert np.isnan(want) or abs(comp['detector_loss%d' % s] - want) <= tol
        got = pred[s - 1]['logits'].grad.double().cpu().numpy()
        tol = C.detector_tolerance('grad', ref['grad%d' % s])
        err = _error(got, ref['grad%d' % s])
        print('%s side %d: dlogits error %.3g, tolerance %.3g' % (name, s, err, tol))
        assert err <= tol, (name, s, err, tol)
