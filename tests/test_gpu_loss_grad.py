"""GPU checks of SuperPointLoss's HIP backward (csrc/losses.hip: detector_loss_backward_kernel, desc_loss_grad_kernel)
against the float64 gradient restatement (tests/loss_grad_restatement.py), whose agreement with the reference's
autograd is measured on the CPU (tests/test_loss_grad_golden.py: reference_error)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_grad_restatement as RG
import loss_restatement as R
from test_loss_grad_golden import GRAD_CASES, KEYS, NAMES, load_grad_case, reference_error

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS32 = float(np.finfo(np.float32).eps)


def leaves(inputs, dev=DEV, dtype=torch.float32):
    """{name: leaf tensor requiring grad} for logits1 / logits2 / desc1 / desc2."""
    return {k: torch.from_numpy(inputs[k]).to(dev, dtype).requires_grad_() for k in NAMES}


def batch(inputs, lv, dev=DEV):
    pred, data = [], []
    for side in (1, 2):
        pred.append({'logits': lv['logits%d' % side], 'desc': lv['desc%d' % side]})
        d = {'keypoints': torch.from_numpy(inputs['keypoints%d' % side]).to(dev),
             'valid_mask': torch.from_numpy(inputs['valid_mask%d' % side]).to(dev)}
        if 'homography%d' % side in inputs:
            d['homography'] = torch.from_numpy(inputs['homography%d' % side]).to(dev)
        data.append(d)
    return pred, data


def kernel_warped(inputs, cfg):
    """The kernel's fp32 warped centres (the correspondence decisions the backward takes too)."""
    from multipoint_amd.utils.losses import descriptor_loss_sums
    lv = {k: torch.from_numpy(inputs[k]).to(DEV) for k in NAMES}
    pred, data = batch(inputs, lv)
    B, D, Hc, Wc = lv['desc1'].shape
    warped = torch.empty((2, B, Hc * Wc, 2), dtype=torch.float32, device=DEV)
    descriptor_loss_sums(lv['desc1'], lv['desc2'], data[0].get('homography'), data[1].get('homography'),
                         data[0]['valid_mask'], data[1]['valid_mask'], dict(R.DEFAULTS, **cfg), warped=warped)
    w = warped.cpu().numpy()
    return w[0], w[1]


def tolerance(err, ref):
    """4 x the reference's recorded fp32 error, at least 8 fp32 ulps of the largest gradient."""
    return max(4.0 * err, 8.0 * EPS32 * float(np.abs(ref).max()))


def assert_grads(got, want, errs, images=None):
    for k in NAMES:
        if want[k] is None:
            continue
        g = got[k].detach().double().cpu().numpy()
        w = want[k]
        if images is not None:
            g, w = g[images], w[images]
        tol = tolerance(errs[k], w)
        e = np.abs(g - w).max()
        assert e <= tol, (k, e, tol)


@pytest.fixture(scope='module')
def errors():
    return {c[0]: reference_error(c) for c in GRAD_CASES}


@pytest.mark.parametrize('train_keys', [False, True], ids=['case_config', 'train_config'])
@pytest.mark.parametrize('case', GRAD_CASES, ids=[c[0] for c in GRAD_CASES])
def test_backward_matches_restatement(case, train_keys, errors):
    """loss.backward() fills .grad of all four inputs with the gradients of the total loss."""
    from multipoint_amd.utils.losses import SuperPointLoss
    inputs, stored, _, noise = load_grad_case(case)
    cfg = R.case_config(case)
    if train_keys:
        cfg = dict(cfg, **{'lambda': 1.0, 'descriptor_loss_threshold': 4.0, 'lambda_d': 250})
    lv = leaves(inputs)
    pred, data = batch(inputs, lv)
    torch.manual_seed(int(stored['seed']))
    loss, _ = SuperPointLoss(cfg)(pred[0], data[0], pred[1], data[1])
    loss.backward()
    want = RG.grads(inputs, cfg, KEYS, {'total': 1.0}, noise[0], noise[1], warped=kernel_warped(inputs, cfg))
    for k in NAMES:
        assert lv[k].grad is not None and lv[k].grad.shape == lv[k].shape, k
    assert_grads({k: lv[k].grad for k in NAMES}, want, errors[case[0]])


# frames with N > 128 cells, N a multiple of none of 128 (own cells per workgroup), 64 and 32 (other-side tile rows): several
# own workgroups per image with a partial last one, a partial last tile, and each of D = 64, 128, 256
GRID_CASES = [
    # name,              seed, B,  H,   W,   D,  ce,    mask,  hom,      thr, multi
    ('d64_120x160',       21, 2, 120, 160,  64, True,  True,  'random', 8.0, False),
    ('d128_120x160',      22, 2, 120, 160, 128, False, True,  'random', 8.0, False),
    ('d256_120x160',      23, 2, 120, 160, 256, True,  False, 'random', 4.0, False),
    ('d256_bce_120x160',  24, 2, 120, 160, 256, False, True,  'random', 8.0, False),
] + [c for c in R.CASES if c[0] == 'ce_240x320']


@pytest.mark.parametrize('case', GRID_CASES, ids=[c[0] for c in GRID_CASES])
def test_backward_on_production_grids(case):
    """All four gradients against the restatement on the kernel's warped centres.  The inputs are on the golden cases'
    exact grids (every dot exact in fp32 for D <= 256), so the decisions agree and an ulp tolerance holds; a wrong
    own-cell offset of a later workgroup, an unwritten cell or a wrong D = 256 tile fails it."""
    from multipoint_amd.utils.losses import SuperPointLoss
    from test_loss_golden import host_noise
    inputs = R.dequantize(R.make_case_inputs(case))
    cfg = R.case_config(case)
    seed, B, H, W = case[1], case[2], case[3], case[4]
    N = (H // 8) * (W // 8)
    assert N > 128 and N % 128 and N % 64 and N % 32
    lv = leaves(inputs)
    pred, data = batch(inputs, lv)
    torch.manual_seed(seed)
    loss, _ = SuperPointLoss(cfg)(pred[0], data[0], pred[1], data[1])
    loss.backward()
    noise = host_noise(seed, B, H // 8, W // 8) if cfg['detector_use_cross_entropy'] else (None, None)
    want = RG.grads(inputs, cfg, KEYS, {'total': 1.0}, noise[0], noise[1], warped=kernel_warped(inputs, cfg))
    for k in NAMES:
        g = lv[k].grad.double().cpu().numpy()
        assert np.isfinite(g).all(), k
        tol = 64.0 * EPS32 * float(np.abs(want[k]).max())
        assert np.abs(g - want[k]).max() <= tol, (k, float(np.abs(g - want[k]).max()), tol)


def test_unneeded_descriptor_side_is_skipped():
    """A side that does not require grad gets none, and the other side's gradient is the same bits as with both."""
    from multipoint_amd.utils.losses import SuperPointLoss
    case = GRAD_CASES[0]
    inputs, stored, _, _ = load_grad_case(case)
    runs = []
    for frozen in (None, 'desc2', 'desc1'):
        lv = leaves(inputs)
        if frozen:
            lv[frozen] = lv[frozen].detach()
        pred, data = batch(inputs, lv)
        torch.manual_seed(int(stored['seed']))
        loss, _ = SuperPointLoss(R.case_config(case))(pred[0], data[0], pred[1], data[1])
        loss.backward()
        runs.append(lv)
    assert runs[1]['desc2'].grad is None and runs[2]['desc1'].grad is None
    assert torch.equal(runs[1]['desc1'].grad, runs[0]['desc1'].grad)
    assert torch.equal(runs[2]['desc2'].grad, runs[0]['desc2'].grad)


def test_inplace_edit_of_saved_descriptors_is_caught():
    """The fp32 channels-last descriptors the backward reads are saved tensors: editing them in place between forward
    and backward raises instead of silently changing the gradients."""
    from multipoint_amd.utils.losses import SuperPointLoss
    case = GRAD_CASES[0]
    inputs, stored, _, _ = load_grad_case(case)
    lv = leaves(inputs)
    cl = {k: lv[k].detach().permute(0, 2, 3, 1).contiguous().requires_grad_() for k in ('desc1', 'desc2')}
    pred, data = batch(inputs, dict(lv, desc1=cl['desc1'].permute(0, 3, 1, 2), desc2=cl['desc2'].permute(0, 3, 1, 2)))
    torch.manual_seed(int(stored['seed']))
    loss, _ = SuperPointLoss(R.case_config(case))(pred[0], data[0], pred[1], data[1])
    with torch.no_grad():
        cl['desc1'].mul_(2.0)
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        loss.backward()


@pytest.mark.parametrize('case', [GRAD_CASES[0], GRAD_CASES[1]], ids=lambda c: c[0])
def test_component_gradients(case, errors):
    """torch.autograd.grad of each entry of values: the upstream coefficients alpha / beta / gamma."""
    from multipoint_amd.utils.losses import SuperPointLoss
    inputs, stored, _, noise = load_grad_case(case)
    cfg = dict(R.case_config(case), **{'lambda': 0.5})
    warped = kernel_warped(inputs, cfg)
    for idx, key in enumerate(('total',) + KEYS):
        lv = leaves(inputs)
        pred, data = batch(inputs, lv)
        torch.manual_seed(int(stored['seed']))
        values, keys = SuperPointLoss(cfg).evaluate(pred[0], data[0], pred[1], data[1])
        assert keys == KEYS
        got = torch.autograd.grad(values[idx], [lv[k] for k in NAMES], allow_unused=True)
        want = RG.grads(inputs, cfg, KEYS, {key: 1.0}, noise[0], noise[1], warped=warped)
        for k, g in zip(NAMES, got):
            w = want[k]
            if np.abs(w).max() == 0:
                assert g is None or not g.abs().max().item(), (key, k)
                continue
            tol = tolerance(errors[case[0]][k], w)
            assert np.abs(g.double().cpu().numpy() - w).max() <= tol, (key, k)


def _tie_inputs(B=2, Hc=8, Wc=12, D=64, seed=5):
    """Descriptors of 0.5 on 4 of the first 8 channels: every dot is 0.25 x overlap, so many equal the margins."""
    rng = np.random.RandomState(seed)
    inputs = {}
    for side in (1, 2):
        d = np.zeros((B, D, Hc, Wc), np.float32)
        for b in range(B):
            for h in range(Hc):
                for w in range(Wc):
                    d[b, rng.choice(8, 4, replace=False), h, w] = 0.5
        inputs['desc%d' % side] = d
        inputs['logits%d' % side] = np.zeros((B, 65, Hc, Wc), np.float32)
        inputs['keypoints%d' % side] = np.zeros((B, 8 * Hc, 8 * Wc), bool)
        inputs['valid_mask%d' % side] = np.ones((B, 1, 8 * Hc, 8 * Wc), bool)
    return inputs


def test_hinge_ties_carry_half_weight(monkeypatch):
    from multipoint_amd.utils.losses import SuperPointLoss
    inputs = _tie_inputs()
    cfg = {'detector_loss': False, 'positive_margin': 0.5, 'negative_margin': 0.25, 'descriptor_loss_threshold': 8.0}
    lv = leaves(inputs)
    pred, data = batch(inputs, lv)
    loss, _ = SuperPointLoss(cfg)(pred[0], data[0], pred[1], data[1])
    loss.backward()
    B, D, Hc, Wc = inputs['desc1'].shape
    d1, d2 = inputs['desc1'].reshape(B, D, -1), inputs['desc2'].reshape(B, D, -1)
    dot = np.einsum('bdi,bdj->bij', d2, d1)
    assert (dot == 0.5).sum() > 100 and (dot == 0.25).sum() > 100
    warped = kernel_warped(inputs, cfg)
    got = {k: lv[k].grad for k in NAMES}
    want = RG.grads(inputs, cfg, KEYS[2:], {'total': 1.0}, warped=warped)
    tol = {k: 64.0 * EPS32 * float(np.abs(want[k]).max()) for k in ('desc1', 'desc2')}
    for k in ('desc1', 'desc2'):
        assert np.abs(got[k].double().cpu().numpy() - want[k]).max() <= tol[k], k
    for tie in (0.0, 1.0):
        monkeypatch.setattr(RG, 'hinge', lambda x, t=tie: np.where(x > 0, 1.0, np.where(x == 0, t, 0.0)))
        alt = RG.grads(inputs, cfg, KEYS[2:], {'total': 1.0}, warped=warped)
        for k in ('desc1', 'desc2'):
            assert np.abs(got[k].double().cpu().numpy() - alt[k]).max() > 100 * tol[k], (tie, k)
    monkeypatch.undo()


def test_device_noise_gradients():
    """'device' labels: bit-identical to 'host' where cells hold <= 1 keypoint; in multi-keypoint cells the labels
    follow the splitmix64 hash, which the restatement reproduces."""
    from multipoint_amd.utils.losses import SuperPointLoss
    case = [c for c in GRAD_CASES if c[10]][0]
    inputs, stored, _, _ = load_grad_case(case)
    cfg = dict(R.case_config(case), descriptor_loss=False)
    B, H, W = inputs['keypoints1'].shape
    Hc, Wc = H // 8, W // 8

    def run(inp, mode, seed=3):
        lv = leaves(inp)
        pred, data = batch(inp, lv)
        torch.manual_seed(0)
        loss, _ = SuperPointLoss(dict(cfg, label_noise=mode, label_noise_seed=seed))(pred[0], data[0], pred[1], data[1])
        loss.backward()
        return [lv['logits%d' % s].grad for s in (1, 2)]

    dev = run(inputs, 'device')
    labels = [R.detector_labels(inputs['keypoints%d' % s], RG.device_noise(3 * 2 + s - 1, B, Hc, Wc)) for s in (1, 2)]
    want = RG.grads(inputs, cfg, KEYS[:2], {'total': 1.0}, labels=labels)
    for s in (1, 2):
        w = want['logits%d' % s]
        assert np.abs(dev[s - 1].double().cpu().numpy() - w).max() <= 8 * EPS32 * np.abs(w).max()
    single = dict(inputs)
    for s in (1, 2):
        cells = R.space_to_depth(inputs['keypoints%d' % s])
        keep = np.cumsum(cells, 1) <= 1
        single['keypoints%d' % s] = (cells & keep).reshape(B, 8, 8, Hc, Wc).transpose(0, 3, 1, 4, 2).reshape(B, H, W)
    a, b = run(single, 'device'), run(single, 'host')
    for s in (0, 1):
        assert torch.equal(a[s], b[s])


def test_backward_is_deterministic():
    from multipoint_amd.utils.losses import SuperPointLoss
    case = GRAD_CASES[4]                                          # D = 128
    inputs, stored, _, _ = load_grad_case(case)
    runs = []
    for _ in range(2):
        lv = leaves(inputs)
        pred, data = batch(inputs, lv)
        torch.manual_seed(int(stored['seed']))
        loss, _ = SuperPointLoss(R.case_config(case))(pred[0], data[0], pred[1], data[1])
        loss.backward()
        runs.append([lv[k].grad.clone() for k in NAMES])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_values_without_and_with_grad():
    from multipoint_amd.utils.losses import SuperPointLoss
    case = GRAD_CASES[0]
    inputs, stored, _, _ = load_grad_case(case)
    loss_fn = SuperPointLoss(R.case_config(case))

    def values(requires_grad, no_grad=False):
        lv = leaves(inputs)
        if not requires_grad:
            lv = {k: v.detach() for k, v in lv.items()}
        pred, data = batch(inputs, lv)
        torch.manual_seed(int(stored['seed']))
        if no_grad:
            with torch.no_grad():
                return loss_fn.evaluate(pred[0], data[0], pred[1], data[1])[0]
        return loss_fn.evaluate(pred[0], data[0], pred[1], data[1])[0]

    plain = values(False)
    assert plain.grad_fn is None and not plain.requires_grad
    under = values(True, no_grad=True)
    assert under.grad_fn is None
    graded = values(True)
    assert graded.grad_fn is not None and graded.dtype == torch.float64
    assert torch.equal(plain, under) and torch.equal(plain, graded.detach())


@pytest.mark.parametrize('variant', ['fp16', 'noncontiguous', 'cpu'])
def test_input_dtype_device_layout(variant):
    """Gradients come back in each input's dtype, device and shape; they are the fp32 device gradients converted."""
    from multipoint_amd.utils.losses import SuperPointLoss
    case = GRAD_CASES[0]
    inputs, stored, _, _ = load_grad_case(case)
    cfg = R.case_config(case)

    def run(lv, dev):
        pred, data = batch(inputs, lv, dev)
        torch.manual_seed(int(stored['seed']))
        loss, _ = SuperPointLoss(cfg)(pred[0], data[0], pred[1], data[1])
        loss.backward()

    if variant == 'fp16':
        base = leaves({k: inputs[k].astype(np.float16).astype(np.float32) for k in NAMES})
        lv = leaves(inputs, dtype=torch.float16)
        dev = DEV
    elif variant == 'cpu':
        base = leaves(inputs)
        lv = leaves(inputs, dev='cpu')
        dev = 'cpu'
    else:
        base = leaves(inputs)
        big = {k: torch.from_numpy(np.concatenate([inputs[k], inputs[k]], 1)).to(DEV).requires_grad_() for k in NAMES}
        lv = {k: big[k][:, :inputs[k].shape[1]] for k in NAMES}                  # channel slices: not contiguous
        assert not any(v.is_contiguous() for v in lv.values())
        dev = DEV
    run(base, DEV)
    run(lv, dev)
    for k in NAMES:
        leaf = big[k] if variant == 'noncontiguous' else lv[k]
        g = leaf.grad
        assert g is not None and g.dtype == leaf.dtype and g.device == leaf.device and g.shape == leaf.shape, k
        if variant == 'noncontiguous':
            n = inputs[k].shape[1]
            assert torch.equal(g[:, :n], base[k].grad) and not g[:, n:].any(), k
        else:
            assert torch.equal(g.to(DEV), base[k].grad.to(g.dtype)), k


def test_empty_valid_mask_gives_nan_for_that_image_only(errors):
    from multipoint_amd.utils.losses import SuperPointLoss
    case = GRAD_CASES[0]
    inputs, stored, _, noise = load_grad_case(case)
    inputs = dict(inputs)
    vm = inputs['valid_mask1'].copy()
    vm[0] = False
    inputs['valid_mask1'] = vm
    cfg = R.case_config(case)
    lv = leaves(inputs)
    pred, data = batch(inputs, lv)
    torch.manual_seed(int(stored['seed']))
    loss, _ = SuperPointLoss(cfg)(pred[0], data[0], pred[1], data[1])
    loss.backward()
    for k in ('logits1', 'desc1', 'desc2'):
        assert torch.isnan(lv[k].grad[0]).all(), k
    for k in NAMES:
        assert torch.isfinite(lv[k].grad[1:]).all(), k
    assert torch.isfinite(lv['logits2'].grad).all()
    want = RG.grads(inputs, cfg, KEYS, {'total': 1.0}, noise[0], noise[1], warped=kernel_warped(inputs, cfg))
    assert_grads({k: lv[k].grad for k in NAMES}, want, errors[case[0]], images=slice(1, None))


def test_memory_is_linear_in_cells():
    """B = 32 at 480x640, D = 64: forward + backward grow torch's peak by less than 64 MB beyond the gradients
    themselves and the kept host noise."""
    from multipoint_amd.utils.losses import SuperPointLoss
    B, H, W, D = 32, 480, 640, 64
    Hc, Wc = H // 8, W // 8
    g = torch.Generator(device=DEV).manual_seed(0)
    leaves_, pred, data = [], [], []
    for s in range(2):
        desc = torch.randn((B, Hc, Wc, D), device=DEV, generator=g)
        desc = (desc / desc.norm(dim=-1, keepdim=True)).requires_grad_()
        logits = torch.randn((B, 65, Hc, Wc), device=DEV, generator=g).requires_grad_()
        leaves_ += [desc, logits]
        pred.append({'logits': logits, 'desc': desc.permute(0, 3, 1, 2)})
        data.append({'keypoints': torch.rand((B, H, W), device=DEV, generator=g) < 0.005,
                     'valid_mask': torch.ones((B, 1, H, W), dtype=torch.bool, device=DEV)})
    for mode in ('host', 'device'):
        for t in leaves_:
            t.grad = None
        loss_fn = SuperPointLoss({'label_noise': mode})
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(DEV)
        torch.cuda.reset_peak_memory_stats(DEV)
        loss, _ = loss_fn(pred[0], data[0], pred[1], data[1])
        loss.backward()
        torch.cuda.synchronize()
        kept = sum(t.grad.numel() * 4 for t in leaves_)
        if mode == 'host':
            kept += 2 * B * 64 * Hc * Wc * 4
        grow = torch.cuda.max_memory_allocated(DEV) - base - kept
        assert grow < 64 * 2 ** 20, (mode, grow)
        assert all(torch.isfinite(t.grad).all() for t in leaves_)


class _Net(torch.nn.Module):
    """A small differentiable detector / descriptor network: 1 x H x W -> logits 65 x H/8 x W/8, desc 64 x H/8 x W/8."""

    def __init__(self):
        super().__init__()
        self.c1 = torch.nn.Conv2d(1, 16, 3, stride=2, padding=1)
        self.c2 = torch.nn.Conv2d(16, 32, 3, stride=2, padding=1)
        self.c3 = torch.nn.Conv2d(32, 64, 3, stride=2, padding=1)
        self.det = torch.nn.Conv2d(64, 65, 1)
        self.desc = torch.nn.Conv2d(64, 64, 1)

    def forward(self, x):
        x = F.relu(self.c3(F.relu(self.c2(F.relu(self.c1(x))))))
        return {'logits': self.det(x), 'desc': F.normalize(self.desc(x), dim=1)}


def _dense_loss64(pred1, data1, pred2, data2, noise1, noise2, cfg):
    """The dense SuperPointLoss in float64 torch, from its definition (N^2 tensors; identity warps: no homography)."""
    def det(pred, data, noise):
        lg = pred['logits'].double()
        B, _, Hc, Wc = lg.shape
        kp = data['keypoints'].reshape(B, Hc, 8, Wc, 8).permute(0, 2, 4, 1, 3).reshape(B, 64, Hc, Wc).float()
        lab = torch.cat([3.0 * kp + noise, torch.full((B, 1, Hc, Wc), 2.0, device=lg.device)], 1).argmax(1)
        vm = data['valid_mask'].reshape(B, Hc, 8, Wc, 8).permute(0, 2, 4, 1, 3).reshape(B, 64, Hc, Wc).all(1).double()
        ce = F.cross_entropy(lg, lab, reduction='none') * vm
        return (ce.sum((1, 2)) / vm.sum((1, 2))).mean()

    total = det(pred1, data1, noise1) + (det(pred2, data2, noise2) if pred2 is not None else 0.0)
    if pred2 is None:
        return total
    d1, d2 = pred1['desc'].double(), pred2['desc'].double()
    B, D, Hc, Wc = d1.shape
    hh, ww = torch.meshgrid(torch.arange(Hc), torch.arange(Wc), indexing='ij')
    c = torch.stack([hh * 8.0 + 4, ww * 8.0 + 4], -1).reshape(-1, 2).double().to(d1.device)
    corr = ((c[None, :, :] - c[:, None, :]).norm(dim=-1) <= cfg['descriptor_loss_threshold']).double()
    dot = torch.einsum('bdi,bdj->bij', d2.reshape(B, D, -1), d1.reshape(B, D, -1))
    zero = torch.zeros(1, dtype=torch.float64, device=d1.device)
    pos = cfg['lambda_d'] * corr * torch.max(zero, cfg['positive_margin'] - dot)
    neg = (1 - corr) * torch.max(zero, dot - cfg['negative_margin'])
    v1 = data1['valid_mask'].reshape(B, Hc, 8, Wc, 8).permute(0, 2, 4, 1, 3).reshape(B, 64, -1).all(1).double()
    v2 = data2['valid_mask'].reshape(B, Hc, 8, Wc, 8).permute(0, 2, 4, 1, 3).reshape(B, 64, -1).all(1).double()
    m = v2[:, :, None] * v1[:, None, :]
    norm = m.sum((1, 2))
    desc = (((pos + neg) * m).sum((1, 2)) / norm).mean()
    return total + cfg['lambda'] * desc


@pytest.mark.parametrize('pair', [True, False], ids=['pair', 'single_detector_only'])
def test_training_step_matches_float64_torch(pair):
    """One Adam step with the HIP loss and one with the float64 dense formulation: the same parameter gradients and
    the same updated parameters."""
    from multipoint_amd.utils.losses import SuperPointLoss
    B, H, W = 2, 64, 96
    cfg = {'lambda': 1.0, 'descriptor_loss_threshold': 4.0, 'lambda_d': 250, 'descriptor_loss': pair}
    full = dict(R.DEFAULTS, **cfg)
    rng = np.random.RandomState(7)
    img = [torch.from_numpy(rng.uniform(size=(B, 1, H, W)).astype(np.float32)).to(DEV) for _ in range(2)]
    data = []
    for s in range(2):
        vm = np.zeros((B, 1, H, W), bool)
        vm[:, :, 4:H - 8, 8:W - 4] = True
        data.append({'keypoints': torch.from_numpy(rng.uniform(size=(B, H, W)) < 0.02).to(DEV),
                     'valid_mask': torch.from_numpy(vm).to(DEV)})
    nets, grads = [], []
    for use_hip in (True, False):
        torch.manual_seed(0)
        net = _Net().to(DEV)
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        opt.zero_grad()
        p1 = net(img[0])
        p2 = net(img[1]) if pair else None
        torch.manual_seed(11)
        if use_hip:
            if pair:
                loss, _ = SuperPointLoss(cfg)(p1, data[0], p2, data[1])
            else:
                loss, _ = SuperPointLoss(cfg)(p1, data[0])
        else:
            n1 = torch.rand((B, 64, H // 8, W // 8)).to(DEV)
            n2 = torch.rand((B, 64, H // 8, W // 8)).to(DEV) if pair else None
            loss = _dense_loss64(p1, data[0], p2, data[1] if pair else None, n1, n2, full)
        loss.sum().backward()
        grads.append([None if p.grad is None else p.grad.clone() for p in net.parameters()])
        opt.step()
        nets.append([p.detach().clone() for p in net.parameters()])
    for a, b in zip(grads[0], grads[1]):
        assert (a is None) == (b is None)
        if b is None:                                             # the descriptor head without the descriptor loss
            continue
        scale = b.abs().max().item()
        assert scale > 0 and (a - b).abs().max().item() <= 1e-4 * scale
    for a, b, g in zip(nets[0], nets[1], grads[1]):
        if g is None:
            assert torch.equal(a, b)
            continue
        big = g.abs() > 1e-3 * g.abs().max()
        assert (a - b).abs().max().item() <= 2e-3
        assert (a - b)[big].abs().max().item() <= 1e-5


def test_c_abi_rejects_bad_arguments():
    from multipoint_amd import _lib
    h = _lib.get_handle(DEV)
    n = ctypes.c_longlong()
    assert h.lib.mp_loss_workspace_bytes(2, 64, 64, ctypes.byref(n)) == 0
    ws = torch.empty(n.value, dtype=torch.uint8, device=DEV)
    fo = torch.ones((2, 4), dtype=torch.float64, device=DEV)
    coef = torch.ones(2, dtype=torch.float64, device=DEV)
    d = torch.zeros((2, 8, 8, 64), device=DEV)
    g1, g2 = torch.empty_like(d), torch.empty_like(d)
    kp = torch.zeros((2, 64, 64), dtype=torch.uint8, device=DEV)
    lg = torch.zeros((2, 65, 8, 8), device=DEV)
    gl = torch.empty_like(lg)
    P, S = _lib.ptr, _lib.stream_ptr(torch.device(DEV))

    def desc(D=64, Hc=8, H=64, nbytes=n.value, a=d, go=g1, go2=g2, f=fo):
        return h.lib.mp_descriptor_loss_backward(h.ptr, P(a), P(d), 2, Hc, 8, D, None, None, None, None, H, 64, 8.0, 1.0,
                                                 0.2, 250.0, 1, P(f), P(coef), P(ws), nbytes, P(go), P(go2), S)

    def det(Hc=8, H=64, nbytes=n.value, a=lg, go=gl):
        return h.lib.mp_detector_loss_backward(h.ptr, P(a), 2, Hc, 8, P(kp), None, H, 64, 1, None, 0, P(fo), P(coef),
                                               P(ws), nbytes, P(go), S)
    assert desc() == 0 and det() == 0
    assert desc(a=None) == -1 and desc(f=None) == -1                 # NULL tensors
    assert desc(go=None, go2=None) == -1                             # no gradient asked for
    assert desc(go=None) == 0 and desc(go2=None) == 0                # one side skipped
    assert det(a=None) == -1 and det(go=None) == -1
    assert desc(D=32) == -1 and desc(D=96) == -1                     # D outside {64, 128, 256}
    assert desc(H=72) == -1 and det(H=72) == -1                      # H != 8 Hc
    assert desc(Hc=7) == -1 and det(Hc=7) == -1
    assert desc(nbytes=16) == -1 and det(nbytes=16) == -1            # workspace too small
    torch.cuda.synchronize()
