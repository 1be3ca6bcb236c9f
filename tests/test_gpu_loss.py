"""GPU checks of SuperPointLoss (multipoint_amd/utils/losses.py, csrc/losses.hip) against the reference's losses
(tests/golden/superpoint_loss.npz) and the float64 restatement (tests/loss_restatement.py)."""
import ctypes

import numpy as np
import pytest
import torch

import loss_restatement as R
from test_loss_golden import analytic_identity_count, load_case

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def to_gpu(inputs):
    pred, data = [], []
    for side in (1, 2):
        pred.append({'logits': torch.from_numpy(inputs['logits%d' % side]).to(DEV),
                     'desc': torch.from_numpy(inputs['desc%d' % side]).to(DEV)})
        d = {'keypoints': torch.from_numpy(inputs['keypoints%d' % side]).to(DEV),
             'valid_mask': torch.from_numpy(inputs['valid_mask%d' % side]).to(DEV)}
        if 'homography%d' % side in inputs:
            d['homography'] = torch.from_numpy(inputs['homography%d' % side]).to(DEV)
        data.append(d)
    return pred, data


def kernel_sums(inputs, cfg):
    """mp_descriptor_loss's per-image sums and its warped centres (host arrays)."""
    from multipoint_amd.utils.losses import descriptor_loss_sums
    pred, data = to_gpu(inputs)
    B, D, Hc, Wc = pred[0]['desc'].shape
    warped = torch.empty((2, B, Hc * Wc, 2), dtype=torch.float32, device=DEV)
    out = descriptor_loss_sums(pred[0]['desc'], pred[1]['desc'], data[0].get('homography'), data[1].get('homography'),
                               data[0]['valid_mask'], data[1]['valid_mask'], dict(R.DEFAULTS, **cfg), warped=warped)
    return out.cpu().numpy(), warped.cpu().numpy()


@pytest.mark.parametrize('case', R.CASES, ids=[c[0] for c in R.CASES])
def test_golden_host_noise(case):
    """label_noise 'host' under the reference's seed: every component equals the reference's within 1e-5 (the
    multi-keypoint case fails if the noise is drawn differently or in another order)."""
    from multipoint_amd.utils.losses import SuperPointLoss
    inputs, stored = load_case(case)
    pred, data = to_gpu(inputs)
    torch.manual_seed(int(stored['seed']))
    loss, comp = SuperPointLoss(R.case_config(case))(pred[0], data[0], pred[1], data[1])
    assert loss.shape == (1,) and loss.device.type == 'cuda'
    for i, k in enumerate(R.COMPONENTS):
        assert comp[k] == pytest.approx(stored['components'][i], rel=1e-5), k
    assert float(loss) == pytest.approx(float(stored['loss']), rel=1e-5)


@pytest.mark.parametrize('case', [c for c in R.CASES if c[8] == 'identity'], ids=lambda c: c[0])
def test_identity_count_is_exact(case):
    """Identity homographies at threshold 8.0: every 4-neighbour lies at exactly 8.0 -- an approximate sqrt, a < for <=,
    or an off-by-one cell centre changes the count."""
    inputs, stored = load_case(case)
    cfg = R.case_config(case)
    out, warped = kernel_sums(inputs, cfg)
    B, H, W = inputs['keypoints1'].shape
    if cfg['descriptor_loss_use_mask']:
        v1, v2 = R.cell_valid(inputs['valid_mask1'], B, H, W), R.cell_valid(inputs['valid_mask2'], B, H, W)
    else:
        v1 = v2 = np.ones((B, H // 8, W // 8), bool)
    assert np.array_equal(out[:, 2], analytic_identity_count(v1, v2).astype(np.float64))
    assert np.array_equal(out[:, 2], stored['corr_count'].astype(np.float64))
    assert np.array_equal(warped[0], R.warp_centres(None, B, H // 8, W // 8).astype(np.float32))


@pytest.mark.parametrize('case', [c for c in R.CASES if c[8] == 'random'], ids=lambda c: c[0])
def test_random_homography_decisions(case):
    """The kernel's warped centres are within 1e-4 px of the float64 restatement's, and its counts and sums equal the
    restatement's computed from those same fp32 centres."""
    inputs, stored = load_case(case)
    cfg = R.case_config(case)
    out, warped = kernel_sums(inputs, cfg)
    B, H, W = inputs['keypoints1'].shape
    for side in (1, 2):
        ref = R.warp_centres(inputs['homography%d' % side], B, H // 8, W // 8)
        assert np.abs(warped[side - 1] - ref).max() < 1e-4
    v1, v2 = R.cell_valid(inputs['valid_mask1'], B, H, W), R.cell_valid(inputs['valid_mask2'], B, H, W)
    sums = R.descriptor_loss_sums(inputs['desc1'], inputs['desc2'], warped[0], warped[1], v1, v2, cfg)[0]
    assert np.array_equal(out[:, 2], sums[:, 2])
    assert np.array_equal(out[:, 3], sums[:, 3])
    np.testing.assert_allclose(out[:, :2], sums[:, :2], rtol=1e-6)
    assert np.all(np.abs(out[:, 2] - stored['corr_count']) <= stored['near_count'])


def _model(D, seed=0):
    from oracle import mp_oracle as O
    import multipoint_amd.models as models
    cfg = dict(O.SHIPPED_MODEL_CONFIG)
    cfg['descriptor_size'] = D
    net = models.MultiPoint(cfg)
    net.load_state_dict(O.make_weights(seed, cfg))
    net.to(DEV).eval()
    net.set_force_return_logits(True)
    return net


def _augmented_pairs(seed, B, H, W):
    """Image pairs whose second image is the first warped by a random homography (GPU augmentation), with keypoint
    labels and the augmentation's valid masks."""
    from oracle import mp_oracle as O
    from multipoint_amd.datasets.augmentation import homographic_augmentation_batch
    rng = np.random.RandomState(seed)
    img = O.make_images(seed, B, H, W).to(DEV)
    homs = np.stack([R.random_homography(rng, H, W) for _ in range(B)])
    warped, mask = homographic_augmentation_batch(img, homs.astype(np.float64))
    kp1 = torch.from_numpy(rng.uniform(size=(B, H, W)) < 0.005)
    kp2 = torch.from_numpy(rng.uniform(size=(B, H, W)) < 0.005)
    d1 = {'image': img, 'keypoints': kp1.to(DEV), 'valid_mask': torch.ones((B, 1, H, W), dtype=torch.bool, device=DEV),
          'homography': torch.from_numpy(np.broadcast_to(np.eye(3, dtype=np.float32), (B, 3, 3)).copy()).to(DEV)}
    d2 = {'image': warped, 'keypoints': kp2.to(DEV), 'valid_mask': mask, 'homography': torch.from_numpy(homs).to(DEV)}
    return d1, d2


def _restated(pred1, d1, pred2, d2, cfg, seed):
    """The restatement on the same GPU outputs, with the kernel's fp32 warped centres (so that both take the same
    correspondence decisions)."""
    from multipoint_amd.utils.losses import descriptor_loss_sums
    B, _, Hc, Wc = pred1['logits'].shape
    warped = torch.empty((2, B, Hc * Wc, 2), dtype=torch.float32, device=DEV)
    descriptor_loss_sums(pred1['desc'], pred2['desc'], d1['homography'], d2['homography'], d1['valid_mask'],
                         d2['valid_mask'], cfg, warped=warped)
    warped = warped.cpu().numpy()
    torch.manual_seed(seed)
    n1, n2 = torch.rand((B, 64, Hc, Wc)).numpy(), torch.rand((B, 64, Hc, Wc)).numpy()
    inputs = {}
    for s, (p, d) in enumerate(((pred1, d1), (pred2, d2)), 1):
        inputs['logits%d' % s] = p['logits'].cpu().numpy()
        inputs['desc%d' % s] = p['desc'].cpu().numpy()
        inputs['keypoints%d' % s] = d['keypoints'].cpu().numpy()
        inputs['valid_mask%d' % s] = d['valid_mask'].cpu().numpy()
        inputs['homography%d' % s] = d['homography'].cpu().numpy()
    return R.loss(inputs, cfg, n1, n2, warped=(warped[0], warped[1]))


@pytest.mark.parametrize('B,H,W', [(8, 240, 320), (2, 480, 640)])
def test_end_to_end_model_outputs(B, H, W):
    """MultiPoint (force_return_logits) -> SuperPointLoss on augmented pairs equals the restatement applied to the same
    GPU outputs; two calls are bit-identical."""
    from multipoint_amd.utils.losses import SuperPointLoss
    net = _model(64)
    d1, d2 = _augmented_pairs(5, B, H, W)
    with torch.no_grad():
        p1, p2 = net(d1), net(d2)
    assert p1['desc'].permute(0, 2, 3, 1).is_contiguous()          # the channels-last storage is used as it is
    loss_fn = SuperPointLoss()
    torch.manual_seed(3)
    v1, keys = loss_fn.evaluate(p1, d1, p2, d2)
    torch.manual_seed(3)
    v2, _ = loss_fn.evaluate(p1, d1, p2, d2)
    assert torch.equal(v1, v2)
    total, comp, _ = _restated(p1, d1, p2, d2, loss_fn.config, 3)
    got = v1.cpu().numpy()
    assert got[0] == pytest.approx(total, rel=1e-5)
    for i, k in enumerate(keys):
        assert got[i + 1] == pytest.approx(comp[k], rel=1e-5), k


@pytest.mark.parametrize('D', [64, 128, 256])
def test_descriptor_sizes(D):
    """D = 64, 128, 256 on random unit descriptors with random homographies, mask on."""
    from multipoint_amd.utils.losses import SuperPointLoss
    rng = np.random.RandomState(D)
    B, H, W = 2, 120, 160
    inputs = {}
    for s in (1, 2):
        d = rng.standard_normal((B, D, H // 8, W // 8)).astype(np.float32)
        inputs['desc%d' % s] = d / np.linalg.norm(d, axis=1, keepdims=True)
        inputs['logits%d' % s] = rng.standard_normal((B, 65, H // 8, W // 8)).astype(np.float32)
        inputs['keypoints%d' % s] = rng.uniform(size=(B, H, W)) < 0.01
        v = np.zeros((B, 1, H, W), bool)
        v[:, :, 8:-5, 3:-9] = True
        inputs['valid_mask%d' % s] = v
        inputs['homography%d' % s] = np.stack([R.random_homography(rng, H, W) for _ in range(B)])
    pred, data = to_gpu(inputs)
    cfg = {'descriptor_loss_threshold': 8.0}
    torch.manual_seed(9)
    _, comp = SuperPointLoss(cfg)(pred[0], data[0], pred[1], data[1])
    torch.manual_seed(9)
    n1, n2 = torch.rand((B, 64, H // 8, W // 8)).numpy(), torch.rand((B, 64, H // 8, W // 8)).numpy()
    out, warped = kernel_sums(inputs, cfg)
    _, ref, _ = R.loss(inputs, cfg, n1, n2, warped=(warped[0], warped[1]))
    for k in R.COMPONENTS:
        assert comp[k] == pytest.approx(ref[k], rel=1e-5), k


def test_device_noise():
    """label_noise 'device': deterministic for a seed, changed by the seed, equal to 'host' where every cell holds <= 1
    keypoint, and the torch CPU generator is left alone."""
    from multipoint_amd.utils.losses import SuperPointLoss
    case = [c for c in R.CASES if c[10]][0]                          # cells with 2-4 keypoints
    inputs, _ = load_case(case)
    pred, data = to_gpu(inputs)
    cfg = dict(R.case_config(case), descriptor_loss=False)
    state = torch.get_rng_state()
    a = SuperPointLoss(dict(cfg, label_noise='device', label_noise_seed=1)).evaluate(pred[0], data[0], pred[1], data[1])[0]
    b = SuperPointLoss(dict(cfg, label_noise='device', label_noise_seed=1)).evaluate(pred[0], data[0], pred[1], data[1])[0]
    c = SuperPointLoss(dict(cfg, label_noise='device', label_noise_seed=2)).evaluate(pred[0], data[0], pred[1], data[1])[0]
    assert torch.equal(torch.get_rng_state(), state)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    # at most one keypoint per cell: the labels, hence the sums, are those of the host draw
    single = {}
    for s in (1, 2):
        kp = inputs['keypoints%d' % s].copy()
        cells = R.space_to_depth(kp)
        keep = np.cumsum(cells, 1) <= 1
        B, H, W = kp.shape
        single[s] = (cells & keep).reshape(B, 8, 8, H // 8, W // 8).transpose(0, 3, 1, 4, 2).reshape(B, H, W)
        assert R.space_to_depth(single[s]).sum(1).max() == 1
        data[s - 1]['keypoints'] = torch.from_numpy(single[s]).to(DEV)
    d = SuperPointLoss(dict(cfg, label_noise='device', label_noise_seed=7)).evaluate(pred[0], data[0], pred[1], data[1])[0]
    torch.manual_seed(0)
    h = SuperPointLoss(dict(cfg, label_noise='host')).evaluate(pred[0], data[0], pred[1], data[1])[0]
    assert torch.equal(d, h)


def test_memory_is_linear_in_cells():
    """B = 32 at 480x640: torch's peak allocated memory grows by less than 64 MB during the loss (the reference's
    formulation holds several 32 x 4800^2 fp32 tensors, > 10 GB)."""
    from multipoint_amd.utils.losses import SuperPointLoss
    B, H, W, D = 32, 480, 640, 64
    Hc, Wc = H // 8, W // 8
    g = torch.Generator(device=DEV).manual_seed(0)
    pred, data = [], []
    for s in range(2):
        desc = torch.randn((B, Hc, Wc, D), device=DEV, generator=g)
        desc = desc / desc.norm(dim=-1, keepdim=True)
        pred.append({'logits': torch.randn((B, 65, Hc, Wc), device=DEV, generator=g), 'desc': desc.permute(0, 3, 1, 2)})
        data.append({'keypoints': torch.rand((B, H, W), device=DEV, generator=g) < 0.005,
                     'valid_mask': torch.ones((B, 1, H, W), dtype=torch.bool, device=DEV)})
    for mode in ('host', 'device'):
        loss_fn = SuperPointLoss({'label_noise': mode})
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(DEV)
        torch.cuda.reset_peak_memory_stats(DEV)
        v, _ = loss_fn.evaluate(pred[0], data[0], pred[1], data[1])
        torch.cuda.synchronize()
        grow = torch.cuda.max_memory_allocated(DEV) - base
        assert grow < 64 * 2 ** 20, (mode, grow)
        assert torch.isfinite(v).all()


def test_c_abi_rejects_bad_shapes():
    from multipoint_amd import _lib
    h = _lib.get_handle(DEV)
    n = ctypes.c_longlong()
    assert h.lib.mp_loss_workspace_bytes(2, 60, 64, ctypes.byref(n)) == -1
    assert h.lib.mp_loss_workspace_bytes(2, 64, 64, ctypes.byref(n)) == 0 and n.value > 0
    ws = torch.empty(n.value, dtype=torch.uint8, device=DEV)
    out = torch.empty((2, 4), dtype=torch.float64, device=DEV)
    d = torch.zeros((2, 8, 8, 64), device=DEV)
    kp = torch.zeros((2, 64, 64), dtype=torch.uint8, device=DEV)
    lg = torch.zeros((2, 65, 8, 8), device=DEV)
    P, S = _lib.ptr, _lib.stream_ptr(torch.device(DEV))

    def desc(D, Hc, Wc, H, W, nbytes=n.value):
        return h.lib.mp_descriptor_loss(h.ptr, P(d), P(d), 2, Hc, Wc, D, None, None, None, None, H, W, 8.0, 1.0, 0.2, 250.0,
                                        1, P(ws), nbytes, P(out), None, S)
    assert desc(64, 8, 8, 64, 64) == 0
    assert desc(32, 8, 8, 64, 64) == -1                             # D outside {64, 128, 256}
    assert desc(96, 8, 8, 64, 64) == -1
    assert desc(64, 8, 8, 64, 60) == -1                             # W not a multiple of 8
    assert desc(64, 8, 7, 64, 64) == -1                             # cell grid and label maps disagree
    assert desc(64, 8, 8, 64, 64, nbytes=16) == -1                  # workspace too small
    assert h.lib.mp_detector_loss(h.ptr, P(lg), 2, 8, 8, P(kp), None, 64, 64, 1, None, 0, P(ws), n.value, P(out), S) == 0
    assert h.lib.mp_detector_loss(h.ptr, P(lg), 2, 8, 9, P(kp), None, 64, 64, 1, None, 0, P(ws), n.value, P(out), S) == -1
    torch.cuda.synchronize()
