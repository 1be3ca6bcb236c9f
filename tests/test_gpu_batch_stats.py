"""Batch-statistics (training-mode) forward on the GPU: MultiPoint.set_batch_statistics(True) / mp_forward_batch_stats against
the reference fixture tests/golden/batch_statistics.npz and the float64 restatement (tests/batch_stats_restatement.py)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import batch_stats_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# Tolerances against the float64 restatement.  The reference's own fp32 forward (the fixture) is within 8.9e-5 (logits, |logit|
# <= 9) and 8.3e-6 (unit-norm descriptors) of float64 over these cases (tests/test_batch_stats_golden.py); the HIP path rounds
# as often but sums the convolutions in another order (MFMA k-blocks) and forms the affine as x * scale + shift (one fma) instead
# of (x - mean) * invstd * gamma + beta, so its error is of the same order.  We hold it to 4x the reference's worst case.
TOL_LOGITS = 4e-4
TOL_DESC = 4e-5
# the statistics themselves: mean / unbiased variance accumulated in fp64 from fp32 activations, relative to the layer's scale
TOL_STATS = 2e-5


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'batch_statistics.npz'))


def _net(cfg, sd):
    from multipoint_amd.models import MultiPoint
    net = MultiPoint(cfg)
    net.load_state_dict(sd)
    net.to(DEV)
    return net


def _data(img, opt):
    d = {'image': img.to(DEV)}
    if opt is not None:
        d['is_optical'] = opt.to(DEV)
    return d


def _case(golden, idx):
    case = R.CASES[idx]
    seed = int(golden['seed']) + idx
    sd = R.case_weights(case, seed)
    img, opt = R.case_inputs(case, seed)
    return case, R.case_config(case), sd, img, opt


@pytest.mark.parametrize('idx', range(len(R.CASES)), ids=[c[0] for c in R.CASES])
def test_golden_cases(golden, idx):
    case, cfg, sd, img, opt = _case(golden, idx)
    name = case[0]
    net = _net(cfg, sd)
    net.set_batch_statistics(True)
    with torch.no_grad():
        out = net(_data(img, opt))
    assert out['prob'] is None and net.training is False
    assert out['logits'].shape == (img.shape[0], 65, img.shape[2] // 8, img.shape[3] // 8)
    lg, ds = out['logits'].cpu().numpy(), out['desc'].cpu().numpy()
    l64, d64, st64 = R.forward_train64(sd, img, cfg, opt)
    assert np.abs(lg - l64.numpy()).max() < TOL_LOGITS
    assert np.abs(ds - d64.numpy()).max() < TOL_DESC
    assert np.abs(lg - golden[name + '/logits']).max() < TOL_LOGITS
    assert np.abs(ds - golden[name + '/desc']).max() < TOL_DESC
    # 0.9 running_old + 0.1 (our batch mean, unbiased var) == the reference's running statistics after its forward
    stats = net.last_batch_statistics()
    assert list(stats) == list(st64)                  # state_dict order; an encoder without images has no entry
    for p in R.bn_prefixes(cfg):
        ref = golden['%s/running/%s' % (name, p)]
        if p not in stats:
            assert np.array_equal(ref, np.stack([sd[p + '.running_mean'].numpy(), sd[p + '.running_var'].numpy()]))
            continue
        m, v = (t.cpu().double() for t in stats[p])
        m64, v64 = st64[p]
        scale = 1 + max(float(m64.abs().max()), float(v64.abs().max()))
        assert float((m - m64).abs().max()) < TOL_STATS * scale and float((v - v64).abs().max()) < TOL_STATS * scale, p
        blend = np.stack([(0.9 * sd[p + '.running_mean'].double() + 0.1 * m).numpy(),
                          (0.9 * sd[p + '.running_var'].double() + 0.1 * v).numpy()])
        assert np.abs(blend - ref).max() < 4e-6 * (1 + np.abs(ref).max()), p
    # the model's own running statistics are not modified
    for k, t in net.state_dict().items():
        assert torch.equal(t, sd[k]), k


def test_running_statistics_differ_from_the_batch(golden):
    """The fixture's running statistics are not the batch's: the eval-mode forward gives other logits."""
    _, cfg, sd, img, opt = _case(golden, 0)
    net = _net(cfg, sd)
    net.set_force_return_logits(True)
    with torch.no_grad():
        ev = net(_data(img, opt))['logits'].cpu().numpy()
    assert np.abs(ev - golden['shipped/logits']).max() > 0.5


def test_bit_identical_runs_and_eval_untouched(golden):
    _, cfg, sd, img, opt = _case(golden, R.CASES.index(next(c for c in R.CASES if c[0] == 'ms_mixed')))
    net = _net(cfg, sd)
    data = _data(img, opt)
    with torch.no_grad():
        e1 = net(data)
        net.set_batch_statistics(True)
        a = net(data)
        sa = {k: (m.clone(), v.clone()) for k, (m, v) in net.last_batch_statistics().items()}
        b = net(data)
        sb = net.last_batch_statistics()
        net.set_batch_statistics(False)
        e2 = net(data)
    assert torch.equal(a['logits'], b['logits']) and torch.equal(a['desc'], b['desc'])
    for k in sa:
        assert torch.equal(sa[k][0], sb[k][0]) and torch.equal(sa[k][1], sb[k][1])
    assert torch.equal(e1['prob'], e2['prob']) and torch.equal(e1['desc'], e2['desc'])


def test_refusals(golden):
    from oracle import mp_oracle as O
    from multipoint_amd.models import MultiPoint, SuperPointMagicLeap
    img = O.make_images(0, 2, 16, 16).to(DEV)
    mp = MultiPoint(dict(O.SHIPPED_MODEL_CONFIG, mixed_precision=True))
    mp.load_state_dict(O.make_weights(0, dict(O.SHIPPED_MODEL_CONFIG)))
    mp.to(DEV)
    mp.set_batch_statistics(True)
    with pytest.raises(NotImplementedError, match='mixed_precision'):
        mp({'image': img})
    ml = SuperPointMagicLeap()
    ml.load_state_dict(O.make_weights_magicleap(0))
    ml.to(DEV)
    ml.set_batch_statistics(True)
    with pytest.raises(NotImplementedError, match='no BatchNorm'):
        ml({'image': img})
    net = _net(dict(O.SHIPPED_MODEL_CONFIG), O.make_weights(0, dict(O.SHIPPED_MODEL_CONFIG)))
    net.set_batch_statistics(True)
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        net({'image': img[:1, :, :8, :8].contiguous()})
    # the C ABI refuses the same cases with MP_EINVAL and a message
    for model in (mp, ml, net):
        h = model._handle
        logits = torch.empty((1, 65, 1, 1), device=DEV)
        rc = h.lib.mp_forward_batch_stats(h.ptr, ctypes.c_void_p(img.data_ptr()), None, 1, 8, 8,
                                          ctypes.c_void_p(logits.data_ptr()), None, None, None)
        assert rc == -1
        msg = h.lib.mp_last_error(h.ptr).decode()
        assert ('mixed_precision' in msg) if model is mp else ('no BatchNorm' in msg) if model is ml else \
            ('more than 1 value per channel' in msg), msg


def test_training_shape_b32_240x320():
    """train.py's config shape (batch 32 at 240x320) on the shipped model against the float64 restatement."""
    from oracle import mp_oracle as O
    cfg = dict(O.SHIPPED_MODEL_CONFIG)
    sd = R.case_weights(('b32', {}), 11)
    img = O.make_images(12, 32, 240, 320)
    net = _net(cfg, sd)
    net.set_batch_statistics(True)
    with torch.no_grad():
        out = net({'image': img.to(DEV)})
    torch.set_num_threads(min(16, torch.get_num_threads()))
    l64, d64, st64 = R.forward_train64(sd, img, cfg)
    assert np.abs(out['logits'].cpu().numpy() - l64.numpy()).max() < TOL_LOGITS
    assert np.abs(out['desc'].cpu().numpy() - d64.numpy()).max() < TOL_DESC
    for p, (m, v) in net.last_batch_statistics().items():
        m64, v64 = st64[p]
        scale = 1 + max(float(m64.abs().max()), float(v64.abs().max()))
        assert float((m.cpu().double() - m64).abs().max()) < TOL_STATS * scale, p
        assert float((v.cpu().double() - v64).abs().max()) < TOL_STATS * scale, p


def test_cli_batch_statistics_equals_direct_loop(tmp_path):
    from test_gpu_validation_cli import _setup, _run
    import random
    import multipoint_amd.datasets as datasets
    import multipoint_amd.utils as utils
    from multipoint_amd.utils.losses import SuperPointLoss
    from predict_align_image_pair import load_network
    config, cfg_path, mdir = _setup(tmp_path)
    out_bs, out_ev = str(tmp_path / 'bs.json'), str(tmp_path / 'ev.json')
    r = _run(['-y', cfg_path, '-m', mdir, '-s', '3', '-v', 'e1', '--batch-statistics', '--save-json', out_bs])
    assert r.returncode == 0, r.stdout + r.stderr
    r = _run(['-y', cfg_path, '-m', mdir, '-s', '3', '-v', 'e1', '--save-json', out_ev])
    assert r.returncode == 0, r.stdout + r.stderr
    bs, ev = json.load(open(out_bs)), json.load(open(out_ev))
    assert bs['eval_mode'] is False and ev['eval_mode'] is True
    # train.py's validation loop with set_batch_statistics(True) and SuperPointLoss called directly
    seed = 3
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
    val = dict(config['dataset'], filename=config['training']['validation']['filename'],
               keypoints_filename=config['training']['validation']['keypoints'])
    loader = torch.utils.data.DataLoader(datasets.ImagePairDataset(val), batch_size=config['training']['batchsize'], shuffle=False)
    net = load_network(config, mdir, 'e1', torch.device(DEV), seed)
    net.set_batch_statistics(True)
    loss_fn = SuperPointLoss(config['loss'])
    total = 0.0
    with torch.no_grad():
        for data in loader:
            data = utils.data_to_device(data, torch.device(DEV))
            loss, _ = loss_fn(net(data['optical']), data['optical'], net(data['thermal']), data['thermal'])
            total += float(loss)
    total /= len(loader)
    assert bs['versions']['e1']['loss'] == pytest.approx(total, rel=1e-6)
    assert abs(bs['versions']['e1']['loss'] - ev['versions']['e1']['loss']) > 1e-3 * abs(ev['versions']['e1']['loss'])
