"""Batch-statistics (training-mode) forward, CPU side: the reference fixture tests/golden/batch_statistics.npz against the
float64 restatement (tests/batch_stats_restatement.py), and the argument checks that need no GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import batch_stats_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'batch_statistics.npz'))


@pytest.mark.parametrize('idx', range(len(R.CASES)), ids=[c[0] for c in R.CASES])
def test_fixture_matches_float64_restatement(golden, idx):
    case = R.CASES[idx]
    name, cfg, seed = case[0], R.case_config(case), int(golden['seed']) + idx
    sd = R.case_weights(case, seed)
    img, opt = R.case_inputs(case, seed)
    assert np.array_equal(golden[name + '/image'], img.numpy())           # the seeded inputs regenerate bit for bit
    if opt is not None:
        assert np.array_equal(golden[name + '/is_optical'].astype(bool), opt.numpy())
    logits, desc, stats = R.forward_train64(sd, img, cfg, opt)
    # the reference's fp32 forward against float64: 9e-5 (logits, |logit| <= 9) / 9e-6 (unit descriptors) over these cases
    assert np.abs(golden[name + '/logits'] - logits.numpy()).max() < 2e-4
    assert np.abs(golden[name + '/desc'] - desc.numpy()).max() < 2e-5
    blended = R.blend_running(sd, stats)
    for p in R.bn_prefixes(cfg):
        got = golden['%s/running/%s' % (name, p)]
        if p in blended:
            want = np.stack([t.numpy() for t in blended[p]])
            assert np.abs(got - want).max() <= 2e-6 * (1 + np.abs(want).max()), p
        else:       # an encoder without images does not run: its running statistics are untouched
            assert np.array_equal(got, np.stack([sd[p + '.running_mean'].numpy(), sd[p + '.running_var'].numpy()])), p


def test_fixture_covers_the_issue_configs(golden):
    from oracle import mp_oracle as O
    cfgs = [O.full_config(R.case_config(c)) for c in R.CASES]
    assert any(c['bn_first'] for c in cfgs) and any(not c['final_batchnorm'] for c in cfgs)
    assert any(not c['double_convolution'] for c in cfgs) and any(not c['reflection_pad'] for c in cfgs)
    assert {c.get('channel_version', 0) for c in cfgs} == {0, 1, 2}
    assert {c['descriptor_size'] for c in cfgs} >= {64, 128, 256}
    ms = [c for c in R.CASES if c[5] is not None]
    assert any(0 < sum(c[5]) < len(c[5]) for c in ms) and any(sum(c[5]) == len(c[5]) for c in ms)


def _model(**over):
    from oracle import mp_oracle as O
    from multipoint_amd.models import MultiPoint
    return MultiPoint(dict(O.SHIPPED_MODEL_CONFIG, **over))


def test_set_batch_statistics_validates_like_set_force_return_logits():
    net = _model()
    for bad in (1, 0, None, 'yes', np.bool_(True)):
        with pytest.raises(ValueError, match='needs to be a bool'):
            net.set_batch_statistics(bad)
    net.set_batch_statistics(True)
    assert net.training is False
    with pytest.raises(NotImplementedError):
        net.train()
    net.set_batch_statistics(False)
    with pytest.raises(RuntimeError, match='no forward'):
        net.last_batch_statistics()


def test_refusals_before_any_launch():
    with pytest.raises(NotImplementedError, match='mixed_precision'):
        _model(mixed_precision=True)._check_batch_statistics(2, 64, 64, None)
    from multipoint_amd.models import SuperPointMagicLeap
    ml = SuperPointMagicLeap()
    with pytest.raises(NotImplementedError, match='no BatchNorm'):
        ml._check_batch_statistics(2, 64, 64, None)
    net = _model()
    with pytest.raises(ValueError, match='more than 1 value per channel'):
        net._check_batch_statistics(1, 8, 8, None)
    net._check_batch_statistics(2, 8, 8, None)
    net._check_batch_statistics(1, 8, 16, None)
    ms = _model(multispectral=True)
    with pytest.raises(ValueError, match='more than 1 value per channel'):      # one optical image at 8x8: its encoder's layers
        ms._check_batch_statistics(3, 8, 8, torch.tensor([1, 0, 0], dtype=torch.uint8))
    ms._check_batch_statistics(3, 8, 8, torch.tensor([0, 0, 0], dtype=torch.uint8))


def test_abi_declares_the_entry_points():
    from multipoint_amd import _lib, build
    hdr = open(os.path.join(ROOT, 'include', 'multipoint_hip.h')).read()
    for fn in ('mp_forward_batch_stats', 'mp_batch_stats_count', 'mp_batch_stats_layer'):
        assert fn in _lib.SIGNATURES and (fn + '(') in hdr
    assert 'batchnorm_stats.hip' in build.SOURCES and build.SCRATCH_CAPS['batchnorm_stats.hip'] == 0


def test_cli_flag_and_description():
    sys.path.insert(0, ROOT)
    import compute_validation_loss as C
    args = C.build_parser().parse_args(['--batch-statistics'])
    assert args.batch_statistics is True
    assert C.build_parser().parse_args([]).batch_statistics is False
    assert '--batch-statistics' in C.DESCRIPTION and 'DataParallel' in C.DESCRIPTION
