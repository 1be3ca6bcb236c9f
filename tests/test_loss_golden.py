"""CPU checks of the SuperPointLoss evaluation: the float64 restatement (tests/loss_restatement.py) against the reference's
losses stored in tests/golden/superpoint_loss.npz, and the configuration errors of multipoint_amd.utils.losses, which
must be raised before any device work."""
import os

import numpy as np
import pytest
import torch

import loss_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'superpoint_loss.npz')


def load_case(case):
    z = np.load(GOLDEN)
    name = case[0]
    q = {k.split('/', 1)[1]: z[k] for k in z.files if k.startswith(name + '/')}
    stored = {k: q.pop(k) for k in ('seed', 'loss', 'components', 'corr_count', 'near_count')}
    return R.dequantize(q), stored


def host_noise(seed, B, Hc, Wc):
    """The reference's two torch.rand draws (image 1, then image 2) under torch.manual_seed(seed)."""
    torch.manual_seed(int(seed))
    return torch.rand((B, 64, Hc, Wc)).numpy(), torch.rand((B, 64, Hc, Wc)).numpy()


@pytest.mark.parametrize('case', R.CASES, ids=[c[0] for c in R.CASES])
def test_restatement_matches_reference(case):
    inputs, stored = load_case(case)
    B, H, W = inputs['keypoints1'].shape
    cfg = R.case_config(case)
    n1, n2 = host_noise(stored['seed'], B, H // 8, W // 8) if cfg['detector_use_cross_entropy'] else (None, None)
    total, comp, desc = R.loss(inputs, cfg, n1, n2)
    for i, k in enumerate(R.COMPONENTS):
        assert comp[k] == pytest.approx(stored['components'][i], rel=1e-5), k
    assert total == pytest.approx(float(stored['loss']), rel=1e-5)
    # correspondence decisions: only pairs at the threshold (within 1e-5 * threshold) may go the other way
    diff = np.abs(desc[:, 2] - stored['corr_count'])
    assert np.all(diff <= stored['near_count']), (desc[:, 2], stored['corr_count'], stored['near_count'])


def test_identity_counts_are_analytic():
    """Identity homographies, threshold 8: a valid cell corresponds to itself and its valid 4-neighbours (distance exactly
    8.0) -- the golden count of the reference equals that closed form."""
    for case in R.CASES:
        if case[8] != 'identity':
            continue
        inputs, stored = load_case(case)
        B, H, W = inputs['keypoints1'].shape
        use_mask = R.case_config(case)['descriptor_loss_use_mask']
        v1 = R.cell_valid(inputs['valid_mask1'], B, H, W) if use_mask else np.ones((B, H // 8, W // 8), bool)
        v2 = R.cell_valid(inputs['valid_mask2'], B, H, W) if use_mask else np.ones((B, H // 8, W // 8), bool)
        assert np.array_equal(analytic_identity_count(v1, v2), stored['corr_count'])


def analytic_identity_count(v1, v2):
    """sum over cells (i side 2, j side 1) with j == i or a 4-neighbour of i, both valid."""
    n = (v1 & v2).reshape(len(v1), -1).sum(1)
    n = n + (v2[:, 1:, :] & v1[:, :-1, :]).reshape(len(v1), -1).sum(1) + (v2[:, :-1, :] & v1[:, 1:, :]).reshape(len(v1), -1).sum(1)
    n = n + (v2[:, :, 1:] & v1[:, :, :-1]).reshape(len(v1), -1).sum(1) + (v2[:, :, :-1] & v1[:, :, 1:]).reshape(len(v1), -1).sum(1)
    return n


def test_multi_keypoint_case_depends_on_the_noise():
    """The tie-break case is only a check if another draw of the noise changes the labels and the loss."""
    case = [c for c in R.CASES if c[10]][0]
    inputs, stored = load_case(case)
    B, H, W = inputs['keypoints1'].shape
    n1, n2 = host_noise(stored['seed'], B, H // 8, W // 8)
    m1, m2 = host_noise(int(stored['seed']) + 1, B, H // 8, W // 8)
    assert (R.detector_labels(inputs['keypoints1'], n1) != R.detector_labels(inputs['keypoints1'], m1)).sum() > 10
    a = R.loss(inputs, R.case_config(case), n1, n2)[1]['detector_loss1']
    b = R.loss(inputs, R.case_config(case), m1, m2)[1]['detector_loss1']
    assert abs(a - b) > 1e-3 * abs(a)


# ---- configuration errors, raised before any device work (these run without a GPU) ----

def _pred(B=1, Hc=2, Wc=2, D=64):
    return {'logits': torch.zeros(B, 65, Hc, Wc), 'desc': torch.zeros(B, D, Hc, Wc)}


def _data(B=1, H=16, W=16):
    return {'keypoints': torch.zeros(B, H, W, dtype=torch.bool), 'valid_mask': torch.ones(B, 1, H, W, dtype=torch.bool)}


def test_reference_surface():
    import multipoint_amd.utils.losses as L
    cls = getattr(L, 'SuperPointLoss')
    loss = cls({'lambda': 0.5, 'detector_use_cross_entropy': False})
    assert loss.config['lambda'] == 0.5 and loss.config['detector_use_cross_entropy'] is False
    assert loss.config['lambda_d'] == 250 and loss.config['descriptor_loss_threshold'] == 8.0
    assert cls.default_config['lambda'] == 0.0001                 # the class defaults are left alone
    assert set(cls.default_config) == {'detector_loss', 'detector_use_cross_entropy', 'descriptor_loss',
                                       'descriptor_loss_threshold', 'sparse_descriptor_loss',
                                       'sparse_descriptor_loss_num_cell_divisor', 'descriptor_loss_use_mask',
                                       'positive_margin', 'negative_margin', 'lambda_d', 'lambda'}
    assert loss.component_keys(True) == R.COMPONENTS


def test_bad_configurations_raise_before_device_work():
    import multipoint_amd.utils.losses as L
    with pytest.raises(NotImplementedError, match='sparse_descriptor_loss'):
        L.SuperPointLoss({'sparse_descriptor_loss': True})
    with pytest.raises(ValueError, match='label_noise'):
        L.SuperPointLoss({'label_noise': 'gpu'})
    loss = L.SuperPointLoss()
    with pytest.raises(ValueError, match='The data and the label must be present to compute the loss'):
        loss(_pred(), _data(), _pred(), None)
    with pytest.raises(ValueError, match='The data and the label must be present to compute the loss'):
        loss(_pred(), _data(), None, _data())
    with pytest.raises(ValueError, match='The descriptor loss requires predictions from two images'):
        loss(_pred(), _data())
    loss.config['sparse_descriptor_loss'] = True
    with pytest.raises(NotImplementedError, match='sparse_descriptor_loss'):
        loss(_pred(), _data(), _pred(), _data())
