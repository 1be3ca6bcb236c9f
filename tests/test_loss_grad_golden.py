"""CPU checks of the float64 gradient restatement (tests/loss_grad_restatement.py) against the gradients of the
reference's SuperPointLoss stored in tests/golden/superpoint_loss_grad.npz (torch autograd, fp32, image 0 of each case).
The measured fp32 error of the reference (reference_error) is what the GPU tolerance is built from."""
import os

import numpy as np
import pytest

import loss_grad_restatement as RG
import loss_restatement as R
from test_loss_golden import host_noise, load_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'superpoint_loss_grad.npz')
GRAD_CASES = [c for c in R.CASES if c[0] != 'ce_240x320']
NAMES = ('logits1', 'logits2', 'desc1', 'desc2')
KEYS = ('detector_loss1', 'detector_loss2', 'descriptor_loss', 'positive_dist', 'negative_dist')


def load_grad_case(case):
    """(inputs, stored loss values, {name: reference fp32 gradient of image 0}, host noise pair or (None, None))."""
    inputs, stored = load_case(case)
    z = np.load(GOLDEN)
    ref = {k: z['%s/%s' % (case[0], k)] for k in NAMES}
    B, H, W = inputs['keypoints1'].shape
    noise = host_noise(stored['seed'], B, H // 8, W // 8) if R.case_config(case)['detector_use_cross_entropy'] else (None, None)
    return inputs, stored, ref, noise


def reference_error(case):
    """{name: max |reference fp32 gradient - float64 restatement|} over image 0, the restatement on float64 centres."""
    inputs, _, ref, noise = load_grad_case(case)
    g = RG.grads(inputs, R.case_config(case), KEYS, {'total': 1.0}, noise[0], noise[1])
    return {k: float(np.abs(g[k][0] - ref[k].astype(np.float64)).max()) for k in NAMES}


@pytest.mark.parametrize('case', GRAD_CASES, ids=[c[0] for c in GRAD_CASES])
def test_restatement_matches_reference_gradients(case):
    """The restatement equals the reference's autograd within fp32 rounding: a few 1e-7 of the largest gradient."""
    _, _, ref, _ = load_grad_case(case)
    err = reference_error(case)
    for k in NAMES:
        assert np.abs(ref[k]).max() > 0, k
        assert err[k] <= 2e-6 * np.abs(ref[k]).max(), (k, err[k])


def test_tie_rule_matters():
    """A hinge at exactly 0 has derivative 1/2: 0 or 1 there moves the gradient of a pair on the margin."""
    assert RG.hinge(np.array([-1.0, 0.0, 1.0])).tolist() == [0.0, 0.5, 1.0]


def test_device_noise_restatement_is_a_uniform_draw():
    u = RG.device_noise(3, 2, 4, 5)
    assert u.dtype == np.float32 and u.shape == (2, 64, 4, 5)
    assert 0.0 <= u.min() and u.max() < 1.0 and 0.4 < u.mean() < 0.6
    assert not np.array_equal(u, RG.device_noise(4, 2, 4, 5))


def test_fixture_is_small():
    assert os.path.getsize(GOLDEN) < 700 * 1024
