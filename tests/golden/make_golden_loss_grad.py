"""Generate tests/golden/superpoint_loss_grad.npz: the gradients of the REFERENCE's SuperPointLoss
(multipoint/utils/losses.py), imported in place through ref_shim (nothing of it is copied), computed by torch autograd
on the CPU.  Run from the repository root where the reference checkout exists:

    python tests/golden/make_golden_loss_grad.py

The cases are tests/loss_restatement.py's CASES with their seeds, except the 240x320 one; the inputs are those of
tests/golden/superpoint_loss.npz (make_case_inputs).  `loss.backward()` of the total loss (upstream gradient 1); per case
the fp32 gradients of image 0 of logits1, logits2, desc1 and desc2 are stored (the file stays small)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402
import loss_restatement as R  # noqa: E402

GRAD_CASES = [c for c in R.CASES if c[0] != 'ce_240x320']
NAMES = ('logits1', 'logits2', 'desc1', 'desc2')


def main():
    ref_shim.install()
    import multipoint.utils.losses as RL
    out = {}
    for case in GRAD_CASES:
        name, seed = case[0], case[1]
        inputs = R.dequantize(R.make_case_inputs(case))
        cfg = dict(R.DEFAULTS, **R.case_config(case))
        leaves = {k: torch.from_numpy(inputs[k]).requires_grad_() for k in NAMES}
        pred, data = [], []
        for side in (1, 2):
            pred.append({'logits': leaves['logits%d' % side], 'desc': leaves['desc%d' % side]})
            d = {'keypoints': torch.from_numpy(inputs['keypoints%d' % side]),
                 'valid_mask': torch.from_numpy(inputs['valid_mask%d' % side])}
            if 'homography%d' % side in inputs:
                d['homography'] = torch.from_numpy(inputs['homography%d' % side])
            data.append(d)
        torch.manual_seed(seed)
        loss, _ = RL.SuperPointLoss(dict(cfg))(pred[0], data[0], pred[1], data[1])
        loss.backward()
        for k in NAMES:
            out['%s/%s' % (name, k)] = leaves[k].grad[0].numpy().astype(np.float32)
        out[name + '/loss'] = np.float64(loss.item())
        print('%-20s loss %.6f  max|grad| %s' % (name, loss.item(), ' '.join(
            '%s=%.3g' % (k, float(leaves[k].grad.abs().max())) for k in NAMES)))
    path = os.path.join(HERE, 'superpoint_loss_grad.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
