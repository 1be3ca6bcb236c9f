"""Generate tests/golden/superpoint_loss.npz from the REFERENCE's SuperPointLoss (multipoint/utils/losses.py), imported in
place through ref_shim (nothing of it is copied).  Run from the repository root where the reference checkout exists:

    python tests/golden/make_golden_loss.py

Per case (tests/loss_restatement.py: CASES, make_case_inputs) it stores the inputs (logits / descriptors as int8 codes of
exact fp32 values), the torch seed, the reference's five loss components, the number of corresponding valid pairs per
image and the number of valid pairs whose fp32 distance lies within 1e-5 * threshold of the threshold (the pairs whose
decision another correctly computed fp32 distance may take the other way)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_shim  # noqa: E402
import loss_restatement as R  # noqa: E402


def reference_counts(RH, inputs, cfg):
    """Correspondence and near-threshold counts of the reference's own warped centres and distances."""
    B, H, W = inputs['keypoints1'].shape
    Hc, Wc = H // 8, W // 8
    coord = torch.stack(torch.meshgrid(torch.arange(Hc), torch.arange(Wc), indexing='ij'), dim=-1) * 8.0 + 4.0
    coord = coord.unsqueeze(0).expand([B, -1, -1, -1]).reshape(B, -1, 2).clone()
    warped = []
    for side in (1, 2):
        h = inputs.get('homography%d' % side)
        warped.append(coord if h is None else RH.warp_points_pytorch(coord, torch.from_numpy(h).inverse()))
    dist = (warped[0].unsqueeze(1) - warped[1].unsqueeze(2)).norm(dim=-1)          # [b][i (side 2)][j (side 1)]
    thr = cfg['descriptor_loss_threshold']
    if cfg['descriptor_loss_use_mask']:
        v1 = torch.from_numpy(R.cell_valid(inputs['valid_mask1'], B, H, W)).reshape(B, 1, -1)
        v2 = torch.from_numpy(R.cell_valid(inputs['valid_mask2'], B, H, W)).reshape(B, -1, 1)
        m = v1 & v2
    else:
        m = torch.ones_like(dist, dtype=torch.bool)
    corr = ((dist <= thr) & m).reshape(B, -1).sum(1).numpy()
    near = (((dist - thr).abs() <= 1e-5 * thr) & m).reshape(B, -1).sum(1).numpy()
    return corr.astype(np.int64), near.astype(np.int64)


def main():
    ref_shim.install()
    import multipoint.utils.homographies as RH
    import multipoint.utils.losses as RL
    out = {}
    for case in R.CASES:
        name, seed = case[0], case[1]
        q = R.make_case_inputs(case)
        inputs = R.dequantize(q)
        cfg = dict(R.DEFAULTS, **R.case_config(case))
        pred, data = [], []
        for side in (1, 2):
            pred.append({'logits': torch.from_numpy(inputs['logits%d' % side]),
                         'desc': torch.from_numpy(inputs['desc%d' % side])})
            d = {'keypoints': torch.from_numpy(inputs['keypoints%d' % side]),
                 'valid_mask': torch.from_numpy(inputs['valid_mask%d' % side])}
            if 'homography%d' % side in inputs:
                d['homography'] = torch.from_numpy(inputs['homography%d' % side])
            data.append(d)
        torch.manual_seed(seed)
        loss, comp = RL.SuperPointLoss(dict(cfg))(pred[0], data[0], pred[1], data[1])
        corr, near = reference_counts(RH, inputs, cfg)
        for k, v in q.items():
            out['%s/%s' % (name, k)] = v
        out[name + '/seed'] = np.int64(seed)
        out[name + '/loss'] = np.float64(loss.item())
        out[name + '/components'] = np.array([comp[k] for k in R.COMPONENTS], np.float64)
        out[name + '/corr_count'] = corr
        out[name + '/near_count'] = near
        print('%-20s loss %.6f  %s  corr %s near %s' % (name, loss.item(), ' '.join('%s=%.6g' % (k, comp[k]) for k in R.COMPONENTS),
                                                      corr.tolist(), near.tolist()))
    path = os.path.join(HERE, 'superpoint_loss.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
