"""Generate tests/golden/batch_statistics.npz from the REFERENCE's MultiPoint (multipoint/models/MultiPoint.py) in its default
TRAINING mode -- the mode train.py's validation loop runs it in (it never calls net.eval()) -- imported in place through
ref_shim (nothing of it is copied).  Run from the repository root where the reference checkout exists:

    python tests/golden/make_golden_batch_stats.py

Per case (tests/batch_stats_restatement.py: CASES) the weights and images are regenerated from the seed; stored are the
images, is_optical, the reference's logits and descriptors (fp32, under torch.no_grad()) and every BatchNorm layer's running
mean / variance AFTER the forward (momentum 0.1 blend of the batch statistics into the seeded running statistics)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_shim  # noqa: E402
import batch_stats_restatement as R  # noqa: E402

SEED = 3


def main():
    ref_shim.install()
    from multipoint.models.MultiPoint import MultiPoint as RefMultiPoint
    torch.manual_seed(0)
    out = {'seed': np.int64(SEED)}
    for i, case in enumerate(R.CASES):
        name = case[0]
        cfg = R.case_config(case)
        sd = R.case_weights(case, SEED + i)
        img, opt = R.case_inputs(case, SEED + i)
        net = RefMultiPoint({k: v for k, v in cfg.items() if k != 'type'})
        net.load_state_dict(sd)                  # the default mode: training (train.py never calls net.eval())
        assert net.training
        data = {'image': img}
        if opt is not None:
            data['is_optical'] = opt
        with torch.no_grad():
            pred = net(data)
        assert pred['prob'] is None
        out[name + '/image'] = img.numpy()
        if opt is not None:
            out[name + '/is_optical'] = opt.numpy().astype(np.uint8)
        out[name + '/logits'] = pred['logits'].numpy()
        if 'desc' in pred:
            out[name + '/desc'] = pred['desc'].numpy()
        after = net.state_dict()
        for p in R.bn_prefixes(cfg):
            out['%s/running/%s' % (name, p)] = np.stack([after[p + '.running_mean'].numpy(), after[p + '.running_var'].numpy()])
    path = os.path.join(HERE, 'batch_statistics.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
