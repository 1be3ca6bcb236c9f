"""Generator of tests/golden/first_block_parent_bits.npz (GPU, MI355X): prob and desc of the default (`auto`) fp32 forward, recorded
from the build BEFORE the fused first-block launch (conv_wino43.hip, F1) took its weights by MFMA broadcast and kept the second
block's taps in registers.  That change re-places LDS instructions and changes no multiply-add, so every later build must return
these bits (tests/test_gpu_first_block_bits.py).

    python tests/make_golden_first_block.py [--out FILE]

Cases (name -> B, H, W, MP_DEBUG), each for the shipped configuration and for bn_first (the first block's BatchNorm is then folded
into its weights instead of the second convolution's):
    one_item     (1, 16, 32)   one item, every edge of its patch reflected
    edge_items   (2, 32, 64)   edge items only
    interior     (3, 48, 96)   one interior item per image
    walk27       (3, 48, 96)   ncu=8,nxcd=1: 8 workgroups walk 27 items -- interior <-> edge cursor changes, the patch-buffer flip and
                               the patch prefetch of item k + 2
    walk_deep    (2, 64, 64)   ncu=8,nxcd=1: conv3 .. conv8 with several items per workgroup as well
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(HERE, 'golden', 'first_block_parent_bits.npz')
SEED = 20
CONFIGS = [('shipped', {}), ('bn_first', {'bn_first': True})]
CASES = [('one_item', 1, 16, 32, ''), ('edge_items', 2, 32, 64, ''), ('interior', 3, 48, 96, ''),
         ('walk27', 3, 48, 96, 'ncu=8,nxcd=1'), ('walk_deep', 2, 64, 64, 'ncu=8,nxcd=1')]


def images(B, H, W):
    """B frames of SyntheticPairs (optical, thermal, optical, ... of pairs 0, 1, ..), seeded."""
    import torch
    from multipoint_amd.datasets.synthetic_pairs import SyntheticPairs
    frames = [SyntheticPairs.make_pair(SEED + H + W, b // 2, H, W)[b % 2] for b in range(B)]
    return torch.from_numpy(np.stack(frames))


def run_case(cfg_upd, B, H, W, debug):
    """prob, desc (numpy) of a NEW handle created under MP_DEBUG=debug (the library reads it when the handle is made)."""
    import multipoint_amd.models as M
    from oracle import mp_oracle as O
    cfg = dict(O.SHIPPED_MODEL_CONFIG); cfg.update(cfg_upd)
    sd = O.make_weights(0, cfg)
    old = os.environ.get('MP_DEBUG')
    if debug:
        os.environ['MP_DEBUG'] = debug
    else:
        os.environ.pop('MP_DEBUG', None)
    try:
        net = M.MultiPoint(cfg); net.load_state_dict(sd); net.to('cuda'); net.eval()
        out = net({'image': images(B, H, W).cuda()})
        return out['prob'].cpu().numpy(), out['desc'].cpu().numpy()
    finally:
        if old is None:
            os.environ.pop('MP_DEBUG', None)
        else:
            os.environ['MP_DEBUG'] = old


def main(argv):
    out = argv[argv.index('--out') + 1] if '--out' in argv else GOLDEN
    arrays = {}
    for cname, upd in CONFIGS:
        for name, B, H, W, debug in CASES:
            prob, desc = run_case(upd, B, H, W, debug)
            assert np.isfinite(prob).all() and np.isfinite(desc).all()
            arrays['%s.%s.prob' % (cname, name)] = prob
            arrays['%s.%s.desc' % (cname, name)] = desc
            print(cname, name, prob.shape, desc.shape, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **arrays)
    print('wrote %s: %d bytes' % (out, os.path.getsize(out)))


if __name__ == '__main__':
    main(sys.argv[1:])
