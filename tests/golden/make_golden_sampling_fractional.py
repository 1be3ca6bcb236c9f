#!/usr/bin/env python3
"""Generates tests/golden/sampling_fractional.npz by IMPORTING the reference on PyTorch-CPU.
Run where the reference checkout is available (ref_shim.REFERENCE_ROOT):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sampling_fractional.py

The fixture holds what the reference's interpolate_descriptors (multipoint/utils/utils.py:159-167) returns for FRACTIONAL
keypoints -- its keypoints.float() admits them -- next to its inputs: a D = 64 coarse map of 6 x 8 cells for a 48 x 64 frame and
32 (y, x) positions, among them the four corners of the coarse grid (exactly on it), positions a rounding away from inner grid
nodes, the frame's last row and column, and positions slightly outside the frame (taps beyond the map are zero: grid_sample's
padding).  Data only, never reference source."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402

models, utils = ref_shim.install()

D, Hc, Wc, H, W = 64, 6, 8, 48, 64
rng = np.random.default_rng(20)
desc = rng.standard_normal((D, Hc, Wc)).astype(np.float32)
special = [
    (0.0, 0.0), (0.0, W), (H, 0.0), (H, W),                                   # the coarse grid's corners, exactly on it
    (H / 5.0, W / 7.0), (2 * H / 5.0, 3 * W / 7.0), (4 * H / 5.0, 6 * W / 7.0),   # inner nodes, to a rounding
    (H - 1.0, 10.25), (17.5, W - 1.0), (H - 1.0, W - 1.0),                    # the frame's last row and column
    (-0.3, 20.0), (12.0, -0.45), (H + 0.4, 33.3), (30.7, W + 0.25), (-0.2, -0.2), (H + 0.3, W + 0.3),     # slightly outside
]
n_rand = 32 - len(special)
kp = np.concatenate([np.array(special, np.float64),
                     np.stack([rng.uniform(0, H - 1, n_rand), rng.uniform(0, W - 1, n_rand)], 1)]).astype(np.float32)
assert kp.shape == (32, 2)
kp_t = torch.from_numpy(kp.copy())             # (a float tensor is normalised IN PLACE by the reference: give it a copy)
out = utils.interpolate_descriptors(kp_t, torch.from_numpy(desc), H, W).numpy()
assert out.shape == (32, D) and np.isfinite(out).all()

path = os.path.join(HERE, 'sampling_fractional.npz')
np.savez_compressed(path, desc=desc, kp=kp, H=np.array(H), W=np.array(W), out=out)
print('wrote %s (%d bytes)' % (path, os.path.getsize(path)))
