#!/usr/bin/env python3
"""Generates tests/golden/reference_drivers.npz by IMPORTING the reference on PyTorch-CPU.
Run where the reference checkout is available (ref_shim.REFERENCE_ROOT):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_reference.py

The fixture holds what the reference's own code returns -- model state-dict layouts, forwards, its host helpers, its
matchers, its evaluation / homographic-adaptation drivers (run with the oracle serving the absent third-party calls,
exactly as tests/test_oracle_vs_reference.py did against the imported reference) -- so that test module needs no
reference checkout.  Inputs are NOT stored where they come from seeds (oracle.make_weights / make_images, numpy
default_rng): the tests rebuild them.  The detector-metrics driver's probability maps are stored as
well (values at or below the detection threshold zeroed: its box-NMS reads only prob > threshold): its bookkeeping is
compared exactly, and float32 forwards differ in the last bits between CPUs.  Image sizes are small to keep the fixture
small.  Data only, never
reference source."""
import collections
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import ref_shim  # noqa: E402
from oracle import mp_oracle as O  # noqa: E402
from oracle import ha_oracle as HA  # noqa: E402

models, utils = ref_shim.install()
RH = ref_shim.install_homographies()
import multipoint.utils.evaluation as ev  # noqa: E402
import multipoint.utils.utils as ru  # noqa: E402

cv2 = sys.modules['cv2']
G = {}


def put_layout(prefix, net):
    sd = net.state_dict()
    G[prefix + '__keys'] = np.array(list(sd.keys()))
    G[prefix + '__shapes'] = np.array(json.dumps([list(v.shape) for v in sd.values()]))
    G[prefix + '__dtypes'] = np.array([str(v.dtype) for v in sd.values()])


def put_forward(prefix, r, keys=('prob', 'desc')):
    for k in keys:
        G[prefix + '__' + k] = r[k].numpy()


def ref_net(cfg, sd=None):
    net = models.MultiPoint(dict(cfg)).eval()
    if sd is not None:
        net.load_state_dict(sd)
    return net


def ref_forward(cfg, sd, data):
    with torch.no_grad():
        return ref_net(cfg, sd)(data)


def nms(boxes, scores, iou):
    keep = O.nms_greedy(boxes.numpy().astype(np.float32), scores.numpy().astype(np.float32), float(iou))
    return torch.as_tensor(np.asarray(keep), dtype=torch.int64)


def batched_nms(boxes, scores, idxs, iou):
    keep = []
    for i in torch.unique(idxs):
        sel = torch.nonzero(idxs == i)[:, 0]
        keep.append(sel[nms(boxes[sel], scores[sel], iou)])
    keep = torch.cat(keep) if keep else torch.zeros(0, dtype=torch.int64)
    return keep[torch.argsort(scores[keep], descending=True, stable=True)]


class BFMatcher:
    def __init__(self, norm, crossCheck=False):
        assert crossCheck

    def match(self, d1, d2):
        q, t, d = O.bf_match_crosscheck(d1, d2)
        return [cv2.DMatch(int(a), int(b), float(c)) for a, b, c in zip(q, t, d)]


class KeyPoint:
    def __init__(self, x, y, size):
        self.pt = (x, y)


ru.nms = nms
ru.batched_nms = batched_nms
cv2.BFMatcher = BFMatcher
cv2.perspectiveTransform = lambda pts, h: O.warp_keypoints(pts[0][:, ::-1], h)[None, :, ::-1]   # oracle: (y, x)
cv2.KeyPoint = KeyPoint
cv2.findHomography = lambda *a, **k: (None, None)
cv2.RANSAC = 8
cv2.NORM_L2 = 4


def raises_value_error(fn):
    try:
        fn()
    except ValueError:
        return True
    return False


# ---- forwards and state-dict layouts --------------------------------------------------------------------------
cfg = dict(O.SHIPPED_MODEL_CONFIG)
put_layout('shipped', ref_net(cfg))
put_forward('shipped', ref_forward(cfg, O.make_weights(21, cfg), {'image': O.make_images(22, 2, 48, 64)}))

cfg = {'multispectral': True, 'descriptor_size': 128}
put_layout('multispectral', ref_net(cfg))
flags = torch.tensor([[True], [False], [False], [True]])
put_forward('multispectral', ref_forward(cfg, O.make_weights(5, cfg), {'image': O.make_images(6, 4, 24, 32), 'is_optical': flags}))

for name, upd in (('cv1', {'channel_version': 1}), ('cv2', {'channel_version': 2, 'descriptor_size': 128})):
    cfg = dict(O.SHIPPED_MODEL_CONFIG); cfg.update(upd)
    put_layout(name, ref_net(cfg))
    put_forward(name, ref_forward(cfg, O.make_weights(51, cfg), {'image': O.make_images(52, 2, 32, 48)}))

net = models.SuperPointMagicLeap().eval()
put_layout('magicleap', net)
net.load_state_dict(O.make_weights_magicleap(8))
with torch.no_grad():
    put_forward('magicleap', net({'image': O.make_images(9, 2, 24, 32)}), ('logits', 'desc', 'prob'))

# ---- host helpers ---------------------------------------------------------------------------------------------
a = {'a': 1, 'b': {'c': 2, 'd': 3}}; b = {'b': {'c': 5}, 'e': 6}
G['helpers__dict_update'] = np.array(json.dumps(utils.dict_update(copy.deepcopy(a), b)))
w = collections.OrderedDict([('module__encoder.1.weight', 1), ('x__y__detector.4.bias', 2), ('plain', 3)])
G['helpers__fix_keys'] = np.array(json.dumps(list(utils.fix_model_weigth_keys(w).items())))
x = torch.from_numpy(np.random.default_rng(4).standard_normal((2, 64, 3, 4)).astype(np.float32))
G['helpers__d2s_in'] = x.numpy()
G['helpers__d2s_out'] = utils.depth_to_space(x, 8).numpy()
G['helpers__default_config'] = np.array(json.dumps(models.MultiPoint.default_config, sort_keys=True))
for i, cfg in enumerate(({'multispectral': False, 'descriptor_size': 64}, {'bn_first': True}, {'final_batchnorm': False})):
    put_layout('helpers_cfg%d' % i, ref_net(cfg))

# ---- descriptor sampling and matchers -------------------------------------------------------------------------
rng = np.random.default_rng(1)
desc = rng.standard_normal((16, 60, 80)).astype(np.float32)
kp = np.stack([rng.integers(0, 480, 500), rng.integers(0, 640, 500)], 1).astype(np.int64)
kp_t = torch.from_numpy(kp.copy())
r = utils.interpolate_descriptors(kp_t, torch.from_numpy(desc), 480, 640).numpy()
assert np.array_equal(kp_t.numpy(), kp)
G['interp__desc'] = r
m = utils.NNMatcher(0.7).match(r[:250], r[200:])
G['interp__nn_query'] = np.array([x.queryIdx for x in m], np.int64)
G['interp__nn_train'] = np.array([x.trainIdx for x in m], np.int64)
G['interp__nn_distance'] = np.array([x.distance for x in m], np.float64)
G['interp__nn_negative_raises'] = np.array(raises_value_error(lambda: utils.NNMatcher(-1.0)))

rng = np.random.default_rng(8)
d1 = rng.standard_normal((120, 64)).astype(np.float32); d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
d2 = np.concatenate([d1[:60] + 0.05 * rng.standard_normal((60, 64)).astype(np.float32),
                     rng.standard_normal((50, 64)).astype(np.float32)]); d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
for thr in (0.4, 0.7, 1.3):
    m = utils.get_matches(d1, d2, 'thresholdmatcher', threshold=thr)
    G['thr%g__query' % thr] = np.array([x.queryIdx for x in m], np.int64)
    G['thr%g__train' % thr] = np.array([x.trainIdx for x in m], np.int64)
    G['thr%g__distance' % thr] = np.array([x.distance for x in m], np.float32)
G['thr__negative_raises'] = np.array(raises_value_error(lambda: utils.ThresholdMatcher(-0.5)))

# ---- evaluation drivers ---------------------------------------------------------------------------------------
cfg = dict(O.SHIPPED_MODEL_CONFIG)
sd = O.make_weights(31, cfg)
H, W, B = 96, 128, 3
rng = np.random.default_rng(5)
opt = O.make_images(41, B, H, W)
th = (opt + 0.02 * torch.from_numpy(rng.standard_normal(opt.shape).astype(np.float32))).clamp(0, 1)
ho = torch.eye(3).repeat(B, 1, 1); ht = torch.eye(3).repeat(B, 1, 1)
ht[:, 0, 2] = torch.tensor([0.0, 1.0, -2.0]); ht[1, 0, 0] = 1.01
ones = torch.ones((B, 1, H, W), dtype=torch.bool)
batch = {'optical': {'image': opt, 'valid_mask': ones, 'homography': ho, 'is_optical': torch.ones(B, 1, dtype=torch.bool)},
         'thermal': {'image': th, 'valid_mask': ones, 'homography': ht, 'is_optical': torch.zeros(B, 1, dtype=torch.bool)}}
pred = {'nms': 4, 'detection_threshold': 0.015, 'topk': 150, 'cpu_nms': True, 'reprojection_threshold': 3,
        'matching': {'method': 'bfmatcher', 'method_kwargs': {'crossCheck': True}, 'knn_matches': False}}
with torch.no_grad():
    r = ev.compute_descriptor_metrics(ref_net(cfg, sd), [batch], torch.device('cpu'), pred, 4.0, 4.0)
for k in ('tp_optical', 'tp_thermal', 'distance_optical', 'm_score_optical', 'm_score_thermal', 'm_score',
          'nn_map_optical', 'nn_map_thermal', 'recall_optical'):
    G['descmetrics__' + k] = np.asarray(r[k], np.float64)

sd = O.make_weights(33, cfg)
rng = np.random.default_rng(6)
opt = O.make_images(43, B, H, W)
th = (opt + 0.02 * torch.from_numpy(rng.standard_normal(opt.shape).astype(np.float32))).clamp(0, 1)
ho = torch.eye(3).repeat(B, 1, 1); ht = torch.eye(3).repeat(B, 1, 1)
ht[:, 0, 2] = torch.tensor([0.0, 2.0, -3.0]); ho[2, 1, 2] = 1.5; ht[1, 0, 0] = 1.02
batch = {'optical': {'image': opt, 'valid_mask': ones, 'homography': ho}, 'thermal': {'image': th, 'valid_mask': ones, 'homography': ht}}
with torch.no_grad():
    mean, rep, n_o, n_t = ev.compute_repeatability_multispectral(
        ref_net(cfg, sd), [batch], torch.device('cpu'), {'prediction': {'nms': 4, 'detection_threshold': 0.015, 'topk': 120,
                                                                     'cpu_nms': True}}, distance_thresh=3)
G['repeat__mean'] = np.array(mean, np.float64)
G['repeat__rep'] = np.asarray(rep, np.float64)
G['repeat__n_optical'] = np.asarray(n_o, np.int64)
G['repeat__n_thermal'] = np.asarray(n_t, np.int64)

rng = np.random.default_rng(3)
for case in range(6):
    H, W = 40, 56
    prob = np.zeros((H, W), np.float32)
    n = [60, 200, 5, 0, 400, 1][case]
    idx = rng.choice(H * W, n, replace=False)
    prob.flat[idx] = rng.permutation(n).astype(np.float32) / max(n, 1) * 0.9 + 0.01
    km = np.zeros((H, W), bool)
    g = [40, 150, 0, 10, 300, 1][case]
    gi = np.concatenate([rng.choice(idx, min(g // 2, n), replace=False), rng.choice(H * W, g - min(g // 2, n), replace=False)]) if g else np.zeros(0, int)
    km.flat[gi.astype(int)] = True
    if case == 5:
        km[:] = False; km.flat[idx[0]] = True
    if n == 0:
        continue                                         # the reference's indexing fails on an empty prediction list
    r = ev.compute_tp_fp_dist(torch.from_numpy(prob), torch.from_numpy(km))
    for j, k in enumerate(('tp', 'fp', 'prob', 'n_gt', 'dist')):
        G['tpfp%d__%s' % (case, k)] = np.asarray(r[j])
H, W = 64, 96
sd = O.make_weights(31, cfg)
batches = []
for b in range(2):
    img = O.make_images(50 + b, 2, H, W)
    vm = torch.ones((2, 1, H, W), dtype=torch.bool); vm[:, :, :6] = False
    with torch.no_grad():
        pr = O.forward(sd, img, cfg)['prob'] * vm
    G['detmetrics__prob_map%d' % b] = np.where(pr.numpy() > 0.015, pr.numpy(), 0)    # box-NMS reads prob > threshold only
    pn = O.box_nms(pr.numpy(), 4, 0.015)
    km = torch.zeros((2, H, W), dtype=torch.bool)
    for i in range(2):
        kept = np.argwhere(pn[i, 0] > 0.015)
        sel = kept[rng.choice(len(kept), len(kept) // 2, replace=False)]
        sel = np.clip(sel + rng.integers(-2, 3, sel.shape), 0, [H - 1, W - 1])
        km[i, sel[:, 0], sel[:, 1]] = True
    batches.append({'image': img, 'valid_mask': vm, 'keypoints': km, 'is_optical': torch.ones(2, 1, dtype=torch.bool)})
with torch.no_grad():
    precision, recall, prob, dist = ev.compute_detector_metrics(ref_net(cfg, sd), batches,
                                                                torch.device('cpu'), {'nms': 4, 'detection_threshold': 0.015})
for k, v in (('precision', precision), ('recall', recall), ('prob', prob), ('dist', dist)):
    G['detmetrics__' + k] = np.asarray(v)
G['detmetrics__map'] = np.array(ev.compute_mAP(precision, recall), np.float64)

# ---- homographic adaptation -----------------------------------------------------------------------------------
from multipoint_amd.utils.homographies import homography_adaptation_default_config  # noqa: E402
cases = [{}, {'allow_artifacts': False, 'max_angle': 0.4}, {'perspective': False, 'n_scales': 3},
         {'rotation': False, 'translation': False, 'scaling_amplitude': 0.5},
         dict(homography_adaptation_default_config['homographies'])]
mats, states = [], []
for seed in range(100, 112):
    for kw in cases:
        for shape in ((240, 320), (64, 64)):
            np.random.seed(seed)
            mats.append(RH.sample_homography(np.array(shape), **kw))
            states.append(np.random.get_state()[1][:4].copy())
G['sample_h__cases'] = np.array(json.dumps(cases))
G['sample_h__mats'] = np.array(mats, np.float64)
G['sample_h__states'] = np.array(states)

pristine = copy.deepcopy(RH.homography_adaptation_default_config)
HA_CASES = ((False, {'num': 3, 'erosion_radius': 2, 'mask_border': True, 'min_count': 2, 'filter_size': 0}),
            (False, {'num': 3, 'erosion_radius': 4, 'mask_border': False, 'min_count': 0, 'filter_size': 5}),
            (True, {'num': 3, 'aggregation': 'prod', 'erosion_radius': 3, 'min_count': 3}),
            (True, {'num': 2, 'aggregation': 'sum', 'erosion_radius': 0, 'filter_size': 3}))
for c, (pair, hc) in enumerate(HA_CASES):
    cfg = {'multispectral': True, 'descriptor_size': 64} if pair else dict(O.SHIPPED_MODEL_CONFIG)
    net = ref_net(cfg, O.make_weights(17, cfg))
    img = O.make_images(41, 4 if pair else 2, 32, 40)
    RH.homography_adaptation_default_config.clear()      # the reference's dict_update writes into its default
    RH.homography_adaptation_default_config.update(copy.deepcopy(pristine))
    np.random.seed(23)
    with torch.no_grad():
        if pair:
            fl = [torch.ones(2, 1, dtype=torch.bool), torch.zeros(2, 1, dtype=torch.bool)]
            data = {'optical': {'image': img[:2], 'is_optical': fl[0]}, 'thermal': {'image': img[2:], 'is_optical': fl[1]}}
            want = RH.homographic_adaptation_multispectral(data, net, copy.deepcopy(hc))
        else:
            want = RH.homographic_adaptation({'image': img}, net, copy.deepcopy(hc))
    G['ha%d__prob' % c] = want.numpy()
    full = HA.full_config(hc)
    np.random.seed(23)
    G['ha%d__homs' % c] = np.array([RH.sample_homography(np.array([32, 40]), **full['homographies'])
                                    for _ in range(hc['num'] - 1)], np.float64)

out = os.path.join(HERE, 'reference_drivers.npz')
np.savez_compressed(out, **G)
print('wrote %s (%d arrays, %d bytes)' % (out, len(G), os.path.getsize(out)))
