"""GPU: the RIFT baseline end to end -- contrast inversion through ClassicDetectors, the planted optical / thermal pairs of
tests/rift_cases.py through PairPipeline and utils.find_transform against the float64 restatement's own chain (whose counts
tests/test_rift_host.py regenerates), and the command line with the fixture model directory tests/golden/rift."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import lghd_restatement as L
import rift_cases as C
import rift_restatement as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_DIR = os.path.join(ROOT, 'tests', 'golden', 'rift')
DEV = 'cuda'
PRED = {'nms': 0, 'detection_threshold': 0.015, 'topk': 0, 'reprojection_threshold': 3,
        'matching': {'method': 'bfmatcher', 'method_kwargs': {'crossCheck': True}, 'knn_matches': False}}


def _model(**keys):
    from multipoint_amd.models import ClassicDetectors
    cfg = yaml.safe_load(open(os.path.join(MODEL_DIR, 'params.yaml')))['model']
    assert cfg['type'] == 'ClassicDetectors' and cfg['method'] == 'RIFT'
    cfg.update(keys)
    return ClassicDetectors(cfg).to(DEV).eval()


def test_contrast_inversion():
    """a 96 x 128 smooth frame and its negative: the maximum index maps agree outside the ambiguous pixels of rule 3, and the
    keypoint lists at patch 48 agree except at pixels where the two u8m differ (the 16 pixels of FAST's circle and the centre)"""
    u8 = C.map_frame('smooth_96x128')
    image = torch.from_numpy(np.stack([u8, 255 - u8]).astype(np.float32) / np.float32(255.0))[:, None].to(DEV)
    assert np.array_equal(L.quantize(image[:, 0].cpu().numpy()), np.stack([u8, 255 - u8]))
    model = _model(patch_size=48, fast_threshold=13)
    out = model({'image': image})
    assert set(out) == {'prob', 'mim', 'pc_max', 'pc_min'}
    mim, prob, M = out['mim'].cpu().numpy(), out['prob'].cpu().numpy()[:, 0], out['pc_max'].cpu().numpy()
    amb = C.ambiguous('smooth_96x128')
    print('MIM: %d pixels differ, %d ambiguous' % ((mim[0] != mim[1]).sum(), amb.sum()))
    assert np.array_equal(mim[0][~amb], mim[1][~amb])
    a, b = R.moment_u8(M[0]).astype(np.int32), R.moment_u8(M[1]).astype(np.int32)
    differs = a != b
    touched = np.zeros_like(differs)                   # a pixel whose score or whose neighbours' scores read a differing u8m value
    for y, x in np.argwhere(differs):
        touched[max(y - 4, 0):y + 5, max(x - 4, 0):x + 5] = True
    kp0, kp1 = prob[0] > 0, prob[1] > 0
    print('u8m: %d pixels differ; keypoints %d / %d, %d differ, %d of them away from a differing pixel'
          % (differs.sum(), kp0.sum(), kp1.sum(), (kp0 != kp1).sum(), ((kp0 != kp1) & ~touched).sum()))
    assert kp0.sum() >= 50
    assert np.array_equal(kp0[~touched], kp1[~touched]) and np.array_equal(prob[0][~touched], prob[1][~touched])
    # the comparison must not be vacuous.  The two M differ by float32 rounding (about 1e-7 on a range of 0.26), so
    # 255 Mn moves by about 1e-4 and crosses an integer at about one pixel in 10^4; each such pixel touches 81: well under a quarter
    assert touched.mean() <= 0.25


def test_forward_outputs_and_dense_map():
    """B = 1 returns the dense map of raw counts at the keypoints, as LGHD does; describe() routes on `mim`"""
    u8 = C.map_frame('smooth_96x128')
    image = torch.from_numpy(u8.astype(np.float32) / np.float32(255.0))[None, None].to(DEV)
    model = _model(patch_size=48, fast_threshold=13)
    out = model({'image': image})
    assert set(out) == {'prob', 'mim', 'pc_max', 'pc_min', 'desc'}
    assert out['desc'].shape == (1, 256, 96, 128) and out['pc_max'].shape == out['pc_min'].shape == out['mim'].shape == (1, 96, 128)
    kp = torch.nonzero(out['prob'][0, 0] > 0).to(torch.int32)
    n = kp.shape[0]
    rows = model.describe(out, kp[None], torch.tensor([n], dtype=torch.int32))
    assert rows.shape == (1, n, 256)
    dense = out['desc'][0][:, kp[:, 0].long(), kp[:, 1].long()].t()
    want = R.descriptors(out['mim'][0].cpu().numpy(), kp.cpu().numpy(), 48)
    assert np.array_equal(dense.cpu().numpy()[:, :216], want) and not dense[:, 216:].any()
    diff = np.abs(rows[0].cpu().numpy()[:, :216] - L.unit_rows(want)).max(1)
    print('%d keypoints; unit rows off by more than 1e-6: %s' % (n, np.nonzero(diff > 1e-6)[0].tolist()))
    assert diff.max() <= 1e-6
    assert (out['desc'].abs().sum(1)[0] > 0).sum() == n


@pytest.mark.parametrize('i', range(3))
def test_planted_pair(i):
    """Matches within 3 px of the planted map: at least 0.9 x the float64 restatement's count; find_transform('similarity') on the
    pipeline's matches within 1 px of the planted map at the four corners."""
    from multipoint_amd.pipeline import PairPipeline
    from multipoint_amd.utils import find_transform
    optical, thermal = C.planted_pair(i)
    # (1024 list slots: a frame has about 250 keypoints, and the estimator's launch holds at most 3200 slots a list)
    pipe = PairPipeline(_model(patch_size=C.PAIR_PATCH, fast_threshold=C.PAIR_FAST_THRESHOLD), PRED, capacity=1024)
    res = pipe(torch.from_numpy(optical)[None, None].to(DEV), torch.from_numpy(thermal)[None, None].to(DEV))
    got = res.to_host()[0]
    assert got['desc_optical'].shape[1] == 256 and not got['desc_optical'][:, 216:].any()
    err = C.planted_error(i, got['kp_optical'][got['match_query']], got['kp_thermal'][got['match_train']])
    correct = int((err <= 3.0).sum())
    Hm, mask, nin = find_transform(res, 'similarity', reproj_threshold=3.0, max_iters=2000, seed=0)
    T = Hm[0].cpu().numpy()
    corner = C.corner_error(i, T) if T.any() else float('inf')
    print('pair %d: %d / %d keypoints (restatement %d / %d), %d mutual matches (restatement %d), %d within 3 px (restatement %d), '
          '%d inliers, corner error %.3f px' % (i, len(got['kp_optical']), len(got['kp_thermal']), len(C.restated_pair(i)[0][0]),
                                                len(C.restated_pair(i)[1][0]), len(err), C.RESTATED_MUTUAL[i], correct,
                                                C.RESTATED_CORRECT[i], int(nin[0]), corner))
    assert correct >= 0.9 * C.RESTATED_CORRECT[i]
    assert corner <= 1.0


def test_configuration_keys():
    from multipoint_amd.models import ClassicDetectors
    assert ClassicDetectors.default_config == {'method': 'SURF', 'prob_smoothing': False, 'smoothing_kernel_size': 5,
                                               'min_keypoints': 100, 'image_H': 512, 'image_W': 640}
    model = ClassicDetectors({'method': 'RIFT'})
    assert (model.patch_size, model.fast_threshold) == (96, 13)
    assert set(model.config) == set(ClassicDetectors.default_config)             # the two keys are popped, as `implementation` is
    for bad in ({'patch_size': 40}, {'patch_size': '48'}, {'patch_size': 48.0}, {'patch_size': 0}, {'patch_size': 168},
                {'fast_threshold': 0}, {'fast_threshold': 256}, {'fast_threshold': 6.5}, {'fast_threshold': None}):
        with pytest.raises(ValueError):
            ClassicDetectors(dict({'method': 'RIFT'}, **bad))
    with pytest.raises(ValueError):
        ClassicDetectors({'method': 'LGHD', 'patch_size': 48})                    # the keys belong to RIFT
    with pytest.raises(ValueError):
        ClassicDetectors({'method': 'RIFTS'})


def test_command_line_runs_the_baseline(tmp_path):
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'config_image_pair_dataset_prediction.yaml')))
    cfg['dataset'].update({'num_samples': 2, 'height': 192, 'width': 240})      # holds the fixture's 96-pixel patches
    cfg['dataset']['augmentation']['homographic']['enable'] = False
    cfg['prediction'].update({'batchsize': 2, 'num_worker': 0, 'topk': 300})
    path = tmp_path / 'cfg.yaml'
    path.write_text(yaml.safe_dump(cfg))
    copy = tmp_path / 'rift'                  # -e writes its results next to the model: run it on a copy of the fixture directory
    shutil.copytree(MODEL_DIR, copy)
    npz = tmp_path / 'pair.npz'
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'predict_align_image_pair.py'), '-y', str(path), '-m', str(copy), '-v', 'none',
                          '-i', '1', '-e', '-p', '--save-npz', str(npz)], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout[-1500:])
    for line in ('Optical keypoints:', 'Thermal keypoints:', 'NN-mAP:', 'M-Score:', 'Homography Correctness:'):
        assert line in out.stdout
    saved = np.load(str(npz))
    assert saved['desc_optical'].shape[1] == 256 and saved['desc_thermal'].shape[1] == 256
    assert len(saved['kp_optical']) > 10 and not saved['desc_optical'][:, 216:].any()
