"""GPU: the LGHD baseline end to end -- PairPipeline(ClassicDetectors) against the restatement pipeline (tests/lghd_restatement.py
for the detector and the descriptors, the oracle's box_nms, a float64 brute-force matcher), the evaluation driver, and both
command lines with the fixture model directory tests/golden/lghd."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import lghd_restatement as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL_DIR = os.path.join(ROOT, 'tests', 'golden', 'lghd')
DEV = 'cuda'
H, W, DY, DX = 96, 120, 3, 5
PRED = {'nms': 4, 'detection_threshold': 0.015, 'topk': 0, 'reprojection_threshold': 3,
        'matching': {'method': 'bfmatcher', 'method_kwargs': {'crossCheck': True}, 'knn_matches': False}}


def _pair():
    """two overlapping 96 x 120 crops of one noise image, (3, 5) pixels apart"""
    big = R.noise_image(31, H + DY, W + DX)
    return np.ascontiguousarray(big[:H, :W]), np.ascontiguousarray(big[DY:, DX:])


def _model():
    from multipoint_amd.models import ClassicDetectors
    cfg = yaml.safe_load(open(os.path.join(MODEL_DIR, 'params.yaml')))['model']
    assert cfg['type'] == 'ClassicDetectors' and cfg['method'] == 'LGHD'
    return ClassicDetectors(cfg).to(DEV).eval()


def _restated_side(image, oracle):
    """(keypoints behind box_nms, raw descriptors from the float64 orientation maps, undecided-pixel mask [4][H][W])"""
    u8 = R.quantize(image)
    bank = R.filter_bank(H, W)
    m64 = R.responses(u8, bank)
    err32 = np.abs(R.responses(u8, bank, single=True) - m64).max()
    undecided = R.top_two_gap(m64) < 16 * err32
    prob = np.zeros((H, W), np.float32)
    valid = R.valid_keypoints(R.fast_keypoints(u8), H, W)
    prob[valid[:, 0], valid[:, 1]] = 1.0
    kept = oracle.box_nms(prob[None, None], PRED['nms'], PRED['detection_threshold'])[0, 0]
    kp = oracle.keypoints_from_map(kept, PRED['detection_threshold'])
    return kp, R.patch_descriptors(R.orientation_maps(m64), kp), undecided


def test_pair_pipeline_agrees_with_the_restatement(oracle):
    from multipoint_amd.pipeline import PairPipeline
    optical, thermal = _pair()
    pipe = PairPipeline(_model(), PRED)
    res = pipe(torch.from_numpy(optical)[None, None].to(DEV), torch.from_numpy(thermal)[None, None].to(DEV))
    assert pipe.tie_redone == 0
    got = res.to_host()[0]
    for side, image in (('optical', optical), ('thermal', thermal)):
        kp, raw, undecided = _restated_side(image, oracle)
        assert len(kp) >= 30
        assert np.array_equal(got['kp_' + side], kp)                                  # lists: exact, row-major
        desc = got['desc_' + side].astype(np.float64)
        assert desc.shape == (len(kp), 384)
        # a patch without a pixel the float64 arg-max leaves undecided (test_gpu_lghd.py, rule 3) has the restatement's row
        clean = np.array([not undecided[:, y - 20:y + 20, x - 20:x + 20].any() for y, x in kp])
        print(side, '%d keypoints, %d with a fully decided patch' % (len(kp), clean.sum()))
        assert clean.mean() >= 0.5
        assert np.abs(desc[clean] - R.unit_rows(raw)[clean]).max() <= 1e-6
        assert np.abs(np.linalg.norm(desc, axis=1) - 1).max() <= 1e-6
    # mutual matches: float64 brute force on the rows the pipeline returned (they are the restatement's wherever the patch is
    # decided, see above), compared where both arg-mins are decided by more than 1e-5 (rule 5)
    a, b = got['desc_optical'].astype(np.float64), got['desc_thermal'].astype(np.float64)
    d = np.sqrt(2.0 - 2.0 * np.clip(a @ b.T, -1.0, 1.0))
    def decided(m):
        s = np.sort(m, axis=1)
        return s[:, 1] - s[:, 0] > 1e-5
    best, best_t = d.argmin(1), d.argmin(0)
    ok = decided(d) & decided(d.T)[best]
    want = np.where(best_t[best] == np.arange(len(a)), best, -1)
    have = np.full(len(a), -1)
    have[got['match_query']] = got['match_train']
    print('mutual matches: %d, %d of %d rows compared' % ((have >= 0).sum(), ok.sum(), len(a)))
    assert ok.mean() >= 0.9 and np.array_equal(have[ok], want[ok])
    hit = have >= 0
    # distances against float64 on the returned rows.  The crops overlap, so true matches have IDENTICAL rows: d = 0, where
    # d = sqrt(2 - 2 t) turns the one rounding of t = 1 - 2^-24 into 4.9e-4.  As in tests/test_gpu_match_modes.py the squared
    # distance is held to 2 tau, tau = 2 (D + 2) 2^-24, and d itself to 1e-6 where d >= 0.5 (tests/test_gpu_match_384.py)
    u64 = 2.0 - 2.0 * np.clip((got['desc_optical'].astype(np.float64)[got['match_query']] *
                               got['desc_thermal'].astype(np.float64)[got['match_train']]).sum(1), -1, 1)
    assert np.abs(got['match_dist'].astype(np.float64) ** 2 - u64).max() <= 2 * 2.0 * 386 * 2.0 ** -24
    far = u64 >= 0.25
    assert np.abs(got['match_dist'] - np.sqrt(u64))[far].max(initial=0) <= 1e-6
    # the crops overlap: most mutual matches are the true correspondence (y, x) -> (y - 3, x - 5)
    shift = got['kp_optical'][got['match_query']] - got['kp_thermal'][got['match_train']]
    assert hit.sum() >= 20 and (np.all(shift == [DY, DX], axis=1)).mean() >= 0.5


def test_descriptor_metrics_driver():
    from multipoint_amd.utils import compute_descriptor_metrics
    optical, thermal = _pair()
    ones = torch.ones((1, 1, H, W), dtype=torch.bool)
    shift = torch.tensor([[[1.0, 0.0, -DX], [0.0, 1.0, -DY], [0.0, 0.0, 1.0]]])            # the thermal crop begins (3, 5) further in
    batch = {'optical': {'image': torch.from_numpy(optical)[None, None], 'valid_mask': ones, 'homography': torch.eye(3)[None]},
             'thermal': {'image': torch.from_numpy(thermal)[None, None], 'valid_mask': ones.clone(), 'homography': shift}}
    out = compute_descriptor_metrics(_model(), [batch], torch.device(DEV), dict(PRED, topk=1000), 4, 4)
    for k in ('nn_map', 'm_score', 'h_correctness'):
        print(k, out[k])
        assert out[k] is not None and np.isfinite(out[k])


def test_scope_fences():
    from multipoint_amd.models import ClassicDetectors
    with pytest.raises(NotImplementedError):
        ClassicDetectors({'method': 'SIFT'})
    with pytest.raises(ValueError):
        _model()({'image': torch.zeros((1, 1, 56, 70), device=DEV)})


def _config(tmp_path):
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'config_image_pair_dataset_prediction.yaml')))
    cfg['dataset'].update({'num_samples': 2, 'height': 96, 'width': 120})
    cfg['dataset']['augmentation']['homographic']['enable'] = False
    cfg['prediction'].update({'batchsize': 2, 'num_worker': 0, 'topk': 300})       # (the RANSAC launch holds 3200 keypoints a list)
    path = tmp_path / 'cfg.yaml'
    path.write_text(yaml.safe_dump(cfg))
    return str(path)


def test_command_lines_run_the_baseline(tmp_path):
    cfg = _config(tmp_path)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'predict_align_image_pair.py'), '-y', cfg, '-m', MODEL_DIR, '-v', 'none',
                          '-i', '0', '-p'], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    for line in ('Optical keypoints:', 'Thermal keypoints:', 'Matches (bfmatcher):', 'Estimated Homography:'):
        assert line in out.stdout
    assert int(out.stdout.split('Optical keypoints:')[1].split()[0]) > 20
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'predict_keypoints.py'), '-y', cfg, '-m', MODEL_DIR, '-v', 'none', '-b'],
                         capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert 'optical keypoints per image:' in out.stdout
    # -e writes its results next to the model: run it on a copy of the fixture directory
    copy = tmp_path / 'lghd'
    shutil.copytree(MODEL_DIR, copy)
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'predict_align_image_pair.py'), '-y', cfg, '-m', str(copy), '-v', 'none',
                          '-i', '1', '-e', '-p', '--refine'], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    for line in ('NN-mAP:', 'M-Score:', 'Homography Correctness:', 'Refinement:'):
        assert line in out.stdout
    assert os.listdir(copy / 'descriptor_evaluation')
