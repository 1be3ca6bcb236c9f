"""GPU (MI355X): estimate_initial_transform.py end to end with the weight-free LGHD baseline on frames of two sizes, and
PairPipeline.run_two_sized, which it is built on."""
import json
import os
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
HO, WO, HT, WT, DY, DX = 108, 135, 96, 120, 5, 9          # both sizes 5-smooth, as the LGHD filter bank needs
SEEDS = range(100, 106)


def _levels(seed):
    return np.rint(R.noise_image(seed, HO, WO) * 255.0).astype(np.int64)          # the grey levels 0..255 of the noise image


def _write_pairs(directory):
    """6 pairs: the optical frame is a 108 x 135 noise image as an 8-bit file, the thermal frame its 96 x 120 crop at
    (dy, dx) = (5, 9) as a 16-bit file (level v as 257 v, so v / 255 on both paths)."""
    from PIL import Image
    for i, seed in enumerate(SEEDS):
        v = _levels(seed)
        Image.fromarray(v.astype(np.uint8)).save(os.path.join(directory, '%d_optical.png' % i))
        Image.fromarray((v[DY:DY + HT, DX:DX + WT] * 257).astype(np.uint16)).save(os.path.join(directory, '%d_thermal.png' % i))


def _config(tmp_path):
    """The shipped prediction config with reprojection_threshold 0.5.  Keypoints are integers, so a true match has error 0
    under the true translation and any other match at least 1: at 0.5 px the consensus set of the true model holds true
    matches only, and its refit and polish give the translation to rounding.  (At the shipped 3 px it also takes in matches
    between NEIGHBOURING corners -- the box NMS keeps different neighbours near the two frames' different borders -- and the
    refit over them is a translation only to a few hundredths.)  Checked on the CPU with the restatement pipeline
    (tests/lghd_restatement.py, the oracle's box_nms, float64 mutual matching) for these seeds: 1243 pooled matches, 1154 of
    them true, and at 0.5 px oracle.ransac_homography's consensus set is exactly those 1154."""
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'config_image_pair_dataset_prediction.yaml')))
    cfg['prediction'].update({'reprojection_threshold': 0.5})
    path = tmp_path / 'cfg.yaml'
    path.write_text(yaml.safe_dump(cfg))
    return str(path)


def _run(cfg, directory, *extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'estimate_initial_transform.py'), '-y', cfg, '-m', MODEL_DIR,
                           '-v', 'none', '-i', str(directory), '--batch', '4'] + list(extra), capture_output=True, text=True, cwd=ROOT)


def test_command_line_writes_the_translation(tmp_path, monkeypatch):
    pairs = tmp_path / 'preprocessed'
    os.makedirs(pairs)
    _write_pairs(str(pairs))
    cfg = _config(tmp_path)
    out = _run(cfg, pairs)
    assert out.returncode == 0, out.stderr[-2000:]
    written = (pairs / 'initial_transform.yaml').read_text()
    T = np.array(yaml.safe_load(written)['perspective'], np.float64)
    print(out.stdout[-1500:])
    assert T.shape == (3, 3) and np.abs(T - [[1, 0, DX], [0, 1, DY], [0, 0, 1]]).max() <= 1e-6     # thermal (x, y) -> optical (x + 9, y + 5)
    report = json.load(open(pairs / 'initial_transform_report.json'))
    per_pair = report['inliers_per_pair']
    assert report['pairs_read'] == report['pairs_used'] == 6 and sorted(per_pair) == [str(i) for i in range(6)]
    assert report['inliers'] == sum(per_pair.values()) and 8 <= report['inliers'] <= report['matches_pooled']
    assert report['pairs_with_4_inliers'] == sum(v >= 4 for v in per_pair.values()) >= 1
    assert 0.0 <= report['cost_after_polish'] <= report['cost_before_polish']
    # a second run without --force fails and leaves the file as it is
    again = _run(cfg, pairs)
    assert again.returncode != 0 and 'force' in again.stderr and (pairs / 'initial_transform.yaml').read_text() == written
    # align_images.py starts from the written file: its argument parsing and its yaml read, up to the first batch
    import align_images
    from multipoint_amd.utils import alignment

    class Reached(Exception):
        pass

    def stop(optical, thermal, t_init, params):
        assert t_init.shape == (3, 3) and np.abs(t_init - T).max() == 0
        raise Reached()
    monkeypatch.setattr(alignment, 'align_images_mutual_information', stop)
    with pytest.raises(Reached):
        align_images.main(['-y', os.path.join(ROOT, 'configs', 'config_align_images.yaml'), '-i', str(pairs), '-o', str(tmp_path / 'out')])


def test_run_two_sized_builds_interleaved_results():
    """Frames of two sizes: lists, descriptors and matches as two single-camera runs give them; H / W are the thermal frame's;
    equal shapes take the existing route."""
    from multipoint_amd.models import ClassicDetectors
    from multipoint_amd.pipeline import PairPipeline
    cfg = yaml.safe_load(open(os.path.join(MODEL_DIR, 'params.yaml')))['model']
    pred = {'nms': 4, 'detection_threshold': 0.015, 'topk': 0,
            'matching': {'method': 'bfmatcher', 'method_kwargs': {'crossCheck': True}, 'knn_matches': False}}
    pipe = PairPipeline(ClassicDetectors(cfg).to(DEV).eval(), pred)
    v = np.stack([_levels(s) for s in (100, 101)])
    optical = torch.from_numpy((v / 255.0).astype(np.float32))[:, None].to(DEV)
    thermal = optical[:, :, DY:DY + HT, DX:DX + WT].contiguous()
    res = pipe.run_two_sized(optical, thermal)
    assert (res.H, res.W) == (HT, WT) and res.num_pairs == 2 and res.kp_yx.shape[0] == 4 and res.match_mode == 'mutual'
    got = res.to_host()
    for p in range(2):
        # each camera alone, as a pair with itself, through the existing entry
        o = pipe(optical[p:p + 1], optical[p:p + 1]).to_host()[0]
        t = pipe(thermal[p:p + 1], thermal[p:p + 1]).to_host()[0]
        assert np.array_equal(got[p]['kp_optical'], o['kp_optical']) and np.array_equal(got[p]['kp_thermal'], t['kp_thermal'])
        assert np.array_equal(got[p]['desc_optical'], o['desc_optical']) and np.array_equal(got[p]['desc_thermal'], t['desc_thermal'])
        shift = got[p]['kp_optical'][got[p]['match_query']] - got[p]['kp_thermal'][got[p]['match_train']]
        assert len(shift) >= 50 and np.all(shift == [DY, DX], axis=1).mean() >= 0.8
    same = pipe.run_two_sized(thermal, thermal)
    ref = pipe(thermal, thermal)
    assert (same.H, same.W) == (HT, WT) and torch.equal(same.kp_count, ref.kp_count)
    for x, y in zip(same.to_host(), ref.to_host()):                        # (rows beyond a list's count are not defined)
        for key in ('kp_optical', 'kp_thermal', 'match_query', 'match_train'):
            assert np.array_equal(x[key], y[key])
