"""GPU (MI355X): the two command lines with --transform similarity, end to end on the fixtures of the existing CLI tests
(tests/test_gpu_initial_transform_cli.py's LGHD pairs of two frame sizes, tests/test_gpu_guided.py's synthetic-shapes
configuration)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import yaml

import test_gpu_initial_transform_cli as ITC                # (its pairs, configuration and runner)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_estimate_initial_transform_with_a_similarity(tmp_path):
    """The thermal frames are crops of the optical ones at (dy, dx) = (5, 9): optical -> thermal is the translation (-9, -5), a
    similarity of angle 0 and scale 1.  At the fixture's 0.5 px threshold the consensus set holds exact matches only, so the
    least-squares similarity over it is that translation to rounding."""
    pairs = tmp_path / 'preprocessed'
    os.makedirs(pairs)
    ITC._write_pairs(str(pairs))
    out = ITC._run(ITC._config(tmp_path), pairs, '--transform', 'similarity')
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout[-1200:])
    assert 'Estimated similarity transform (optical -> thermal):' in out.stdout and 'Similarity: angle' in out.stdout
    Tm = np.array(yaml.safe_load((pairs / 'initial_transform.yaml').read_text())['perspective'], np.float64)
    assert Tm.shape == (3, 3) and np.abs(Tm - [[1, 0, ITC.DX], [0, 1, ITC.DY], [0, 0, 1]]).max() <= 1e-6
    assert np.abs(Tm[2] - [0, 0, 1]).max() <= 1e-12 and abs(Tm[0, 0] - Tm[1, 1]) <= 1e-12 and abs(Tm[0, 1] + Tm[1, 0]) <= 1e-12
    report = json.load(open(pairs / 'initial_transform_report.json'))
    assert report['transform'] == 'similarity' and report['pairs_used'] == 6
    sim = report['similarity']
    assert abs(sim['angle']) <= 1e-6 and abs(sim['scale'] - 1.0) <= 1e-6 and abs(sim['dx'] + ITC.DX) <= 1e-6 and abs(sim['dy'] + ITC.DY) <= 1e-6
    assert 8 <= report['inliers'] == sum(report['inliers_per_pair'].values()) <= report['matches_pooled']
    assert 0.0 <= report['cost_after_polish'] <= report['cost_before_polish']


def test_predict_align_image_pair_with_a_similarity(tmp_path):
    d = tmp_path / 'multipoint'
    d.mkdir()
    with open(os.path.join(ROOT, 'model_weights', 'multipoint', 'params.yaml')) as f:
        (d / 'params.yaml').write_text(f.read())
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'config_image_pair_dataset_prediction.yaml')))
    cfg['dataset'].update({'num_samples': 2, 'height': 120, 'width': 160})
    cfg['dataset']['augmentation']['homographic']['enable'] = False
    cfg['prediction'].update({'topk': 300, 'batchsize': 1, 'num_worker': 0})
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    cfg['prediction']['transform_model'] = 'similarity'
    (tmp_path / 'cfg_similarity.yaml').write_text(yaml.safe_dump(cfg))
    script = [sys.executable, os.path.join(ROOT, 'predict_align_image_pair.py'), '-m', str(d), '-v', 'none']
    # two fresh child processes, side by side: the flag, and the configuration key without the flag
    runs = [subprocess.Popen(script + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
            for extra in (['-y', str(tmp_path / 'cfg.yaml'), '--refine', '--transform', 'similarity'],
                          ['-y', str(tmp_path / 'cfg_similarity.yaml'), '--refine'])]
    (flag, ferr), (key, kerr) = [r.communicate() for r in runs]
    assert runs[0].returncode == 0, ferr[-2000:]
    assert runs[1].returncode == 0, kerr[-2000:]

    def stable(text):                                   # (from the keypoint counts on: no timing lines behind them)
        lines = [l for l in text.split('\n') if not re.search(r'took:|Box nms:', l)]
        return lines[[i for i, l in enumerate(lines) if l.startswith('Optical keypoints:')][0]:]
    assert stable(flag) == stable(key)
    print('\n'.join(l for l in stable(flag) if re.search(r'imilarity|inliers|Refine', l)))
    assert 'Estimated similarity transform:' in flag and 'Estimated Homography:' not in flag
    assert len([l for l in flag.split('\n') if l.startswith('RANSAC inliers:')]) == 1
    line = [l for l in flag.split('\n') if l.startswith('Refinement:')]
    assert len(line) == 1
    assert re.match(r'Refinement: \d+ inliers of \d+ matches -> (\d+ inliers of \d+ matches|no refined estimate|unchanged)', line[0])
    # the printed estimate is a similarity with last row (0, 0, 1), or the identity the script falls back to without a model
    at = flag.split('\n').index('Estimated similarity transform:')
    rows = [[float(v) for v in re.findall(r'-?\d+\.?\d*(?:e[-+]?\d+)?', l)] for l in flag.split('\n')[at + 1:at + 4]]
    H = np.array(rows)
    assert H.shape == (3, 3) and H[2].tolist() == [0.0, 0.0, 1.0]
    assert abs(H[0, 0] - H[1, 1]) <= 1e-6 * max(1.0, abs(H[0, 0])) and abs(H[0, 1] + H[1, 0]) <= 1e-6 * max(1.0, abs(H[0, 1]))
