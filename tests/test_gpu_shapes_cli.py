"""The SyntheticShapes command-line tools end to end, as child processes: show_synthetic_images.py writes its PNGs and
compute_validation_loss.py validates a checkpoint on generated samples."""
import os
import subprocess
import sys

import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shapes_cases as C  # noqa: E402


def dataset_config():
    cfg = C.case_config('a_draw_lines')
    cfg.update(type='SyntheticShapes', length=4, primitives=['draw_lines', 'draw_polygon', 'draw_star', 'draw_ellipses'])
    cfg['generation']['draw_multiple_polygons']['kernel_boundaries'] = [3, 9]      # yaml knows no tuples
    cfg['augmentation'] = {'photometric': {'enable': False},
                           'homographic': {'enable': True, 'params': {}, 'border_reflect': True, 'valid_border_margin': 0,
                                           'mask_border': True}}
    return cfg


def run(script, args):
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=ROOT, capture_output=True, text=True,
                          timeout=600)


def test_show_synthetic_images(tmp_path):
    from PIL import Image
    cfg_path = tmp_path / 'config.yaml'
    with open(cfg_path, 'w') as f:
        yaml.safe_dump({'dataset': dataset_config()}, f)
    out = tmp_path / 'png'
    r = run('show_synthetic_images.py', ['-y', str(cfg_path), '-n', '2', '-s', '5', '-o', str(out)])
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(out)) == ['0_masked.png', '0_raw.png', '1_masked.png', '1_raw.png']
    for name in os.listdir(out):
        with Image.open(out / name) as im:
            assert im.size == (64, 48) and im.mode == 'RGB'


def test_validation_loss_on_synthetic_shapes(tmp_path):
    from oracle import mp_oracle as O
    mdir = tmp_path / 'model'
    mdir.mkdir()
    torch.save(O.make_weights(1, dict(O.SHIPPED_MODEL_CONFIG)), mdir / 'e1.model')
    config = {'dataset': dataset_config(), 'model': dict(O.SHIPPED_MODEL_CONFIG, type='MultiPoint'),
              'loss': {'type': 'SuperPointLoss', 'detector_loss': True, 'descriptor_loss': False},
              'training': {'batchsize': 2, 'num_worker': 4}}
    cfg_path = tmp_path / 'config.yaml'
    with open(cfg_path, 'w') as f:
        yaml.safe_dump(config, f)
    r = run('compute_validation_loss.py', ['-y', str(cfg_path), '-m', str(mdir), '-s', '3'])
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith('e1: loss')][0]
    loss = float(line.split()[2])
    assert loss == loss and abs(loss) != float('inf') and loss > 0
