"""compute_validation_loss.py --photometric {host,device} on a tiny .npz dataset whose config enables the photometric
augmentation: host noise gives the loss of the same loop run from Python, device noise is reproducible for a seed."""
import json
import os
import random

import numpy as np
import pytest
import torch
import yaml

from test_gpu_validation_cli import _run, _setup
from test_photometric_host import TRAIN_PARAMS, TRAIN_PRIMS

pytestmark = pytest.mark.gpu


def _photometric_setup(tmp_path):
    config, cfg_path, mdir = _setup(tmp_path, photometric=True)
    config['dataset']['augmentation']['photometric'] = {'enable': True, 'primitives': TRAIN_PRIMS, 'params': TRAIN_PARAMS,
                                                        'random_order': True}
    with open(cfg_path, 'w') as f:
        yaml.safe_dump(config, f)
    return config, cfg_path, mdir


def _direct(config, mdir, version, seed, noise):
    """train.py's validation loop with the photometric block on and SuperPointLoss called directly."""
    import multipoint_amd.datasets as datasets
    import multipoint_amd.utils as utils
    from multipoint_amd.utils.losses import SuperPointLoss
    from predict_align_image_pair import load_network
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
    val = dict(config['dataset'], filename=config['training']['validation']['filename'],
               keypoints_filename=config['training']['validation']['keypoints'])
    val['augmentation'] = dict(val['augmentation'], photometric=dict(val['augmentation']['photometric'], noise=noise))
    dataset = datasets.ImagePairDataset(val)
    loader = torch.utils.data.DataLoader(dataset, batch_size=config['training']['batchsize'], shuffle=False)
    net = load_network(config, mdir, version, torch.device('cuda:0'), seed)
    net.set_force_return_logits(True)
    loss_fn = SuperPointLoss(config['loss'])
    total = 0.0
    with torch.no_grad():
        for data in loader:
            data = utils.data_to_device(data, torch.device('cuda:0'))
            loss, _ = loss_fn(net(data['optical']), data['optical'], net(data['thermal']), data['thermal'])
            total += float(loss)
    return total / len(loader)


def test_cli_photometric_host_matches_python_loop(tmp_path):
    config, cfg_path, mdir = _photometric_setup(tmp_path)
    out_json = str(tmp_path / 'val.json')
    r = _run(['-y', cfg_path, '-m', mdir, '-v', 'e1', '-s', '4', '--photometric', 'host', '--save-json', out_json])
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.load(open(out_json))['versions']['e1']['loss']
    assert got == pytest.approx(_direct(config, mdir, 'e1', 4, 'host'), rel=1e-6)
    # without the augmentation the loss differs
    r = _run(['-y', cfg_path, '-m', mdir, '-v', 'e1', '-s', '4', '--no-photometric', '--save-json', out_json])
    assert r.returncode == 0, r.stdout + r.stderr
    assert json.load(open(out_json))['versions']['e1']['loss'] != got


def test_cli_photometric_device_reproducible(tmp_path):
    _, cfg_path, mdir = _photometric_setup(tmp_path)
    losses = []
    for k in range(2):
        out_json = str(tmp_path / ('dev%d.json' % k))
        r = _run(['-y', cfg_path, '-m', mdir, '-v', 'e2', '-s', '9', '--photometric', 'device', '--save-json', out_json])
        assert r.returncode == 0, r.stdout + r.stderr
        losses.append(json.load(open(out_json))['versions']['e2']['loss'])
    assert losses[0] == losses[1] and np.isfinite(losses[0])


def test_cli_photometric_flag_conflict(tmp_path):
    _, cfg_path, mdir = _photometric_setup(tmp_path)
    r = _run(['-y', cfg_path, '-m', mdir, '--photometric', 'device', '--no-photometric'])
    assert r.returncode == 2 and 'not allowed with' in r.stderr
