"""GPU: prepare_images.py end to end -- raw pairs in, the reference's three files per pair out, equal to prepare_frames -- then
align_images.py on its output directory unchanged, the ImageFilePairs dataset on it, and predict_keypoints.py through that
dataset type."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

import frames_restatement as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTICAL, THERMAL, PAIRS = (90, 120), (64, 80), 3


def _u16(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _run(script, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + [str(a) for a in args], capture_output=True, text=True,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


@pytest.fixture(scope='module')
def prepared(tmp_path_factory):
    """three seeded raw pairs, a calibration file and the reference's config, ROS keys included, run through the CLI once"""
    raw = tmp_path_factory.mktemp('raw')
    out = tmp_path_factory.mktemp('out')
    optical = [R.smooth_bgr8(30 + i, *OPTICAL) for i in range(PAIRS)]
    thermal = [R.thermal_u16(40 + i, *THERMAL, base=20000 + 3000 * i) for i in range(PAIRS)]
    # the thermal camera looks at the optical pattern's grey value, upside down, so that the pair has something in common
    for i in range(PAIRS):
        grey = R.resize_bgr8(optical[i], THERMAL).astype(np.float64).mean(-1)[::-1, ::-1]
        thermal[i] = np.clip(thermal[i].astype(np.float64) * 0.2 + 16000 + grey * 40, 0, 65535).astype(np.uint16)
    names = ['0', '1', '10']
    for n, o, t in zip(names, optical, thermal):
        Image.fromarray(np.ascontiguousarray(o[:, :, ::-1])).save(raw / (n + '_optical_raw.png'))
        Image.fromarray(t).save(raw / (n + '_thermal_raw.png'))
    calibration = R.calibration_of([('optical', R.DISTORTIONS[1]), ('thermal', R.DISTORTIONS[2])], OPTICAL, THERMAL)
    (raw / 'calibration.yaml').write_text(yaml.safe_dump(calibration))
    params = {'undistort_images': True, 'compensate_exposure_time': True, 'check_pose': False, 'verbose': True,
              'save_preprocessed_images': True, 'rosbag/topic_optical_images': '/image_republisher/rgb/image_raw',
              'rosbag/max_dt': 0.025, 'image/undistort_alpha': 0.0, 'image/calibration_params': 'calibration.yaml',
              'image/optical/downscale': True, 'image/thermal/rotate': True, 'image/thermal/rescale_outlier_rejection': True,
              'image/show_raw/dt': 20}
    (raw / 'config.yaml').write_text(yaml.safe_dump(params))
    stdout = _run('prepare_images.py', '-y', raw / 'config.yaml', '-i', raw, '-o', out, '--batch', 2)
    return {'raw': raw, 'out': out, 'dir': out / 'preprocessed', 'names': names, 'optical': optical, 'thermal': thermal,
            'params': params, 'calibration': calibration, 'stdout': stdout}


def test_cli_writes_what_prepare_frames_returns(prepared):
    from multipoint_amd.utils import frames
    p = prepared
    assert sorted(os.listdir(p['dir'])) == sorted(n + s for n in p['names'] for s in ('_optical.png', '_thermal_raw.png', '_thermal.png'))
    assert 'Number of pairs: 3' in p['stdout']
    ignored = [l for l in p['stdout'].split('\n') if l.startswith('Accepted and ignored')]
    assert len(ignored) == 1 and all(k in ignored[0] for k in ('rosbag/max_dt', 'check_pose', 'compensate_exposure_time',
                                                               'image/show_raw/dt'))
    opt, raw, rescaled, saved = frames.prepare_frames(np.stack(p['optical']), np.stack(p['thermal']), p['params'],
                                                      p['calibration'], return_saved=True)
    opt, raw, saved = opt.cpu().numpy(), _u16(raw), _u16(saved)
    assert opt.shape == (PAIRS, THERMAL[0], int(OPTICAL[1] * (float(THERMAL[0]) / OPTICAL[0])), 3)
    for k, n in enumerate(p['names']):
        with Image.open(p['dir'] / (n + '_optical.png')) as im:
            assert im.mode == 'RGB' and np.array_equal(np.array(im)[:, :, ::-1], opt[k])
        for suffix, want in (('_thermal_raw.png', raw), ('_thermal.png', saved)):
            with Image.open(p['dir'] / (n + suffix)) as im:
                got = np.array(im)
            assert got.dtype == np.uint16 and np.array_equal(got, want[k]), (n, suffix)
        # and the whole chain is the restatement's
        want = R.prepare_frames(p['optical'][k], p['thermal'][k], p['params'], p['calibration'])
        assert np.array_equal(opt[k], want[0]) and np.array_equal(raw[k], want[1])
        assert np.array_equal(saved[k], R.saved_u16(want[2]))


def test_align_images_runs_on_the_output(prepared, tmp_path):
    p = prepared
    scale = float(OPTICAL[0]) / THERMAL[0]
    ow = int(OPTICAL[1] * (float(THERMAL[0]) / OPTICAL[0]))
    init = [[1.0, 0.0, (ow - THERMAL[1]) / 2.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    assert scale > 1
    (p['dir'] / 'initial_transform.yaml').write_text(yaml.safe_dump({'perspective': init}))
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'config_align_images.yaml')))
    cfg.update({'alignment/bin_sizes': [16, 32], 'alignment/n_pyramid_levels': 1})
    (tmp_path / 'align.yaml').write_text(yaml.safe_dump(cfg))
    stdout = _run('align_images.py', '-y', tmp_path / 'align.yaml', '-i', p['dir'], '-o', tmp_path / 'aligned')
    assert 'Number of pairs: 3' in stdout and 'Alignment method counters:' in stdout
    assert os.path.isfile(tmp_path / 'aligned' / 'transforms.json') and os.path.isfile(tmp_path / 'aligned' / 'failed.log')


def test_image_file_pairs_schema(prepared, tmp_path):
    import multipoint_amd.datasets as datasets
    p = prepared
    # the thermal and optical files of `preprocessed` differ in width: the dataset reads registered pairs, so crop the optical
    # frames onto the thermal ones the way align_images.py's `aligned/best` holds them
    pairs = _registered(p, tmp_path / 'pairs')
    ds = datasets.ImageFilePairs({'directory': str(pairs), 'single_image': False, 'height': 48, 'width': 64})
    assert len(ds) == PAIRS and ds.returns_pair() and [ds.get_name(i) for i in range(PAIRS)] == p['names']
    assert datasets.loader_num_workers(ds, 4) == 0
    sample = ds[2]
    assert set(sample) == {'optical', 'thermal', 'name'} and sample['name'] == '10'
    for side, is_optical in (('optical', True), ('thermal', False)):
        e = sample[side]
        assert set(e) == {'image', 'valid_mask', 'is_optical'}
        assert e['image'].shape == (1, 48, 64) and e['image'].dtype == torch.float32
        assert e['valid_mask'].shape == (1, 48, 64) and e['valid_mask'].dtype == torch.bool and bool(e['valid_mask'].all())
        assert bool(e['is_optical'][0]) == is_optical
        assert 0.0 <= float(e['image'].min()) and float(e['image'].max()) <= 1.0
    # the values: v / 65535 of the 16-bit file, the reference's grey of the colour file; the crop drawn as ImagePairDataset does
    import random
    import pyramid_restatement as P
    random.seed(3)
    full = datasets.ImageFilePairs({'directory': str(pairs), 'single_image': False})[1]
    with Image.open(pairs / '1_thermal.png') as im:
        th = np.array(im)
    with Image.open(pairs / '1_optical.png') as im:
        bgr = np.ascontiguousarray(np.array(im.convert('RGB'))[:, :, ::-1])
    assert np.array_equal(full['thermal']['image'][0].numpy().view(np.uint32), P.frames_to_float(th).view(np.uint32))
    assert np.array_equal(full['optical']['image'][0].numpy().view(np.uint32), P.frames_to_float(bgr[None])[0].view(np.uint32))
    random.seed(3)
    i_h, i_w = random.randint(0, THERMAL[0] - 48), random.randint(0, THERMAL[1] - 64)
    random.seed(3)
    crop = ds[1]
    assert torch.equal(crop['thermal']['image'], full['thermal']['image'][:, i_h:i_h + 48, i_w:i_w + 64])
    single = datasets.ImageFilePairs({'directory': str(pairs)})[0]
    assert set(single) == {'image', 'valid_mask', 'is_optical', 'name'}
    with pytest.raises(ValueError):
        datasets.ImageFilePairs({})


def _registered(p, target):
    os.makedirs(target, exist_ok=True)
    for n in p['names']:
        with Image.open(p['dir'] / (n + '_optical.png')) as im:
            o = np.array(im)
        off = (o.shape[1] - THERMAL[1]) // 2
        Image.fromarray(np.ascontiguousarray(o[:, off:off + THERMAL[1]])).save(target / (n + '_optical.png'))
        with Image.open(p['dir'] / (n + '_thermal.png')) as im:
            Image.fromarray(np.array(im)).save(target / (n + '_thermal.png'))
    return target


def test_predict_keypoints_on_image_file_pairs(prepared, tmp_path):
    pairs = _registered(prepared, tmp_path / 'pairs')
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'config_image_pair_dataset_prediction.yaml')))
    cfg['dataset'] = {'type': 'ImageFilePairs', 'directory': str(pairs), 'single_image': False, 'return_name': True}
    cfg['prediction'].update({'batchsize': 1, 'num_worker': 0})
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    stdout = _run('predict_keypoints.py', '-y', tmp_path / 'cfg.yaml', '-m', os.path.join(ROOT, 'model_weights', 'multipoint'),
                  '-v', 'none', '-i', 1)
    assert 'contains 3 image pairs' in stdout
    assert 'optical keypoints per image:' in stdout and 'thermal keypoints per image:' in stdout
