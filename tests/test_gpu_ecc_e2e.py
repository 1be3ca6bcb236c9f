"""GPU: the ECC refinement through the public surfaces -- utils.alignment.align_images with the alignment/ecc/ keys,
align_images.py --method ecc / --ecc on pairs written as PNG files, predict_align_image_pair.py --ecc-refine."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import ecc_cases as C
import registration_cases as RC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
PARAMS = {'alignment/bin_sizes': [16, 32], 'alignment/normalized_mi': True, 'alignment/smoothing_sigma': 0,
          'alignment/check/both/max_diff_mi': 0.5, 'alignment/accept_init': True, 'alignment/ranking_method': 'sum',
          'alignment/model': 'similarity'}


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(a, b):
    """two align_images results bit for bit"""
    (Ta, ka, ca), (Tb, kb, cb) = a, b
    assert ka == kb and np.array_equal(Ta, Tb) and len(ca) == len(cb)
    for x, y in zip(ca, cb):
        assert sorted(x) == sorted(y)
        for k in x:
            assert np.array_equal(x[k], y[k]) if k == 'transform' else x[k] == y[k], k


def test_align_images_keys():
    from multipoint_amd.utils import alignment as A
    name = 'small_thermal_far'
    optical, thermal, _ = C.pair(name)
    o, t, T0 = gpu(optical), gpu(thermal), C.start(name, 'near')
    absent = A.align_images(o, t, T0, dict(PARAMS))
    off = A.align_images(o, t, T0, dict(PARAMS, **{'alignment/ecc/enable': False, 'alignment/ecc/model': 'affine'}))
    same(absent, off)
    assert not any(c['type'].startswith('ecc') for c in absent[2])
    stats = {}
    T, kind, cands = A.align_images(o, t, T0, dict(PARAMS, **{'alignment/ecc/enable': True}), stats=stats)
    ecc = [c for c in cands if c['type'].startswith('ecc')]
    assert [c['type'] for c in ecc] == ['ecc_gradient_similarity'] and stats['ecc_rounds'] % 8 == 0 and stats['rounds'] > 0
    assert sorted(ecc[0]['mi']) == [16, 32] and ecc[0]['converged'] and C.error(ecc[0]['transform'], name) <= C.SIMILARITY_CAP
    same((None, None, [c for c in cands if not c['type'].startswith('ecc')]), (None, None, absent[2]))     # the others: unchanged
    print('winner', kind, '%.3f px' % C.error(T, name), [(c['type'], round(C.error(c['transform'], name), 3)) for c in cands])
    # the candidate passes through the checks: a limit nothing meets rejects it, a failed refinement is no candidate
    _, _, none = A.align_images(o, t, T0, dict(PARAMS, **{'alignment/ecc/enable': True, 'alignment/run_optimization': False,
                                                         'alignment/check/both/max_diff_mi': 0.0}))
    assert [c['type'] for c in none] == ['init']
    _, _, failed = A.align_images(o, t, T0, dict(PARAMS, **{'alignment/ecc/enable': True, 'alignment/run_optimization': False,
                                                           'alignment/ecc/feature': 'intensity'}))
    assert [c['type'] for c in failed] == ['init']
    # its own keys: model, filter size, iteration limit; a batch
    Ts, kinds, cl = A.align_images(gpu(np.stack([optical, optical]))[:, None], gpu(np.stack([thermal, thermal]))[:, None], T0,
                                   dict(PARAMS, **{'alignment/ecc/enable': True, 'alignment/run_optimization': False,
                                                   'alignment/accept_init': False, 'alignment/ecc/model': 'affine',
                                                   'alignment/ecc/filter_size': 3, 'alignment/ecc/max_iterations': 30}))
    assert kinds == ['ecc_gradient_affine'] * 2 and np.array_equal(Ts[0], Ts[1]) and np.array_equal(Ts[0][2], [0.0, 0.0, 1.0])
    assert cl[0][0]['nit'] <= 30
    with pytest.raises(ValueError):
        A.align_images(o, t, T0, dict(PARAMS, **{'alignment/ecc/enable': True, 'alignment/ecc/model': 'projective'}))


def _write_pairs(directory, n):
    from PIL import Image
    optical, thermal, _ = RC.cli_pairs()
    os.makedirs(directory, exist_ok=True)
    for i in range(n):
        Image.fromarray(optical[i]).save(os.path.join(directory, '%03d_optical.png' % i))
        Image.fromarray(thermal[i]).save(os.path.join(directory, '%03d_thermal.png' % i))
    T_init = C.cli_start(6.0)
    with open(os.path.join(directory, 'initial_transform.yaml'), 'wt') as fh:
        yaml.safe_dump({'perspective': T_init.tolist()}, fh)
    return T_init


CLI_CFG = dict(PARAMS, alignment_method='mi', perspective=True, save_aligned_images=False, use_image_pyramid=True,
               use_smoothing_stage=False, **{'alignment/n_pyramid_levels': 1, 'alignment/filter_size': 5,
                                             'alignment/accept_init': False})


def test_align_images_cli_method_ecc(tmp_path):
    src, dst = tmp_path / 'in', tmp_path / 'out'
    T_init = _write_pairs(str(src), 6)
    assert abs(C.cli_error(T_init) - 6.0) < 1e-6
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(CLI_CFG))
    base = [sys.executable, os.path.join(ROOT, 'align_images.py'), '-i', str(src), '-o', str(dst)]
    # any other method still raises, from the yaml and before any work
    (tmp_path / 'bad.yaml').write_text(yaml.safe_dump(dict(CLI_CFG, alignment_method='ncc')))
    bad = subprocess.run(base + ['-y', str(tmp_path / 'bad.yaml')], capture_output=True, text=True, cwd=ROOT)
    assert bad.returncode != 0 and 'Unkown alignment method: ncc' in bad.stderr and not dst.exists()
    r = subprocess.run(base + ['-y', str(tmp_path / 'cfg.yaml'), '--method', 'ecc', '--batch', '4'], capture_output=True,
                       text=True, cwd=ROOT)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads((dst / 'transforms.json').read_text())
    assert sorted(got) == ['%03d' % i for i in range(6)] and (dst / 'failed.log').read_text() == ''
    for index in sorted(got):
        T = np.array(got[index]['transform'])
        print(index, got[index]['type'], '%.3f px' % C.cli_error(T))
        assert got[index]['type'] == 'ecc_gradient_similarity' and got[index]['model'] == 'similarity'
        assert T[0, 0] == T[1, 1] and T[0, 1] == -T[1, 0] and np.array_equal(T[2], [0.0, 0.0, 1.0])
        assert C.cli_error(T) <= C.SIMILARITY_CAP
    stages = int(re.search(r'ecc_gradient_similarity: (\d+)', r.stdout).group(1))
    assert 6 <= stages <= 12                                      # the final stage of all six pairs, and the pyramid's where it held


def test_align_images_cli_ecc_flag(tmp_path):
    """--ecc: the ECC candidate next to the mutual-information ones (in process: one pair, one bin size)."""
    import align_images
    src, dst = tmp_path / 'in', tmp_path / 'out'
    _write_pairs(str(src), 1)
    cfg = dict(CLI_CFG, use_image_pyramid=False, **{'alignment/bin_sizes': [16]})
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    base = ['-y', str(tmp_path / 'cfg.yaml'), '-i', str(src), '--save-candidates']
    align_images.main(base + ['-o', str(tmp_path / 'plain')])
    align_images.main(base + ['-o', str(dst), '--ecc'])
    got = json.loads((dst / 'transforms.json').read_text())
    assert sorted(got) == ['000'] and got['000']['type'] in ('bin16_normalized_s0_similarity', 'ecc_gradient_similarity')
    plain = sorted(os.listdir(str(tmp_path / 'plain' / 'aligned' / 'all')))
    both = sorted(os.listdir(str(dst / 'aligned' / 'all')))
    assert both == plain + ['000_optical_%d.png' % len(plain)]                     # the same candidates and the ECC one
    args = align_images.build_parser().parse_args([])
    assert args.method is None and args.ecc is False
    with pytest.raises(SystemExit):
        align_images.build_parser().parse_args(['--method', 'ncc'])


def test_predict_cli_ecc_refine(tmp_path):
    d = tmp_path / 'multipoint'
    d.mkdir()
    with open(os.path.join(ROOT, 'model_weights', 'multipoint', 'params.yaml')) as f:
        (d / 'params.yaml').write_text(f.read())
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'config_image_pair_dataset_prediction.yaml')))
    cfg['dataset'].update({'num_samples': 2, 'height': 96, 'width': 120})
    cfg['dataset']['augmentation']['homographic']['enable'] = False
    cfg['prediction'].update({'topk': 300, 'batchsize': 1, 'num_worker': 0, 'ecc_alignment': {'max_iterations': 20}})
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'predict_align_image_pair.py'), '-y', str(tmp_path / 'cfg.yaml'),
                        '-m', str(d), '-v', 'none', '--ecc-refine', '--ecc-transform', 'similarity'],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout.split('\n')
    lines = [l for l in out if l.startswith('ECC alignment:')]
    print(lines)
    assert len(lines) == 1
    ok = re.fullmatch(r'ECC alignment: gradient similarity rho -?\d\.\d+ after \d+ iterations \((converged|iteration limit)\)', lines[0])
    none = re.fullmatch(r'ECC alignment: none \(.+ after \d+ iterations\)', lines[0])
    assert ok or none, lines[0]
    if ok:
        assert out[out.index(lines[0]) + 1] == 'ECC-aligned Homography:'
