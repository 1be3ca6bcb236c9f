"""GPU (MI355X): estimate_initial_transform.py with the pooled ECC refinement (--ecc-refine, --method ecc, the mask flags) on the
planted recording written as PNG files: optical 96 x 128 (8 bit), thermal 72 x 96 (16 bit), six pairs, one transform.  One run
goes through the command line as a process; the others call its main() with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

import ecc_pooled_cases as PC
import estimate_initial_transform as cli

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ECC_KEYS = ['converged', 'corner_shift', 'feature', 'filter_size', 'iterations', 'model', 'optical_mask_kept', 'pairs', 'reject_ratio',
            'rho_end', 'rho_start', 'rounds', 'status', 'success', 'thermal_mask_kept']


def _write(directory, kind):
    from PIL import Image
    optical, thermal = PC.raw(kind)
    os.makedirs(directory, exist_ok=True)
    for i, (o, t) in enumerate(zip(optical, thermal)):
        Image.fromarray(o).save(os.path.join(directory, '%d_optical.png' % i))
        Image.fromarray(t).save(os.path.join(directory, '%d_thermal.png' % i))
    return directory


def _init(path, target=7.0):
    with open(path, 'wt') as fh:
        yaml.safe_dump({'perspective': [[float(v) for v in row] for row in PC.start(target)]}, fh)
    return str(path)


def _result(directory):
    T = np.array(yaml.safe_load(open(os.path.join(directory, 'initial_transform.yaml')))['perspective'], np.float64)
    return T, json.load(open(os.path.join(directory, 'initial_transform_report.json')))


def test_fourier_then_ecc(tmp_path):
    """Through the command line: the Fourier-Mellin similarity refined to a homography over all six pairs lands within the host
    cap of the planted transform; without the new flag the report has no `ecc` key and the yaml is the estimate; --force as
    before."""
    pairs = _write(tmp_path / 'preprocessed', 'clean')
    assert cli.main(['-i', str(pairs), '--method', 'fourier', '--batch', '4']) == 0
    T_plain, report = _result(pairs)
    assert 'ecc' not in report
    base = [sys.executable, os.path.join(ROOT, 'estimate_initial_transform.py'), '-i', str(pairs), '--method', 'fourier', '--batch', '4',
            '--ecc-refine', '--ecc-transform', 'homography']
    refused = subprocess.run(base, capture_output=True, text=True, cwd=ROOT)
    assert refused.returncode == 2 and 'force' in refused.stderr
    assert np.array_equal(_result(pairs)[0], T_plain)
    out = subprocess.run(base + ['--force'], capture_output=True, text=True, cwd=ROOT)
    print(out.stdout[-1500:])
    assert out.returncode == 0, out.stderr[-2000:]
    T, report = _result(pairs)
    ecc = report['ecc']
    print('estimate %.3f px, refined %.3f px' % (PC.error(T_plain), PC.error(T)))
    assert report['method'] == 'fourier' and sorted(ecc) == ECC_KEYS
    assert ecc['model'] == 'homography' and ecc['feature'] == 'gradient' and ecc['filter_size'] == 5 and ecc['success']
    assert ecc['rho_end'] > ecc['rho_start'] and ecc['rho_end'] > 0.9 and ecc['iterations'] >= 1 and ecc['rounds'] % 8 == 0
    assert sorted(ecc['pairs']) == [str(i) for i in range(6)]
    for v in ecc['pairs'].values():
        assert sorted(v) == ['rejected', 'rho', 'valid_share'] and not v['rejected'] and v['rho'] > 0.9 and 0.5 < v['valid_share'] <= 1.0
    assert ecc['thermal_mask_kept'] == ecc['optical_mask_kept'] == 1.0
    assert T[2, 2] == 1.0 and PC.error(T) <= PC.CLEAN_CAP['homography']
    assert 0.0 < ecc['corner_shift'] < 5.0


def test_method_ecc_from_a_yaml(tmp_path):
    pairs = _write(tmp_path / 'preprocessed', 'clean')
    init = _init(tmp_path / 'measured.yaml')
    assert cli.main(['-i', str(pairs), '--method', 'ecc']) == 2                     # no --init
    assert cli.main(['-i', str(pairs), '--method', 'fourier', '--auto-mask']) == 2  # a mask flag without the refinement
    assert cli.main(['-i', str(pairs), '--method', 'ecc', '--init', init, '--ecc-transform', 'homography', '--batch', '4']) == 0
    T, report = _result(pairs)
    print('refined %.3f px' % PC.error(T))
    assert report['method'] == 'ecc' and report['pairs_used'] == 6 and sorted(report['ecc']) == ECC_KEYS
    assert PC.error(T) <= PC.CLEAN_CAP['homography']
    assert 3.0 < report['ecc']['corner_shift'] < 20.0                                 # the start was 7 thermal px off


def test_masks_on_the_artefact_files(tmp_path):
    """--auto-mask meets the masked cap where the same command without it does not; explicit mask images give the same file."""
    from PIL import Image
    pairs = _write(tmp_path / 'preprocessed', 'artefact')
    init = _init(tmp_path / 'measured.yaml')
    base = ['-i', str(pairs), '--method', 'ecc', '--init', init, '--ecc-transform', 'similarity', '--force']
    assert cli.main(base) == 0
    bare = PC.error(_result(pairs)[0])
    assert cli.main(base + ['--auto-mask']) == 0
    T_auto, report = _result(pairs)
    o, t = PC.planted_masks()
    Image.fromarray(o * 255).save(tmp_path / 'optical_mask.png')
    Image.fromarray(t * 255).save(tmp_path / 'thermal_mask.png')
    assert cli.main(base + ['--optical-mask', str(tmp_path / 'optical_mask.png'), '--thermal-mask', str(tmp_path / 'thermal_mask.png')]) == 0
    T_given, given = _result(pairs)
    print('bare %.3f px, masked %.3f px' % (bare, PC.error(T_auto)))
    assert bare > PC.MASKED_CAP['similarity'] and PC.error(T_auto) <= PC.MASKED_CAP['similarity']
    assert np.array_equal(T_auto, T_given) and report['ecc'] == given['ecc']
    tk, ok = PC.grown_masks()
    assert report['ecc']['thermal_mask_kept'] == pytest.approx(tk.mean(), abs=1e-6)
    assert report['ecc']['optical_mask_kept'] == pytest.approx(ok.mean(), abs=1e-6)
    # the eight-parameter model fails without the masks (lambda): nothing is written and the exit status says so
    os.remove(os.path.join(pairs, 'initial_transform.yaml'))
    assert cli.main(['-i', str(pairs), '--method', 'ecc', '--init', init, '--ecc-transform', 'homography']) == 1
    assert not os.path.exists(os.path.join(pairs, 'initial_transform.yaml'))
    assert cli.main(['-i', str(pairs), '--method', 'ecc', '--init', init, '--ecc-transform', 'homography', '--auto-mask']) == 0
    assert PC.error(_result(pairs)[0]) <= PC.MASKED_CAP['homography']
