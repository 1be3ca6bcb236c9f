"""GPU (MI355X): estimate_initial_transform.py --method fourier end to end on planted pairs written as PNG files: optical frames
of 96 x 128 (8 bit), thermal frames of 72 x 96 (16 bit), one shared similarity."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml

import registration_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write(directory, optical, thermal):
    from PIL import Image
    os.makedirs(directory, exist_ok=True)
    for i, (o, t) in enumerate(zip(optical, thermal)):
        Image.fromarray(o).save(os.path.join(directory, '%d_optical.png' % i))
        Image.fromarray(t).save(os.path.join(directory, '%d_thermal.png' % i))


def _run(directory, *extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'estimate_initial_transform.py'), '-i', str(directory), '--method',
                           'fourier', '--batch', '4'] + list(extra), capture_output=True, text=True, cwd=ROOT)


def test_fourier_method_end_to_end(tmp_path):
    optical, thermal, T_true = C.cli_pairs()
    pairs = tmp_path / 'preprocessed'
    _write(pairs, optical, thermal)
    # another model than the similarity: exit status 2 before anything is read
    bad = _run(pairs, '--transform', 'affine')
    assert bad.returncode == 2 and 'similarity' in bad.stderr and not (pairs / 'initial_transform.yaml').exists()
    out = _run(pairs)                                   # six pairs in chunks of 4 and 2: the accumulating path
    print(out.stdout[-1500:])
    assert out.returncode == 0, out.stderr[-2000:]
    written = (pairs / 'initial_transform.yaml').read_text()
    P = np.array(yaml.safe_load(written)['perspective'], np.float64)
    assert P.shape == (3, 3) and P[2].tolist() == [0.0, 0.0, 1.0]
    # perspective is thermal pixel -> optical pixel, as align_images.py reads it: the thermal corners against the truth
    err = C.corner_error(P, np.linalg.inv(T_true), hw=C.GROUP['thermal_hw'])
    err_t = C.corner_error(np.linalg.inv(P), T_true)
    print('thermal corners: %.3f optical px from the truth; optical corners: %.3f thermal px' % (err, err_t))
    assert err <= 1.5
    report = json.load(open(pairs / 'initial_transform_report.json'))
    assert report['method'] == 'fourier' and report['transform'] == 'similarity'
    assert report['pairs_read'] == report['pairs_used'] == 6 and report['branch_180'] is False
    assert sorted(report['similarity']) == ['angle', 'dx', 'dy', 'scale']
    assert report['similarity']['scale'] == pytest.approx(C.GROUP['scale'], rel=0.02)
    assert report['similarity']['angle'] == pytest.approx(-np.radians(C.GROUP['angle']), abs=np.radians(1.0))    # decompose_similarity's sign
    for stage in ('stage1', 'stage2'):
        s = report[stage]
        assert sorted(s) == ['peak', 'ratio', 'second'] and s['ratio'] == pytest.approx(s['peak'] / s['second']) and s['ratio'] >= 1.25
    # an existing yaml is refused without --force and stays as it is
    again = _run(pairs)
    assert again.returncode == 2 and 'force' in again.stderr and (pairs / 'initial_transform.yaml').read_text() == written


def test_flat_frames_write_nothing(tmp_path):
    flat = tmp_path / 'flat'
    _write(flat, np.full((2, 96, 128), 90, np.uint8), np.full((2, 72, 96), 30000, np.uint16))
    out = _run(flat)
    assert out.returncode == 1 and 'nothing written' in out.stderr
    assert sorted(os.listdir(flat)) == ['0_optical.png', '0_thermal.png', '1_optical.png', '1_thermal.png']
