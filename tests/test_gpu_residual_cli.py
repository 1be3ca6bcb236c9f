"""GPU: check_alignment.py --auto on four planted 96 x 128 pairs in align_images.py's output layout: the files it
writes, the proposals, and phase 2 fed with the proposed file.

Measured medians of |d| with 8-bit files (residuals.json of this test): 0.007 px for the aligned pair and the aligned alternative,
3.000 px for the pairs that are 3 px off.  The test config's thresholds (accept 1.0, reject 2.0) lie well between the two."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import yaml
from PIL import Image

import residual_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEDIAN_ALIGNED_MAX, MEDIAN_OFF = 0.1, 3.0


def _run(*args, expect=0):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'check_alignment.py')] + [str(a) for a in args], capture_output=True,
                       text=True, cwd=ROOT)
    assert r.returncode == expect, (r.returncode, r.stderr[-3000:])
    return r.stdout, r.stderr


def _u8(x):
    return np.rint(np.clip(x, 0, 1) * 255.0).astype(np.uint8)


def _png(path):
    with Image.open(str(path)) as im:
        return np.array(im)


@pytest.fixture()
def layout(tmp_path):
    d = tmp_path / 'data'
    best, alls = d / 'aligned' / 'best', d / 'aligned' / 'all'
    best.mkdir(parents=True)
    alls.mkdir()
    thermal = _u8(1.0 - C.scene(C.HW))
    aligned, off, off_other = _u8(C.scene(C.HW)), _u8(C.scene(C.HW, 3.0, 0.0)), _u8(C.scene(C.HW, 0.0, -3.0))
    for index, optical, th in (('000', aligned, thermal), ('001', off, thermal), ('002', off, thermal),
                               ('003', aligned, np.full(C.HW, 128, np.uint8))):
        Image.fromarray(optical).save(str(best / (index + '_optical.png')))
        Image.fromarray(th).save(str(best / (index + '_thermal.png')))
    Image.fromarray(off_other).save(str(alls / '001_optical_0.png'))
    Image.fromarray(aligned).save(str(alls / '001_optical_1.png'))
    eye = np.eye(3)
    shifted = np.array([[1.0, 0, 0], [0, 1.0, -3.0], [0, 0, 1.0]])
    (d / 'transforms.json').write_text(json.dumps({'000': {'transform': eye.tolist(), 'type': 'init'},
                                                   '002': {'transform': shifted.tolist(), 'type': 'init'}}))
    cfg = {'decision': {'min_coverage': 0.25, 'accept_median_px': 1.0, 'accept_p90_px': 1.5, 'reject_median_px': 2.0}}
    (tmp_path / 'auto.yaml').write_text(yaml.safe_dump(cfg))
    return d, tmp_path / 'auto.yaml', aligned


def test_auto_proposals_and_phase_two(layout):
    d, cfg, aligned = layout
    plain = d / 'plain'
    out, _ = _run('-i', d, '--review-dir', plain)
    assert 'review pictures of 4 pairs' in out
    assert not [f for f in os.listdir(str(plain)) if 'residual' in f or 'auto' in f]      # without --auto: nothing new
    plain_files = sorted(os.listdir(str(plain)))

    out, _ = _run('-i', d, '--auto', '--auto-config', cfg)
    review = d / 'review'
    files = sorted(os.listdir(str(review)))
    extra = ['%03d_residual.png' % i for i in range(4)] + ['decisions_auto.txt', 'residuals.json']
    assert files == sorted(plain_files + extra)
    for f in plain_files:                                              # the existing files keep their bytes
        assert (review / f).read_bytes() == (plain / f).read_bytes(), f
    assert (review / 'decisions_template.txt').read_text() == ''.join('%03d ?\n' % i for i in range(4))
    assert (review / 'decisions_auto.txt').read_text() == '000 a\n001 1\n002 r\n003 ?\n'
    assert 'Proposed 3 of 4 pairs (1 left to the reviewer)' in out
    for i in range(4):
        assert _png(review / ('%03d_residual.png' % i)).shape == C.HW + (3,)

    res = json.loads((review / 'residuals.json').read_text())
    pairs = res['pairs']
    assert res['config']['decision']['reject_median_px'] == 2.0 and res['config']['residual']['window'] == 32
    assert [pairs['%03d' % i]['proposal'] for i in range(4)] == ['a', '1', 'r', '?']
    print({k: (v['best']['median_mag'], v['best']['coverage']) for k, v in pairs.items()},
          {k: v['median_mag'] for k, v in pairs['001']['alternatives'].items()})
    assert pairs['000']['best']['median_mag'] <= MEDIAN_ALIGNED_MAX and pairs['000']['best']['coverage'] > 0.8
    assert abs(pairs['001']['best']['median_mag'] - MEDIAN_OFF) < 0.2 and abs(pairs['002']['best']['median_mag'] - MEDIAN_OFF) < 0.2
    assert pairs['002']['best']['median_d'][0] == pytest.approx(3.0, abs=0.2)
    assert sorted(pairs['001']['alternatives']) == ['0', '1']
    assert pairs['001']['alternatives']['1']['median_mag'] <= MEDIAN_ALIGNED_MAX
    assert pairs['001']['alternatives']['0']['proposal'] == 'r' and pairs['001']['best']['proposal'] == 'r'
    assert pairs['003']['best']['confident'] == 0 and pairs['003']['best']['median_mag'] is None
    assert (pairs['000']['masked'], pairs['001']['masked'], pairs['002']['masked']) == (True, False, True)

    _, err = _run('-i', d, '--auto', '--decisions', review / 'decisions_auto.txt', expect=2)
    assert '--auto' in err and not (d / 'aligned' / 'accepted').exists()

    out, _ = _run('-i', d, '--decisions', review / 'decisions_auto.txt')      # phase 2, unchanged, fed with the proposals
    assert 'Accepted 2 images out of 4' in out
    accepted = d / 'aligned' / 'accepted'
    assert sorted(os.listdir(str(accepted))) == ['000_optical.png', '000_thermal.png', '001_optical.png', '001_thermal.png']
    assert np.array_equal(_png(accepted / '001_optical.png'), aligned)  # the alternative the digit names
    assert (d / 'checked.log').read_text().split() == ['000_optical.png', '001_optical.png', '002_optical.png']
