"""GPU: correct_alignment.py on three planted 96 x 128 pairs as 8-bit files in align_images.py's output layout: the
files it writes, the report, that nothing that existed changes, and the unchanged check_alignment.py --auto proposing the new
alternative."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

import field_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(script, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return r.stdout


def _tree(d):
    out = {}
    for base, _, files in os.walk(str(d)):
        for f in files:
            p = os.path.join(base, f)
            out[os.path.relpath(p, str(d))] = hashlib.sha256(open(p, 'rb').read()).hexdigest()
    return out


@pytest.fixture()
def layout(tmp_path):
    d = tmp_path / 'data'
    best = d / 'aligned' / 'best'
    best.mkdir(parents=True)
    for index, kind in (('000', 'aligned'), ('001', 'smooth'), ('002', 'featureless')):
        o, t, _ = C.planted(kind)
        Image.fromarray(C.u8(o)).save(str(best / (index + '_optical.png')))
        Image.fromarray(C.u8(t)).save(str(best / (index + '_thermal.png')))
    (d / 'aligned' / 'all').mkdir()                                      # an alternative align_images.py left: number 0 is taken
    Image.fromarray(C.u8(C.planted('smooth')[0])).save(str(d / 'aligned' / 'all' / '001_optical_0.png'))
    (d / 'transforms.json').write_text('{}')
    return d


def test_corrected_alternative_and_proposal(layout):
    d = layout
    before = _tree(d)
    out = _run('correct_alignment.py', '-i', d, '-y', os.path.join(ROOT, 'configs', 'config_correct_alignment.yaml'))
    assert 'Corrected 1 of 3 pairs' in out
    after = _tree(d)
    for f, digest in before.items():                                   # no file that existed changes its bytes
        assert after[f] == digest, f
    new = sorted(set(after) - set(before))
    assert new == sorted([os.path.join('aligned', 'all', '001_optical_1.png'), os.path.join('corrected', '001_field.npz'),
                          os.path.join('corrected', '001_before.png'), os.path.join('corrected', '001_after.png'),
                          os.path.join('corrected', 'report.json')])
    report = json.loads((d / 'corrected' / 'report.json').read_text())
    pairs = report['pairs']
    assert report['config']['fit']['smoothness'] == 0.25 and report['config']['fit']['rounds'] == 3
    assert (pairs['000']['applied'], pairs['000']['reason'], pairs['000']['alternative']) == (False, 'aligned', None)
    assert (pairs['001']['applied'], pairs['001']['reason'], pairs['001']['alternative']) == (True, 'applied', 1)    # the next free number
    assert (pairs['002']['applied'], pairs['002']['reason'], pairs['002']['alternative']) == (False, 'coverage', None)
    meds = [s['median_mag'] for s in pairs['001']['summaries']]
    print('smooth pair from 8-bit files: median residual by round', meds)
    assert len(meds) == 4 and abs(meds[0] - C.REACHED['smooth']['first']) < 0.05 and meds[-1] < 0.1
    assert pairs['002']['summaries'][0]['median_mag'] is None            # NaN as null
    z = np.load(str(d / 'corrected' / '001_field.npz'))
    assert z['U'].shape == (4, 6, 2) and z['geometry'].tolist() == [23.5, 23.5, 16.0]
    assert len(json.loads(str(z['summaries']))) == 4
    assert C.field_error(z['U'], tuple(z['geometry']), C.planted('smooth')[2]) < 0.1
    with Image.open(str(d / 'aligned' / 'all' / '001_optical_1.png')) as im:
        alt = np.array(im)
    assert alt.shape == C.HW and alt.dtype == np.uint8 and not np.array_equal(alt, C.u8(C.planted('smooth')[0]))
    for tag in ('before', 'after'):
        with Image.open(str(d / 'corrected' / ('001_%s.png' % tag))) as im:
            assert np.array(im).shape == C.HW + (3,)

    _run('check_alignment.py', '-i', d, '--auto')                      # unchanged, it sees an ordinary alternative
    assert (d / 'review' / 'decisions_auto.txt').read_text() == '000 a\n001 1\n002 ?\n'
    res = json.loads((d / 'review' / 'residuals.json').read_text())['pairs']['001']
    assert res['best']['proposal'] == '?' and res['alternatives']['0']['proposal'] == '?' and res['alternatives']['1']['proposal'] == 'a'
    assert res['alternatives']['1']['median_mag'] < 0.1



@pytest.mark.parametrize('colour', [False, True], ids=['grey', 'bgr'])
def test_save_corrected_channels_and_border(tmp_path, colour):
    """The file correct_alignment.py writes: every channel sampled through the one field and rounded as align_images.py rounds, a
    pixel with a tap outside the image written as 0 (not as a blend with the zeros outside), BGR arrays saved in RGB order."""
    sys.path.insert(0, ROOT)
    try:
        import correct_alignment
    finally:
        sys.path.remove(ROOT)
    import field_restatement as F
    rng = np.random.RandomState(4)
    H, W = 40, 72
    optical = rng.randint(30, 256, (H, W, 3) if colour else (H, W)).astype(np.uint8)
    U = rng.uniform(-0.5, 0.5, (2, 4, 2))
    U[0, :, 0] -= 2.5                                                  # the top rows reach above the image
    U[:, -1, 1] += 3.25                                                # and the right columns beyond it
    geo = (12.0, 10.0, 16.0)
    path = tmp_path / 'out.png'
    correct_alignment.save_corrected(str(path), optical, U, geo, 'linear')
    with Image.open(str(path)) as im:
        assert im.mode == ('RGB' if colour else 'L')
        got = np.array(im)
    channels = [optical[:, :, 2 - k] for k in range(3)] if colour else [optical]       # the file's order: R, G, B
    touched = 0
    for k, ch in enumerate(channels):
        want, valid = F.warp(ch.astype(np.float32), U, geo)
        want = np.where(valid == 0, 0, np.clip(np.rint(want), 0, 255)).astype(np.uint8)
        assert np.array_equal(got[:, :, k] if colour else got, want), k
        partial = (valid == 0) & (np.rint(F.warp(ch.astype(np.float32), U, geo)[0]) > 0)
        touched += int(partial.sum())
        assert (want[valid == 0] == 0).all() and (valid[0] == 0).all() and (valid[:, -1] == 0).all() and valid[20, 20] == 1
    assert touched > 0                                                 # some invalid pixels would have held a partial blend
