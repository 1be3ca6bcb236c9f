"""CPU: the fixture conditions of the pooled ECC tests under the float64 restatement alone -- what pooling
gains on the six-pair recording, what one mis-paired frame and static artefacts do to it and what the rejection round and the
grown static masks give back, and the group rules.  The numbers in the comments are what the restatement reaches."""
import numpy as np
import pytest

import ecc_cases as C
import ecc_pooled_cases as PC
import ecc_pooled_restatement as PR
import ecc_restatement as E

MODELS = ('similarity', 'affine', 'homography')


@pytest.mark.parametrize('model', MODELS)
def test_six_pair_recording(model):
    """Starts 3, 7 and 10 px off end under the cap (0.083 / 0.099 / 0.194 px) and within 0.05 px of each other."""
    ends = [PC.restated('clean', t, model) for t in (3.0, 7.0, 10.0)]
    for r in ends:
        print(model, 'error %.3f nit %d' % (PC.error(r['transform']), r['nit']))
        assert r['success'] and r['included'].all()
        assert PC.error(r['transform']) <= PC.CLEAN_CAP[model]
    for r in ends[1:]:
        assert C.corner_distance(r['transform'], ends[0]['transform'], PC.THERMAL_HW) <= PC.SAME_POINT


def test_single_pairs_do_not_determine_a_homography():
    """The case for pooling: from the 10 px start at least two of the six single-pair homographies end beyond 2 px."""
    planes, templates = PC.features('clean')
    errors = []
    for i in range(6):
        r = E.refine_features(planes[i], templates[i], PC.start(10.0), 'homography', PC.FIXTURE_EPS, 50, 0.25)
        errors.append(PC.error(r['transform']))
    print('single-pair homographies', np.round(errors, 2))
    assert sum(e > 2.0 for e in errors) >= 2


def test_mispaired_frame():
    """rho_2 < 0.1 (0.033), every other rho_i > 0.9; the rejection round drops exactly pair 2; the homography after it is within
    0.3 px (0.106) and below the first run's error (0.575)."""
    r = PC.restated('mispaired', 7.0, 'homography', reject_ratio=0.5)
    first = r['first']
    assert first is not None and first['success']
    rho = first['rho_pair']
    print('rho_i', np.round(rho, 3), 'first %.3f after %.3f' % (PC.error(first['transform']), PC.error(r['transform'])))
    assert rho[PC.MISPAIRED] < 0.1 and all(rho[i] > 0.9 for i in range(6) if i != PC.MISPAIRED)
    assert list(np.nonzero(r['rejected'])[0]) == [PC.MISPAIRED]
    assert r['success'] and PC.error(r['transform']) <= PC.REJECTED_CAP
    assert PC.error(r['transform']) < PC.error(first['transform'])
    off = PC.restated('mispaired', 7.0, 'homography', reject_ratio=0.0)
    assert off['first'] is None and not off['rejected'].any()
    assert np.array_equal(off['transform'], first['transform'])


@pytest.mark.parametrize('model', MODELS)
def test_artefact_recording(model):
    """Without masks the static structure pulls the estimate away (similarity 2.73 px; affine and homography end in LAMBDA);
    with the static masks grown by the feature's support it is back under the cap (0.074 / 0.121 / 0.401 px)."""
    bare = PC.restated('artefact', 7.0, model)
    print(model, 'no mask: status', bare['status'], 'error %.3f' % PC.error(bare['transform']))
    if model == 'similarity':
        assert PC.error(bare['transform']) > 1.5
    else:
        assert bare['status'] == PR.LAMBDA and not bare['success']
    masked = PC.restated('artefact', 7.0, model, masked=True)
    print(model, 'masked: error %.3f' % PC.error(masked['transform']))
    assert masked['success'] and PC.error(masked['transform']) <= PC.MASKED_CAP[model]


def test_static_masks():
    """The static masks of the artefact recording are the planted sets exactly; on the clean recording nothing is static."""
    o, t = PC.planted_masks()
    optical, thermal = PC.recording('artefact')
    assert np.array_equal(PR.static_mask(optical), o) and np.array_equal(PR.static_mask(thermal), t)
    optical, thermal = PC.recording('clean')
    assert PR.static_mask(optical).all() and PR.static_mask(thermal).all()


def test_grow():
    m = np.ones((9, 11), np.uint8)
    m[0, 0] = m[4, 5] = 0
    g = PR.grow(m, 2)
    want = np.ones_like(m)
    want[:3, :3] = 0
    want[2:7, 3:8] = 0
    assert np.array_equal(g, want)
    assert np.array_equal(PR.grow(m, 0), m) and not PR.grow(m, 17).any() and PR.grow(np.ones_like(m), 3).all()
    assert PR.mask_radii('gradient', 5) == (3, 4) and PR.mask_radii('intensity', 5) == (2, 3) and PR.mask_radii('gradient', 1) == (1, 2)


@pytest.mark.parametrize('model', MODELS)
def test_group_of_one_is_the_pair_algorithm(model):
    planes, templates = PC.features('clean')
    want = E.refine_features(planes[0], templates[0], PC.start(3.0), model, 1e-6, 50, 0.25)
    got = PR.refine_group(planes[:1], templates[:1], PC.start(3.0), model, 1e-6, 50, 0.25)
    assert got['nit'] == want['nit'] and got['status'] == want['status'] and got['converged'] == want['converged']
    assert np.abs(got['transform'] - want['transform']).max() <= 1e-12


def test_excluded_pair_adds_nothing():
    """A group with an excluded pair (inactive, or with a constant thermal frame) has the iterates of the group without it."""
    planes, templates = PC.features('clean')
    without, inactive, constant = [], [], []
    keep = [0, 1, 3, 4, 5]
    PR.refine_group([planes[i] for i in keep], [templates[i] for i in keep], PC.start(7.0), 'homography', 0.0, 5, history=without)
    PR.refine_group(planes, templates, PC.start(7.0), 'homography', 0.0, 5, active=[i != 2 for i in range(6)], history=inactive)
    flat = list(templates)
    flat[2] = np.zeros_like(templates[2])
    r = PR.refine_group(planes, flat, PC.start(7.0), 'homography', 0.0, 5, history=constant)
    assert not r['included'][2] and np.isnan(r['rho_pair'][2]) and r['included'].sum() == 5
    for a, b, c in zip(without, inactive, constant):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0]) and a[1] == b[1] == c[1]
    none = PR.refine_group(planes, templates, PC.start(7.0), 'similarity', active=[False] * 6)
    assert none['status'] == PR.FEW_VALID and none['nit'] == 0


def test_other_groups():
    """group_case(): 0.094 / 0.104 / 0.208 px; shift_groups_case(): similarity 0.204 / 0.162 / 0.104 px."""
    for model in MODELS:
        r = PC.group_restated(7.0, model)
        print('group_case', model, '%.3f' % PC.error(r['transform']))
        assert r['success'] and PC.error(r['transform']) <= PC.CLEAN_CAP[model]
    optical, thermal, gid, truths, starts = PC.shift_groups()
    for g in range(3):
        sel = np.nonzero(gid == g)[0]
        planes = [E.image_planes(E.features(optical[i], PC.KSIZE)) for i in sel]
        templates = [E.features(thermal[i], PC.KSIZE) for i in sel]
        r = PR.refine_group(planes, templates, starts[g], 'similarity', PC.FIXTURE_EPS)
        print('shift group', g, '%.3f' % PC.shift_error(r['transform'], g))
        assert r['success'] and PC.shift_error(r['transform'], g) <= 0.5
