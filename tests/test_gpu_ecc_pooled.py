"""GPU: csrc/ecc_pooled.hip and the pooled entries of multipoint_amd.utils.ecc against the float64 restatement
(tests/ecc_pooled_restatement.py) -- mask growth and the static mask bit for bit, the raw sums with masks, one group step, whole
trajectories, group indexing, exclusion and failures, the bits, the rejection round and the refusals."""
import numpy as np
import pytest

import ecc_cases as C
import ecc_pooled_cases as PC
import ecc_pooled_restatement as PR
import ecc_restatement as E
import registration_cases as RC
from multipoint_amd.utils import ecc as U
from test_gpu_ecc import MODELS, SHAPES, SUM_SLACK, frames, gpu, transforms_for

pytestmark = pytest.mark.gpu

KEYS = ('transform', 'rho', 'nit', 'status', 'converged', 'n_included', 'rho_pair', 'valid_pair', 'included')


def same_bits(a, b, groups=None, pairs=None, other_groups=None, other_pairs=None):
    """Every field of two results bit for bit, over chosen groups / pairs of each."""
    for k in KEYS:
        x, y = getattr(a, k), getattr(b, k)
        if k in ('rho_pair', 'valid_pair', 'included'):
            x = x if pairs is None else x[pairs]
            y = y if other_pairs is None else y[other_pairs]
        else:
            x = x if groups is None else x[groups]
            y = y if other_groups is None else y[other_groups]
        assert np.array_equal(x, y, equal_nan=True), k


def seeded(hw, seed=3, share=0.02):
    m = np.ones(hw, np.uint8)
    rng = np.random.default_rng(seed)
    m[rng.random(hw) < share] = 0
    return m


@pytest.mark.parametrize('hw', ((8, 8), (13, 17), (72, 96)))
def test_mask_growth(hw):
    H, W = hw
    none, corner, centre, every = (np.ones(hw, np.uint8) for _ in range(4))
    corner[0, 0] = 0
    centre[H // 2, W // 2] = 0
    every[:] = 0
    masks = np.stack([none, corner, centre, every, seeded(hw)])
    for R in (0, 1, 3, 17):
        want = np.stack([PR.grow(m, R) for m in masks])
        got = U.grow_mask(gpu(masks), R).cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, want), R
        assert np.array_equal(U.grow_mask(gpu(masks[4] * 200), R).cpu().numpy(), want[4])           # any nonzero value is 'use'
        assert np.array_equal(U.grow_mask(gpu(masks[2].astype(bool)), R).cpu().numpy(), want[2])
    assert U.ecc_mask_radii('gradient', 5) == (3, 4) and U.ecc_mask_radii('intensity', 5) == (2, 3)
    assert U.ecc_mask_radii('gradient', 1) == (1, 2) and U.ecc_mask_radii('intensity', 1) == (0, 1)


def test_static_mask():
    """The same frames in batches of 1, of 3 and all at once give the same plane: the planted sets on the artefact recording,
    nothing on the clean one."""
    for kind in ('artefact', 'clean'):
        for frames_ in PC.recording(kind):
            want = PR.static_mask(frames_)
            planes = []
            for batch in (1, 3, len(frames_)):
                sm = U.StaticMask(frames_.shape[1:], 'cuda')
                for at in range(0, len(frames_), batch):
                    sm.update(gpu(frames_[at:at + batch]))
                planes.append(sm.mask().cpu().numpy())
            for p in planes:
                assert p.dtype == np.uint8 and np.array_equal(p, want), kind
    o, t = PC.planted_masks()
    optical, thermal = PC.recording('artefact')
    assert np.array_equal(PR.static_mask(optical), o) and np.array_equal(PR.static_mask(thermal), t)
    with pytest.raises(ValueError):
        U.StaticMask((16, 16), 'cuda').mask()


POOLED_SHAPES = SHAPES + (((65, 64), (70, 75)),)
MASK_CASES = ('none', 'edge', 'chunk', 'optical', 'thermal', 'both')


def case_masks(case, thw, ihw, rt):
    """(thermal use-mask or None, optical use-mask or None) of a mask case, BEFORE growth.  'chunk': the grown excluded set
    covers every row that holds a pixel of the first chunk of 4096 (on a 64-wide template it ends exactly on the chunk boundary;
    a one-chunk template is excluded whole).  'edge': it begins at the row that holds pixel 4096, the first of the second
    chunk, where the template is tall enough for the growth, else it is the bottom rows."""
    (H, W), (Ho, Wo) = thw, ihw
    t = np.ones(thw, np.uint8)
    o = np.ones(ihw, np.uint8)
    o[Ho // 3:Ho // 3 + 2, Wo // 4:Wo // 2] = 0
    o[:, :1] = 0
    if case == 'none':
        return None, None
    if case == 'edge':
        t[min(4096 // W, H - 1) + rt:] = 0
        if not (t == 0).any():
            t[-1] = 0
        return t, None
    if case == 'chunk':
        t[:max(min(-(-4096 // W), H) - rt, 1)] = 0
        return t, None
    if case == 'optical':
        return None, o
    t[H // 2, W // 3:W // 2] = 0
    t[:1] = 0
    return (t, None) if case == 'thermal' else (t, o)


@pytest.mark.parametrize('B', (1, 3))
@pytest.mark.parametrize('shapes', POOLED_SHAPES)
def test_sums_with_masks(shapes, B):
    """The valid count exact and every sum within test_gpu_ecc.test_sums' bound of the restatement on the kept set; B = 3 runs
    two groups (ids 0, 1, 0) with per-group masks, the second group's being all 'use'."""
    thw, ihw = shapes
    opt, th = frames(21, B, ihw), frames(22, B, thw)
    kinds = transforms_for(thw, ihw)
    names = sorted(kinds)
    group = [0, 1, 0][:B]
    G = max(group) + 1
    rt, ro = U.ecc_mask_radii('gradient', 5)
    packed = U.ecc_features(gpu(opt), 'gradient', 5, packed=True)[1].cpu().numpy().astype(np.float64)
    planes = [(pk[:, :, 0], pk[:, :, 1], pk[:, :, 2]) for pk in packed]
    template = U.ecc_features(gpu(th), 'gradient', 5).cpu().numpy().astype(np.float64)
    for case in MASK_CASES:
        t, o = case_masks(case, thw, ihw, rt)
        tm = None if t is None else (t if G == 1 else np.stack([t, np.ones_like(t)]))
        om = None if o is None else (o if G == 1 else np.stack([o, np.ones_like(o)]))
        prob = U.SharedEccProblem('gradient', 5).add(gpu(opt), gpu(th), group).finish(
            None if tm is None else gpu(tm), None if om is None else gpu(om))
        tgrown = None if t is None else PR.grow(t, rt)
        ogrown = None if o is None else PR.grow(o, ro)
        for model in MODELS:
            for i, kind in enumerate(names):
                Ts = np.stack([kinds[kind], kinds[names[(i + 1) % len(names)]]])[:G]        # another transform for group 1
                got = prob.sums(Ts, model)
                assert got.shape == (B, U.ecc_sum_count(model))
                for p, g in enumerate(group):
                    ref, mag = PR.pair_sums(planes[p], template[p], Ts[g], model, tgrown if g == 0 else None,
                                            ogrown if g == 0 else None, magnitudes=True)
                    assert got[p, 0] == ref[0], (case, model, kind, p, 'valid count')
                    if case == 'chunk' and thw[0] * thw[1] <= 4096 and g == 0:
                        assert not got[p].any()                                    # every pixel skipped: zeros, no stale sums
                    bad = np.abs(got[p] - ref) > SUM_SLACK * mag
                    assert not bad.any(), (case, model, kind, p, np.nonzero(bad)[0])
    # no mask, groups of one: the bits of ecc_sums
    Ts = np.stack([kinds[names[i % len(names)]] for i in range(B)])
    for model in MODELS:
        a = U.ecc_pooled_sums(gpu(opt), gpu(th), list(range(B)), Ts, model)
        assert np.array_equal(a, U.ecc_sums(gpu(opt), gpu(th), list(range(B)), Ts, model)), model


def test_mask_forms_agree():
    """(H, W) masks for all groups and the same masks repeated as (G, H, W) give the same sums; bool and uint8 alike."""
    optical, thermal = PC.recording('artefact')
    o, t = PC.planted_masks()
    group = [0, 1, 1, 0, 2, 2]
    T = np.stack([PC.start(3.0)] * 3)
    a = U.ecc_pooled_sums(gpu(optical), gpu(thermal), group, T, 'affine', thermal_mask=gpu(t), optical_mask=gpu(o))
    b = U.ecc_pooled_sums(gpu(optical), gpu(thermal), group, T, 'affine', thermal_mask=gpu(np.stack([t] * 3).astype(bool)),
                          optical_mask=gpu(np.stack([o] * 3) * 255))
    assert np.array_equal(a, b)
    assert (a[:, 0] < U.ecc_pooled_sums(gpu(optical), gpu(thermal), group, T, 'affine')[:, 0]).all()


@pytest.mark.parametrize('model', MODELS)
@pytest.mark.parametrize('P', (1, 4, 6))
def test_group_step(P, model):
    """One update of a group on the GPU's own per-pair sums against the numpy pooled solve, with test_gpu_ecc.test_solve_step's
    bound on the pooled matrices: 1000 * 2^-53 * cond(Hs) * (|dp| + |Hs^-1| V)."""
    optical, thermal = (x[:P] for x in PC.recording('clean'))
    T0 = E.start_transform(PC.start(3.0), model)
    K = E.PARAMS[model]
    prob = U.SharedEccProblem().add(gpu(optical), gpu(thermal)).finish()
    s = prob.sums(T0, model)
    status, Tn, rho, _, rho_i, inc = PR.group_solve(list(s), T0, model, thermal[0].size, eps=0.0)
    assert status is None and inc.all()
    r = prob.refine(T0, model, eps=0.0, maxiter=1, chunk=1, reject_ratio=0.0)
    assert r.nit[0] == 1 and r.success[0] and not r.converged[0] and r.rounds == 1 and r.n_included[0] == P
    assert abs(r.rho[0] - rho) <= 1e-12 and np.abs(r.rho_pair - rho_i).max() <= 1e-12
    assert np.array_equal(r.valid_pair, s[:, 0].astype(np.int64)) and r.included.all()
    A, V = np.zeros((K, K)), np.zeros(K)
    lam = 1.0 if rho == 0 else abs(1.0 / rho)
    for sp in s:
        n, (Sw, Sr, _, _, _), SG, Ap, SGw, SGr = E.unpack(sp, K)
        A += Ap
        V += np.abs(SGw) + abs(Sw / n) * np.abs(SG) + 4.0 * lam * (np.abs(SGr) + abs(Sr / n) * np.abs(SG))
    dp = E.parameters(Tn, model) - E.parameters(T0, model)
    bound = 1000.0 * 2.0 ** -53 * np.linalg.cond(A) * (np.abs(dp).max() + (np.abs(np.linalg.inv(A)) @ V).max())
    diff = np.abs(E.parameters(r.transform[0], model) - E.parameters(Tn, model)).max()
    print(model, P, 'cond', np.linalg.cond(A), 'diff', diff, 'bound', bound)
    assert diff <= bound


@pytest.mark.parametrize('maxiter', (1, 3, 10))
@pytest.mark.parametrize('model', ('similarity', 'homography'))
def test_trajectories(model, maxiter):
    """eps = 0: exactly maxiter updates.  The GPU's iterate lies within 4 x the restatement's own float32-against-float64
    distance of the float64 restatement's: the six-pair recording (clean without masks, with artefacts under the planted masks)
    and group_case() (without masks and under the same masks)."""
    o, t = PC.planted_masks()
    tkeep, okeep = PC.grown_masks()
    gopt, gth, _ = RC.group_case()
    worst = 0.0
    runs = []
    for kind, masked in (('clean', False), ('artefact', True)):
        optical, thermal = PC.recording(kind)
        runs.append(('six ' + kind, optical, thermal, masked, PC.restated(kind, 3.0, model, masked, 0.0, maxiter),
                     PC.noise_floor(kind, 3.0, model, maxiter, masked)))
    runs.append(('group', gopt, gth, False, PC.group_restated(3.0, model, 0.0, maxiter), PC.group_noise_floor(3.0, model, maxiter)))
    planes, templates = PC.group_features(False)
    planes32, templates32 = PC.group_features(True)
    a = PR.refine_group(planes, templates, PC.start(3.0), model, 0.0, maxiter, tkeep=tkeep, okeep=okeep)
    b = PR.refine_group(planes32, templates32, PC.start(3.0), model, 0.0, maxiter, f32=True, tkeep=tkeep, okeep=okeep)
    runs.append(('group masked', gopt, gth, True, a, C.corner_distance(a['transform'], b['transform'], PC.THERMAL_HW)))
    for name, optical, thermal, masked, want, floor in runs:
        r = U.estimate_shared_transform_ecc(gpu(optical), gpu(thermal), PC.start(3.0), None, model, eps=0.0, maxiter=maxiter,
                                            thermal_mask=gpu(t) if masked else None, optical_mask=gpu(o) if masked else None,
                                            reject_ratio=0.0)
        assert r.nit[0] == want['nit'] == maxiter and r.status[0] == U.ECC_OK and not r.converged[0]
        d = C.corner_distance(r.transform[0], want['transform'], PC.THERMAL_HW)
        print(name, model, maxiter, 'gpu %.3e floor %.3e ratio %.2f' % (d, floor, d / floor))
        worst = max(worst, d / floor)
        assert d <= 4.0 * floor, (name, d, floor)
    print('worst ratio', worst)


def test_group_indexing():
    """shift_groups_case() with its pairs permuted so that the group ids read 2, 0, 2, 1, 0, 2: every group within 0.5 px under
    the similarity, bit-equal to that group run alone, and the one-pair group the per-pair refinement."""
    optical, thermal, gid, truths, starts = PC.shift_groups()
    perm = [3, 0, 4, 2, 1, 5]
    optical, thermal, gid = optical[perm], thermal[perm], gid[perm]
    assert list(gid) == [2, 0, 2, 1, 0, 2]
    r = U.estimate_shared_transform_ecc(gpu(optical), gpu(thermal), starts, gid, 'similarity', eps=PC.FIXTURE_EPS, reject_ratio=0.0)
    assert r.success.all() and r.converged.all() and list(r.n_included) == [2, 1, 3] and r.included.all()
    for g in range(3):
        err = PC.shift_error(r.transform[g], g)
        print('group', g, 'error %.3f nit %d' % (err, r.nit[g]))
        assert err <= 0.5
        sel = np.nonzero(gid == g)[0]
        alone = U.estimate_shared_transform_ecc(gpu(optical[sel]), gpu(thermal[sel]), starts[g], None, 'similarity',
                                                eps=PC.FIXTURE_EPS, reject_ratio=0.0)
        same_bits(r, alone, groups=[g], pairs=sel)
    one = int(np.nonzero(gid == 1)[0][0])
    pair = U.refine_alignment_ecc_batch(gpu(optical[one]), gpu(thermal[one]), [0], starts[1][None], 'similarity', eps=PC.FIXTURE_EPS)
    assert pair['nit'][0] == r.nit[1] and pair['status'][0] == r.status[1]
    assert C.corner_distance(pair['transform'][0], r.transform[1], PC.THERMAL_HW) <= 1e-9
    assert abs(pair['rho'][0] - r.rho[1]) <= 1e-12 and abs(r.rho_pair[one] - r.rho[1]) <= 1e-12


def test_exclusion_and_failures():
    optical, thermal = (x.copy() for x in PC.recording('clean'))
    start = PC.start(3.0)
    keep = [0, 1, 3, 4, 5]
    without = U.estimate_shared_transform_ecc(gpu(optical[keep]), gpu(thermal[keep]), start, None, 'homography', reject_ratio=0.0)
    assert without.success[0] and without.n_included[0] == 5
    # a constant thermal frame, one NaN pixel in an optical frame, an inactive pair: excluded, and the group has the bits of
    # the group without that pair
    flat = thermal.copy()
    flat[2] = 0.5
    nan = optical.copy()
    nan[2, 48, 64] = np.nan
    for o_, t_, active in ((optical, flat, None), (nan, thermal, None), (optical, thermal, [i != 2 for i in range(6)])):
        r = U.estimate_shared_transform_ecc(gpu(o_), gpu(t_), start, None, 'homography', active=active, reject_ratio=0.0)
        assert not r.included[2] and np.isnan(r.rho_pair[2]) and r.n_included[0] == 5 and r.success[0]
        same_bits(r, without, pairs=keep)
    # every pair of group 1 inactive: FEW_VALID at once; group 2 on raw intensities of inverted pairs would need its own
    # feature, so the LAMBDA group runs in its own call next to a healthy one
    group = [0, 0, 0, 1, 1, 1]
    healthy = U.estimate_shared_transform_ecc(gpu(optical[:3]), gpu(thermal[:3]), start, None, 'similarity', reject_ratio=0.0)
    r = U.estimate_shared_transform_ecc(gpu(optical), gpu(thermal), start, group, 'similarity', active=[1, 1, 1, 0, 0, 0],
                                        reject_ratio=0.0)
    assert r.status[1] == U.ECC_FEW_VALID and not r.success[1] and r.nit[1] == 0 and r.n_included[1] == 0
    assert np.array_equal(r.transform[1], E.start_transform(start, 'similarity'))
    assert not r.included[3:].any() and np.isnan(r.rho_pair[3:]).all()
    same_bits(r, healthy, groups=[0], pairs=[0, 1, 2])
    # lambda's denominator <= 0 at iteration 0: raw intensities of contrast-inverted pairs; the group beside it holds the same
    # optical frames with themselves as the thermal side, cut to the thermal size, and is healthy
    same = np.ascontiguousarray(optical[:3, :72, :96])
    both_o = np.concatenate([optical[:3], optical[:3]])
    both_t = np.concatenate([thermal[:3], same])
    ident = np.eye(3)
    ident[0, 2], ident[1, 2] = 1.5, -1.0
    T0 = np.stack([start, ident])
    r = U.estimate_shared_transform_ecc(gpu(both_o), gpu(both_t), T0, group, 'similarity', feature='intensity', reject_ratio=0.0)
    assert r.status[0] == U.ECC_LAMBDA and r.nit[0] == 0 and not r.success[0] and r.rho[0] < -0.5
    alone = U.estimate_shared_transform_ecc(gpu(optical[:3]), gpu(same), ident, None, 'similarity', feature='intensity',
                                            reject_ratio=0.0)
    assert alone.success[0] and alone.rho[0] > 0.99
    same_bits(r, alone, groups=[1], pairs=[3, 4, 5], other_groups=[0], other_pairs=[0, 1, 2])


@pytest.mark.parametrize('model', ('similarity', 'homography'))
def test_equal_bits(model):
    """A group has the same bits twice in a row, with one iteration or eight per enqueued chunk, and alone against in a batch
    of three groups, with and without masks."""
    optical, thermal, gid, truths, starts = PC.shift_groups()
    o, t = PC.planted_masks()
    for masks in ({}, {'thermal_mask': gpu(t), 'optical_mask': gpu(o)}):
        batch = U.estimate_shared_transform_ecc(gpu(optical), gpu(thermal), starts, gid, model, **masks)
        again = U.estimate_shared_transform_ecc(gpu(optical), gpu(thermal), starts, gid, model, **masks)
        one = U.estimate_shared_transform_ecc(gpu(optical), gpu(thermal), starts, gid, model, chunk=1, **masks)
        same_bits(batch, again)
        same_bits(batch, one)
        assert one.rounds <= batch.rounds and batch.rounds % 8 == 0
        for g in range(3):
            sel = np.nonzero(gid == g)[0]
            alone = U.estimate_shared_transform_ecc(gpu(optical[sel]), gpu(thermal[sel]), starts[g], None, model, **masks)
            same_bits(batch, alone, groups=[g], pairs=sel)


def test_rejection_round():
    optical, thermal = PC.recording('mispaired')
    r = U.estimate_shared_transform_ecc(gpu(optical), gpu(thermal), PC.start(7.0), None, 'homography', eps=PC.FIXTURE_EPS)
    first = r.first
    print('rho_i', np.round(first.rho_pair, 3), 'first %.3f after %.3f' % (PC.error(first.transform[0]), PC.error(r.transform[0])))
    assert first.rho_pair[PC.MISPAIRED] < 0.1 and np.delete(first.rho_pair, PC.MISPAIRED).min() > 0.9
    assert list(np.nonzero(r.rejected)[0]) == [PC.MISPAIRED] and not first.rejected.any()
    assert r.rounds > first.rounds and r.rounds % 8 == 0
    assert r.success[0] and r.n_included[0] == 5 and not r.included[PC.MISPAIRED] and np.isnan(r.rho_pair[PC.MISPAIRED])
    assert PC.error(r.transform[0]) <= PC.REJECTED_CAP and PC.error(r.transform[0]) < PC.error(first.transform[0])
    off = U.estimate_shared_transform_ecc(gpu(optical), gpu(thermal), PC.start(7.0), None, 'homography', eps=PC.FIXTURE_EPS,
                                          reject_ratio=0.0)
    assert off.first is None and not off.rejected.any()
    same_bits(off, first)


def test_masks_end_to_end():
    """The artefact recording: the static masks taken on the GPU are the planted sets, and with them the similarity is back under
    the cap; without them it is not."""
    optical, thermal = PC.recording('artefact')
    prob = U.SharedEccProblem(auto_mask=True)
    for at in (0, 2):
        prob.add(gpu(optical[at:at + (2 if at == 0 else 4)]), gpu(thermal[at:at + (2 if at == 0 else 4)]))
    prob.finish()
    o, t = PC.planted_masks()
    assert np.array_equal(prob.static[0][0].mask().cpu().numpy(), t) and np.array_equal(prob.static[0][1].mask().cpu().numpy(), o)
    tk, ok = PC.grown_masks()
    assert abs(prob.thermal_kept[0] - tk.mean()) < 1e-6 and abs(prob.optical_kept[0] - ok.mean()) < 1e-6
    r = prob.refine(PC.start(7.0), 'similarity', eps=PC.FIXTURE_EPS)
    given = U.estimate_shared_transform_ecc(gpu(optical), gpu(thermal), PC.start(7.0), None, 'similarity', eps=PC.FIXTURE_EPS,
                                            thermal_mask=gpu(t), optical_mask=gpu(o))
    same_bits(r, given)
    bare = U.estimate_shared_transform_ecc(gpu(optical), gpu(thermal), PC.start(7.0), None, 'similarity', eps=PC.FIXTURE_EPS)
    print('masked %.3f bare %.3f' % (PC.error(r.transform[0]), PC.error(bare.transform[0])))
    assert r.success[0] and PC.error(r.transform[0]) <= PC.MASKED_CAP['similarity']
    assert PC.error(bare.transform[0]) > 1.5
    rho, rho_pair, n = prob.correlation(r.transform)
    assert abs(rho[0] - r.rho[0]) < 1e-6 and np.abs(rho_pair - r.rho_pair).max() < 1e-6


def test_refusals():
    optical, thermal = PC.recording('clean')
    o, t = gpu(optical), gpu(thermal)
    T = PC.start(3.0)
    with pytest.raises(ValueError):
        U.estimate_shared_transform_ecc(o, t, np.stack([T, T]), [0, 0, 1, 1, 2, 2])          # a group index out of range
    with pytest.raises(ValueError):
        U.estimate_shared_transform_ecc(o, t, T, [0, 0, -1, 1, 1, 1])
    with pytest.raises(ValueError):
        U.estimate_shared_transform_ecc(o, t, T, [0, 0, 2, 2, 2, 2])                         # an empty group
    with pytest.raises(ValueError):
        U.estimate_shared_transform_ecc(o, t, np.stack([T] * 3), [0, 0, 1, 1, 1, 1])         # init_transforms of the wrong count
    with pytest.raises(ValueError):
        U.estimate_shared_transform_ecc(o, t, T, thermal_mask=gpu(np.ones((96, 128), np.uint8)))
    with pytest.raises(ValueError):
        U.estimate_shared_transform_ecc(o, t, T, [0, 0, 1, 1, 1, 1], optical_mask=gpu(np.ones((3, 96, 128), np.uint8)))
    with pytest.raises(ValueError):
        U.estimate_shared_transform_ecc(o, t, T, thermal_mask=gpu(np.ones((72, 96), np.float32)))
    for ratio in (-0.1, 1.5, float('nan')):
        with pytest.raises(ValueError):
            U.estimate_shared_transform_ecc(o, t, T, reject_ratio=ratio)
    with pytest.raises(ValueError):
        U.estimate_shared_transform_ecc(o, t, T, model='projective')
    with pytest.raises(ValueError):
        U.estimate_shared_transform_ecc(o, t, T, active=[True] * 5)
    with pytest.raises(ValueError):
        U.estimate_shared_transform_ecc(o, t[:5], T)
    with pytest.raises(ValueError):
        U.ecc_pooled_sums(o, t, [0, 0, 0, 1, 1, 3], np.stack([T, T]))
    with pytest.raises(ValueError):
        U.grow_mask(gpu(np.ones((16, 16), np.uint8)), -1)
    with pytest.raises(ValueError):
        U.grow_mask(gpu(np.ones((4, 16), np.uint8)), 1)
