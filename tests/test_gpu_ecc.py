"""GPU: csrc/ecc.hip and multipoint_amd.utils.ecc against the float64 restatement (tests/ecc_restatement.py) -- the feature
frames, the valid count, every sum, the solve step, whole trajectories, the stop and failure rules, and the bits."""
import numpy as np
import pytest
import torch

import ecc_cases as C
import ecc_restatement as E
from multipoint_amd.utils import ecc as U

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U24 = 2.0 ** -24
MODELS = ('translation', 'similarity', 'affine', 'homography')
# (template, image): the smallest frames, odd sizes, the planted pairs' sizes, exactly one pixel chunk of 4096, a chunk plus one
SHAPES = (((8, 8), (9, 13)), ((30, 40), (33, 47)), ((72, 96), (96, 128)), ((64, 64), (70, 75)), ((17, 241), (25, 250)))


def frames(seed, B, hw):
    """Smooth random frames in [0, 1]: a blurred noise field, float32 (B, H, W)."""
    rng = np.random.default_rng(seed)
    H, W = hw
    x = rng.random((B, H + 4, W + 4))
    x = sum(x[:, i:i + H, j:j + W] for i in range(5) for j in range(5)) / 25.0
    x = (x - x.min()) / (x.max() - x.min())
    return x.astype(np.float32)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize('B', (1, 3))
@pytest.mark.parametrize('shape', [s for pair in SHAPES for s in pair])
def test_features(shape, B):
    """The blur is bit-exact float32 (pyramid_restatement); behind it gx, gy are one exact float32 subtraction and halving each,
    then gy * gy, one fused multiply-add and one square root, each rounded once: the radicand carries 2 * 2^-24, the root half
    of it plus its own rounding -- 2 * 2^-24 of the value."""
    x = frames(11, B, shape)
    for ksize in (1, 5):
        feat, packed = U.ecc_features(gpu(x), 'gradient', ksize, packed=True)
        feat, packed = feat.cpu().numpy(), packed.cpu().numpy()
        inten = U.ecc_features(gpu(x), 'intensity', ksize).cpu().numpy()
        for b in range(B):
            ref = E.features(x[b], ksize, 'gradient')
            assert np.all(np.abs(feat[b].astype(np.float64) - ref) <= 2 * U24 * ref + 1e-30), (shape, ksize, b)
            for c in ((0, 0), (0, -1), (-1, 0), (-1, -1)):                                # both differences vanish in the corners
                assert feat[b][c] == 0
            assert not packed[b][:, (0, -1), 1].any() and not packed[b][(0, -1), :, 2].any()    # gx, gy on their border lines
            assert np.array_equal(inten[b].view(np.uint32), E.features(x[b], ksize, 'intensity', f32=True).view(np.uint32))
            gx, gy = E.central(feat[b])
            want = np.stack([feat[b], gx, gy, np.zeros_like(gx)], axis=-1)
            assert np.array_equal(packed[b].view(np.uint32), want.view(np.uint32))


def transforms_for(thw, ihw):
    """Transforms of one shape pair, by what they do: every pixel valid, part of the template outside, none valid, a tap exactly
    on the last column (and row), a perspective one."""
    (H, W), (Ho, Wo) = thw, ihw
    inside = np.array([[(Wo - 1.5) / (W - 1), 0.0, 0.25], [0.0, (Ho - 1.5) / (H - 1), 0.125], [0.0, 0.0, 1.0]])
    partly = np.array([[0.98, -0.12, 0.3 * W], [0.12, 0.98, -0.2 * H], [0.0, 0.0, 1.0]])
    none = np.array([[1.0, 0.0, 3.0 * Wo], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    last = np.array([[1.0, 0.0, float(Wo - W)], [0.0, 1.0, float(Ho - H)], [0.0, 0.0, 1.0]])
    persp = np.array([[0.9, 0.05, 0.5], [-0.04, 0.92, 0.8], [1e-3 / W, -2e-3 / H, 1.0]])
    return {'inside': inside, 'partly': partly, 'none': none, 'last': last, 'persp': persp}


# Rounding steps between exact taps and a term, in units of 2^-24 of the term's magnitude (the largest |tap| in place of the
# sample): a bilinear sample is two horizontal lerps (difference 2, fma 1: 3) and a vertical one (the difference of two such
# values 2, fma 1) -- 6; a Jacobian column of the homography adds the reciprocal, the product with it, -(a xs + c ys) in a
# product and an fma, and the product with x or y -- 11 at most; the products of two terms are exact in float64, so a sum of
# G_k G_l carries 22 and second-order terms, rounded up to 24.  The float64 additions (at most 2^24 terms) add 2^-29.
C_TERMS = 24
SUM_SLACK = C_TERMS * U24 + 2.0 ** -29


@pytest.mark.parametrize('B', (1, 3))
@pytest.mark.parametrize('shapes', SHAPES)
def test_sums(shapes, B):
    thw, ihw = shapes
    opt, th = frames(21, B, ihw), frames(22, B, thw)
    kinds = transforms_for(thw, ihw)
    names = sorted(kinds)
    pair = [(i + j) % B for j in range(2) for i in range(len(names))]            # several problems per pair
    Ts = np.stack([kinds[n] for _ in range(2) for n in names])
    _, packed = U.ecc_features(gpu(opt), 'gradient', 5, packed=True)
    packed = packed.cpu().numpy().astype(np.float64)
    template = U.ecc_features(gpu(th), 'gradient', 5).cpu().numpy().astype(np.float64)
    for model in MODELS:
        got = U.ecc_sums(gpu(opt), gpu(th), pair, Ts, model)
        assert got.shape == (len(pair), U.ecc_sum_count(model))
        for q, b in enumerate(pair):
            kind = names[q % len(names)]
            planes = (packed[b, :, :, 0], packed[b, :, :, 1], packed[b, :, :, 2])
            ref, mag = E.sums(planes, template[b], Ts[q], model, magnitudes=True)
            assert got[q, 0] == ref[0], (model, kind, 'valid count')
            if kind == 'inside':
                assert got[q, 0] == thw[0] * thw[1]
            if kind == 'none':
                assert not got[q].any()
            if kind == 'last':                                 # the last template column and row tap the image's last lines
                assert got[q, 0] == (thw[0] - 1) * (thw[1] - 1)
            if kind == 'partly':
                assert 0 < got[q, 0] < thw[0] * thw[1]
            bad = np.abs(got[q] - ref) > SUM_SLACK * mag
            assert not bad.any(), (model, kind, np.nonzero(bad)[0], (np.abs(got[q] - ref) / np.maximum(mag, 1e-300)).max() / U24)
    rho, n = U.ecc_correlation(gpu(opt), gpu(th), pair, Ts)
    assert np.array_equal(n, got[:, 0].astype(np.int64))
    assert np.isnan(rho[names.index('none')]) and np.all(np.abs(rho[np.isfinite(rho)]) <= 1.0)


@pytest.mark.parametrize('model', MODELS)
def test_solve_step(model):
    """One update on the GPU's own sums against numpy.  Both sides run the same float64 formulas; they differ in the order and
    fusing of operations, 2^-53 relative per operation.  The update is Hs^-1 v with v = lambda tp - ip: a perturbation of v by
    2^-53 of its terms' magnitudes V moves it by at most |Hs^-1| V, the factorisation by K cond(Hs) 2^-53 |dp|; lambda itself
    comes from differences of the same kind.  The bound is 1000 * 2^-53 * cond(Hs) * (|dp| + |Hs^-1| V)."""
    name = 'small_thermal_far'
    optical, thermal, _ = C.pair(name)
    T0 = E.start_transform(C.start(name, 'near'), model)
    K = E.PARAMS[model]
    s = U.ecc_sums(gpu(optical), gpu(thermal), [0], T0[None], model)[0]
    status, Tn, rho, _ = E.solve(s, T0, model, thermal.size, eps=0.0)
    assert status is None
    r = U.refine_alignment_ecc_batch(gpu(optical), gpu(thermal), [0], T0[None], model, eps=0.0, maxiter=1, chunk=1)
    assert r['nit'][0] == 1 and r['success'][0] and not r['converged'][0] and r['rounds'] == 1
    assert abs(r['rho'][0] - rho) <= 1e-12
    n, (Sw, Sr, _, _, _), SG, A, SGw, SGr = E.unpack(s, K)
    dp = E.parameters(Tn, model) - E.parameters(T0, model)
    lam = 1.0 if rho == 0 else abs(1.0 / rho)                        # lambda is about 1 / rho near the optimum
    V = np.abs(SGw) + abs(Sw / n) * np.abs(SG) + 4.0 * lam * (np.abs(SGr) + abs(Sr / n) * np.abs(SG))
    bound = 1000.0 * 2.0 ** -53 * np.linalg.cond(A) * (np.abs(dp).max() + (np.abs(np.linalg.inv(A)) @ V).max())
    diff = np.abs(E.parameters(r['transform'][0], model) - E.parameters(Tn, model)).max()
    print(model, 'cond', np.linalg.cond(A), 'diff', diff, 'bound', bound)
    assert diff <= bound


@pytest.mark.parametrize('maxiter', (1, 3, 10))
@pytest.mark.parametrize('model', ('similarity', 'homography'))
def test_trajectories(model, maxiter):
    """eps = 0: exactly maxiter updates.  The GPU's iterate lies within 4 x the restatement's own float32-against-float64
    difference of the float64 restatement's."""
    worst = 0.0
    for name in C.FIXTURES:
        optical, thermal, _ = C.pair(name)
        want = C.restated(name, 'near', model, maxiter, 0.0)
        floor = C.noise_floor(name, 'near', model, maxiter)
        r = U.refine_alignment_ecc_batch(gpu(optical), gpu(thermal), [0], C.start(name, 'near')[None], model, eps=0.0,
                                         maxiter=maxiter)
        assert r['nit'][0] == want['nit'] == maxiter and r['status'][0] == U.ECC_OK and not r['converged'][0]
        d = C.corner_distance(r['transform'][0], want['transform'], thermal.shape)
        print(name, model, maxiter, 'gpu %.3e floor %.3e' % (d, floor))
        worst = max(worst, d / floor)
        assert d <= 4.0 * floor, (name, d, floor)
    print('worst ratio', worst)


@pytest.mark.parametrize('model', ('similarity', 'affine', 'homography'))
def test_eps_stop(model):
    """|rho - rho_prev| < 1e-6: the error of the similarity within the host test's cap, the iteration count within one of the
    restatement's.  Problems of equal thermal size run as one batch, two starts per pair."""
    for hw in ((96, 128), (72, 96)):
        names = [n for n in C.FIXTURES if C.pair(n)[1].shape == hw]
        optical = np.stack([C.pair(n)[0] for n in names])
        thermal = np.stack([C.pair(n)[1] for n in names])
        pair = [i for i in range(len(names)) for _ in ('near', 'far')]
        T0 = np.stack([C.start(n, level) for n in names for level in ('near', 'far')])
        r = U.refine_alignment_ecc_batch(gpu(optical), gpu(thermal), pair, T0, model)
        assert r['rounds'] % 8 == 0
        for q, (n, level) in enumerate((n, level) for n in names for level in ('near', 'far')):
            want = C.restated(n, level, model, 50, 1e-6)
            assert r['success'][q] and r['converged'][q] and r['status'][q] == U.ECC_OK
            err = C.error(r['transform'][q], n)
            print(n, level, model, 'error %.3f nit %d (restatement %.3f, %d)' % (err, r['nit'][q], C.error(want['transform'], n),
                                                                                 want['nit']))
            if model == 'similarity':
                assert err <= C.SIMILARITY_CAP
            assert abs(int(r['nit'][q]) - want['nit']) <= 1
            assert abs(r['rho'][q] - want['rho']) < 1e-4


def test_failure_statuses():
    name = 'small_thermal_far'
    optical, thermal, T = C.pair(name)
    o, t = gpu(optical), gpu(thermal)
    start = C.start(name, 'near')
    # fewer valid pixels than min_valid H W: the template pushed out of the image; and with a min_valid nothing can meet
    far = start.copy()
    far[0, 2] += 500.0
    r = U.refine_alignment_ecc_batch(o, t, [0, 0], np.stack([far, start]), 'similarity')
    assert r['status'][0] == U.ECC_FEW_VALID and not r['success'][0] and r['nit'][0] == 0
    assert np.array_equal(r['transform'][0], E.start_transform(far, 'similarity'))
    assert r['status'][1] == U.ECC_OK and r['success'][1]                         # its neighbour in the batch goes on
    r = U.refine_alignment_ecc_batch(o, t, [0], start[None], 'similarity', min_valid=1.0)
    assert r['status'][0] == U.ECC_FEW_VALID
    # lambda's denominator <= 0: raw intensities of a contrast-inverted pair, at iteration 0
    r = U.refine_alignment_ecc_batch(o, t, [0], start[None], 'similarity', feature='intensity')
    assert r['status'][0] == U.ECC_LAMBDA and r['nit'][0] == 0 and not r['success'][0] and r['rho'][0] < -0.9
    # G^T G not positive definite: an image without any horizontal gradient under a translation
    ramp = np.repeat(np.linspace(0.0, 1.0, 40, dtype=np.float32)[:, None] ** 2, 48, axis=1)
    tmpl = np.ascontiguousarray(ramp[4:36, 6:38]) + 0.01 * frames(5, 1, (32, 32))[0]
    T0 = np.array([[1.0, 0.0, 6.3], [0.0, 1.0, 4.4], [0.0, 0.0, 1.0]])
    r = U.refine_alignment_ecc_batch(gpu(ramp), gpu(tmpl), [0], T0[None], 'translation', feature='intensity', ksize=1)
    assert r['status'][0] == U.ECC_NOT_POSITIVE and not r['success'][0] and r['rho'][0] > 0.9
    # a non-finite value: a constant image has no variance, rho is 0 / 0
    flat = np.full((40, 48), 0.5, np.float32)
    r = U.refine_alignment_ecc_batch(gpu(flat), gpu(tmpl), [0], T0[None], 'translation', feature='intensity', ksize=1)
    assert r['status'][0] == U.ECC_NONFINITE and not r['success'][0] and np.isnan(r['rho'][0])
    # maxiter is no failure
    r = U.refine_alignment_ecc_batch(o, t, [0], start[None], 'similarity', eps=0.0, maxiter=2)
    assert r['success'][0] and not r['converged'][0] and r['nit'][0] == 2 and r['rounds'] == 8


def test_refusals():
    x = gpu(frames(1, 1, (16, 16)))
    with pytest.raises(ValueError):
        U.ecc_features(gpu(frames(1, 1, (7, 16))))
    with pytest.raises(ValueError):
        U.ecc_features(x, 'gradient', 4)
    with pytest.raises(ValueError):
        U.ecc_features(x, 'edges')
    with pytest.raises(ValueError):
        U.refine_alignment_ecc_batch(x, x, [0], np.eye(3)[None], 'projective')
    with pytest.raises(ValueError):
        U.refine_alignment_ecc_batch(x, x, [1], np.eye(3)[None])                   # pair index outside the batch
    with pytest.raises(ValueError):
        U.refine_alignment_ecc_batch(x, x, [0] * 4097, np.tile(np.eye(3), (4097, 1, 1)))
    with pytest.raises(ValueError):
        U.refine_alignment_ecc_batch(x, x, [0], np.eye(3)[None], maxiter=0)
    with pytest.raises(ValueError):
        U.refine_alignment_ecc_batch(x, x, [0], np.eye(3)[None], eps=-1.0)
    bad = np.eye(3)
    bad[2, 2] = 0.0
    with pytest.raises(ValueError):
        U.refine_alignment_ecc_batch(x, x, [0], bad[None], 'similarity')


@pytest.mark.parametrize('model', ('similarity', 'homography'))
def test_equal_bits(model):
    """A problem has the same bits alone, inside a batch with other pairs and starts, with one iteration or eight per enqueued
    chunk, and twice in a row."""
    names = [n for n in C.NAMES if C.pair(n)[1].shape == (72, 96)]
    optical = np.stack([C.pair(n)[0] for n in names])
    thermal = np.stack([C.pair(n)[1] for n in names])
    pair = [0, 1, 2, 1, 0]
    T0 = np.stack([C.start(names[b], 'near' if q < 3 else 'far') for q, b in enumerate(pair)])
    o, t = gpu(optical), gpu(thermal)
    batch = U.refine_alignment_ecc_batch(o, t, pair, T0, model)
    again = U.refine_alignment_ecc_batch(o, t, pair, T0, model)
    one = U.refine_alignment_ecc_batch(o, t, pair, T0, model, chunk=1)
    keys = ('transform', 'rho', 'nit', 'status', 'converged')
    for k in keys:
        assert np.array_equal(batch[k], again[k]) and np.array_equal(batch[k], one[k]), k
    assert one['rounds'] <= batch['rounds']
    for q, b in enumerate(pair):
        alone = U.refine_alignment_ecc_batch(gpu(optical[b]), gpu(thermal[b]), [0], T0[q][None], model)
        for k in keys:
            assert np.array_equal(alone[k][0], batch[k][q]), (k, q)
    s = U.ecc_sums(o, t, pair, T0, model)
    for q, b in enumerate(pair):
        assert np.array_equal(U.ecc_sums(gpu(optical[b]), gpu(thermal[b]), [0], T0[q][None], model)[0], s[q])
