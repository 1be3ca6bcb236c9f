"""GPU: the mutual-information alignment kernels (csrc/mutual_info.hip) and multipoint_amd.utils.alignment against the numpy
restatement tests/mi_restatement.py: exact histograms, the objective within 1e-9, bit-identity across batches and runs, the
device Nelder-Mead against the host one on the device objective, recovery of a known alignment, and the CLI flags."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import mi_restatement as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
# (source Ho, Wo, destination H, W)
SHAPES = [(40, 56, 40, 56), (48, 64, 48, 64), (48, 64, 40, 56)]
BINS = [16, 100, 256]          # 16: an LDS copy of the histogram per workgroup; 100, 256: global atomics


@pytest.fixture(scope='module')
def A():
    from multipoint_amd.utils import alignment
    return alignment


def _pairs(shape, seed=0, constant_thermal=False):
    """B = 2 pairs: structured optical frames (8-bit levels), thermal frames that depend on them"""
    Ho, Wo, H, W = shape
    opt = np.stack([np.round(R.blob_image(seed + b, Ho, Wo, 25) * 255) / 255 for b in range(2)]).astype(np.float32)
    rng = np.random.default_rng(seed + 10)
    th = np.stack([(1.0 - R.blob_image(seed + b, Ho, Wo, 25)[:H, :W]) ** 2 + 0.05 * rng.random((H, W))
                   for b in range(2)]).astype(np.float32)
    if constant_thermal:
        th = np.full_like(th, 0.375)
    return opt, th


def _histogram_transforms(W, H):
    return [np.eye(3),
            np.array([[1, 0, 0.37], [0, 1, -0.81], [0, 0, 1.0]]),                           # a fractional translation
            np.array([[0.8, 0.1, -6.0], [-0.12, 1.1, 4.0], [1e-3, -5e-4, 1.0]]),           # part of the frame outside: min = -1
            np.array([[1, 0, 1000.0], [0, 1, 1000.0], [0, 0, 1.0]]),                        # everything outside: min = max = -1
            np.zeros((3, 3))]                                                               # singular: every pixel reads (0, 0)


def _objective_transforms():
    return [np.eye(3),
            np.array([[1, 0, 0.37], [0, 1, -0.81], [0, 0, 1.0]]),
            np.array([[0.8, 0.1, -6.0], [-0.12, 1.1, 4.0], [1e-3, -5e-4, 1.0]]),
            np.array([[1.03, -0.02, 1.5], [0.015, 0.97, -0.7], [-2e-5, 3e-5, 1.0]])]


@pytest.mark.parametrize('constant_thermal', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_histograms_are_exact(A, shape, constant_thermal):
    Ho, Wo, H, W = shape
    opt, th = _pairs(shape, 0, constant_thermal)
    Ts = _histogram_transforms(W, H)
    pair, bins, T = [], [], []
    for b in range(2):
        for n in BINS:
            for t in Ts:
                pair.append(b); bins.append(n); T.append(t)
    o, t = torch.from_numpy(opt).to(DEV), torch.from_numpy(th).to(DEV)
    counts, minmax, warped = A.joint_histograms(o[:, None], t[:, None], pair, bins, np.stack(T), return_warped=True)
    minmax, warped = minmax.cpu().numpy(), warped.cpu().numpy()
    seen_border = seen_flat = False
    for e in range(len(pair)):
        w = R.warp_image(opt[pair[e]], T[e], H, W)
        assert np.array_equal(warped[e].view(np.uint32), w.view(np.uint32)), (e, 'warped frame')
        assert minmax[e, 0] == w.min() and minmax[e, 1] == w.max()
        want = R.joint_histogram(w.ravel(), th[pair[e]].ravel(), bins[e])
        got = counts[e].numpy()
        assert got.sum() == H * W
        assert np.array_equal(got, want), (e, bins[e])
        seen_border |= bool(w.min() == -1.0 and w.max() > -1.0)
        seen_flat |= bool(w.min() == w.max())
    assert seen_border and seen_flat
    # the two histogram strategies give the same counts
    sel = [e for e in range(len(pair)) if bins[e] == 16]
    for strategy in (1, 2):
        c2, _, _ = A.joint_histograms(o, t, [pair[e] for e in sel], [16] * len(sel), np.stack([T[e] for e in sel]),
                                      strategy=strategy)
        for e, c in zip(sel, c2):
            assert torch.equal(c, counts[e])


@pytest.fixture(scope='module')
def objective_inputs():
    shape = SHAPES[2]
    opt, th = _pairs(shape, 3)
    return shape, opt, th, torch.from_numpy(opt).to(DEV)[:, None], torch.from_numpy(th).to(DEV)[:, None]


@pytest.mark.parametrize('regularize', [False, True])
@pytest.mark.parametrize('sigma', [0, 1.5])
@pytest.mark.parametrize('normalized', [False, True])
def test_objective_against_the_restatement(A, objective_inputs, normalized, sigma, regularize):
    """|delta| <= 1e-9: the sums run in fp64 over at most 131072 terms of magnitude <= 0.37 with log within 1 ulp,
    4 * 131072 * 2^-53 * 6 = 3.5e-10."""
    shape, opt, th, o, t = objective_inputs
    Ts = np.stack(_objective_transforms())                       # E = 4
    init = np.stack([np.eye(3), np.array([[1.01, 0, 0.5], [0, 0.99, -0.5], [0, 0, 1.0]])])       # per pair
    worst = 0.0
    for n in BINS:
        got = A.negative_mutual_information_batch(o, t, np.stack([Ts, Ts]), n, init_transforms=init, regularize=regularize,
                                                  normalized_mi=normalized, smoothing_sigma=sigma).cpu().numpy()
        assert got.shape == (2, 4) and got.dtype == np.float64
        for b in range(2):
            for e in range(4):
                want = R.negative_mi(Ts[e], opt[b], th[b], init[b], n, regularize, normalized, sigma)
                worst = max(worst, abs(got[b, e] - want))
    print('largest |device - restatement| = %.3g' % worst)
    assert worst <= 1e-9


def test_bit_identity(A, objective_inputs):
    shape, opt, th, o, t = objective_inputs
    Ts = np.stack(_objective_transforms())
    for n, sigma, normalized in ((16, 0, True), (100, 1.5, False), (256, 0, True)):
        batch = A.negative_mutual_information_batch(o, t, np.stack([Ts, Ts]), n, normalized_mi=normalized, smoothing_sigma=sigma)
        again = A.negative_mutual_information_batch(o, t, np.stack([Ts, Ts]), n, normalized_mi=normalized, smoothing_sigma=sigma)
        assert torch.equal(batch, again)                         # a batch of 8, twice
        for b in range(2):
            for e in (0, 2):
                alone = A.negative_mutual_information_batch(o[b:b + 1], t[b:b + 1], Ts[e][None, None], n,
                                                           normalized_mi=normalized, smoothing_sigma=sigma)
                assert alone.item() == batch[b, e].item()
                one = A.calculate_negative_mutual_information(Ts[e].ravel(), o[b, 0], t[b, 0], np.eye(3), n,
                                                              normalized_mi=normalized, smoothing_sigma=sigma)
                assert one == batch[b, e].item()
        # mixed bin counts inside one launch change nothing either
        mixed = A.negative_mutual_information_batch(o, t, np.stack([Ts, Ts]), [n, 32, n, 64], normalized_mi=normalized,
                                                    smoothing_sigma=sigma)
        assert torch.equal(mixed[:, [0, 2]], batch[:, [0, 2]])
    # mutual_information_2d takes the samples as they are: the warped frame of the identity is the optical frame itself
    H, W = shape[2:]
    x, y = o[0, 0, :H, :W].contiguous(), t[0, 0]
    for n, sigma, normalized in ((100, 5, False), (16, 0, True)):
        mi = A.mutual_information_2d(x.reshape(-1), y.reshape(-1), sigma=sigma, bins=n, normalized=normalized)
        v = A.negative_mutual_information_batch(x[None, None], y[None, None], np.eye(3)[None, None], n, normalized_mi=normalized,
                                                smoothing_sigma=sigma)
        assert mi == -v.item()
        assert abs(mi - R.mutual_information_2d(x.cpu().numpy().ravel(), y.cpu().numpy().ravel(), sigma, n, normalized)) <= 1e-9
    w = A.warp_image(o[:, :, :H, :W].contiguous(), Ts[2], H, W)
    assert w.shape == (2, 1, H, W)
    assert np.array_equal(w[1, 0].cpu().numpy(), R.warp_image(opt[1][:H, :W], Ts[2], H, W))


def test_device_nelder_mead_is_the_host_one(A, objective_inputs):
    """The restatement's Nelder-Mead, calling the device objective one point at a time, against mp_mi_refine_*: bit for bit."""
    shape, opt, th, o, t = objective_inputs
    x0 = np.array([[1.02, 0.01, 1.2], [-0.01, 0.98, -0.9], [1e-5, 0.0, 1.0]])
    # (pair, bins, maxiter, maxfun, xatol, fatol): four plain problems, one that stops on the call limit, one that is finished
    # by its loose tolerances at the first check, next to the live ones
    base = [(0, 16, 60, 10 ** 6, 1e-6, 1e-6), (0, 100, 60, 10 ** 6, 1e-6, 1e-6), (1, 16, 60, 10 ** 6, 1e-6, 1e-6),
            (1, 100, 60, 10 ** 6, 1e-6, 1e-6), (0, 16, 10 ** 6, 23, 1e-6, 1e-6), (1, 100, 60, 10 ** 6, 10.0, 10.0),
            (1, 16, 10 ** 6, 7, 1e-6, 1e-6)]
    for regularize, normalized in ((False, True), (True, False)):
        # an eighth problem whose call limit falls inside a shrink (4 calls into the first shrink any of the first four
        # problems makes): the vertex that moved last keeps its old value
        problems, cut = list(base), None
        for b, n, maxiter, _, xatol, fatol in base[:4]:
            shrinks = []
            R.nelder_mead(lambda x: A.calculate_negative_mutual_information(x, o[b, 0], t[b, 0], x0, n, regularize=regularize,
                                                                            normalized_mi=normalized),
                          x0.ravel(), xatol=xatol, fatol=fatol, maxiter=maxiter, shrinks=shrinks)
            if shrinks:
                cut = (b, n, 10 ** 6, shrinks[0] + 4, xatol, fatol)
                break
        assert cut is not None, 'none of the problems shrinks within 60 iterations'
        problems.append(cut)
        dev = A.refine_alignment_batch(o, t, [p[0] for p in problems], [p[1] for p in problems], np.stack([x0] * len(problems)),
                                       regularize=regularize, normalized_mi=normalized, maxiter=[p[2] for p in problems],
                                       maxfun=[p[3] for p in problems], xatol=[p[4] for p in problems],
                                       fatol=[p[5] for p in problems], chunk=16)
        for q, (b, n, maxiter, maxfun, xatol, fatol) in enumerate(problems):
            def f(x):
                return A.calculate_negative_mutual_information(x, o[b, 0], t[b, 0], x0, n, regularize=regularize,
                                                               normalized_mi=normalized)
            host = R.nelder_mead(f, x0.ravel(), xatol=xatol, fatol=fatol, maxiter=maxiter, maxfun=maxfun)
            print(q, host['nit'], host['nfev'], host['success'], host['fun'])
            assert np.array_equal(dev['transform'][q].ravel(), host['x']), q
            assert dev['value'][q] == host['fun']
            assert (dev['nit'][q], dev['nfev'][q], bool(dev['success'][q])) == (host['nit'], host['nfev'], host['success']), q
        assert dev['nfev'][4] == 23 and not dev['success'][4] and dev['nfev'][6] == 7
        assert dev['nit'][5] == 1 and dev['nfev'][5] == 10 and dev['success'][5]
        assert not dev['success'][0] and dev['nit'][0] == 60
        assert dev['nfev'][7] == cut[3] and not dev['success'][7]


def test_refusals(A, objective_inputs):
    shape, opt, th, o, t = objective_inputs
    eye = np.eye(3)[None]
    for bins in (0, 257):
        with pytest.raises(ValueError, match='bins'):
            A.joint_histograms(o, t, [0], [bins], eye)
        with pytest.raises(ValueError, match='bins'):
            A.refine_alignment_batch(o, t, [0], [bins], eye)
    with pytest.raises(ValueError, match='pair'):
        A.joint_histograms(o, t, [2], [16], eye)
    with pytest.raises(ValueError, match='sigma'):
        A.calculate_negative_mutual_information(np.eye(3), o[0, 0], t[0, 0], np.eye(3), 16, smoothing_sigma=40)
    with pytest.raises(ValueError, match='LDS'):
        A.joint_histograms(o, t, [0], [100], eye, strategy=1)
    import ctypes
    from multipoint_amd import _lib
    h = _lib.get_handle(torch.device(DEV))
    ws = torch.empty(1024, dtype=torch.uint8, device=DEV)
    Td = torch.eye(3, dtype=torch.float64, device=DEV).reshape(1, 9)
    out = torch.empty(1, dtype=torch.float64, device=DEV)
    one, sixteen = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(16)
    H, W = shape[2:]
    args = lambda optical, ws_, nbytes: (h.ptr, optical, shape[0], shape[1], _lib.ptr(t), H, W, 2, one, sixteen, _lib.ptr(Td), 1, 0.0,
                                         0, None, _lib.ptr(out), ws_, nbytes, None)
    assert h.lib.mp_mi_objective(*args(_lib.ptr(o), _lib.ptr(ws), 1024)) == -1          # a workspace that is too small
    assert b'workspace' in h.lib.mp_last_error(h.ptr)
    assert h.lib.mp_mi_objective(*args(None, _lib.ptr(ws), 1024)) == -1                 # a NULL tensor
    assert h.lib.mp_mi_objective(*args(_lib.ptr(o), None, 1 << 30)) == -1
    live = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert h.lib.mp_mi_refine_step(h.ptr, _lib.ptr(ws), 1, _lib.ptr(live), None) == -3   # no refinement begun in that workspace
    need = _lib.c_ll()
    assert h.lib.mp_mi_workspace_bytes(1, 1, 1, 0, 64, 16, 0, ctypes.byref(need)) == -1
    assert h.lib.mp_mi_workspace_bytes(1, 1, 1, 48, 64, 300, 0, ctypes.byref(need)) == -1


def test_recovery(A):
    """A known alignment is recovered from a start about 2 px off, in the reference's direction (thermal -> optical).
    The restatement under scipy's Nelder-Mead on the CPU (bins 16 / 32 / 64, normalised, ranking 'sum'): four-corner error
    2.356 px at the start, 0.146 px (a sixteenth) for the candidate align_images' ranking picks, the 32-bin one; the 16- and 64-bin
    runs end at 0.911 and 0.942 px.  The device run is asked for less
    than half the initial error: trajectories are chaotic and need not match the CPU's.  With the direction flipped (the
    inverse handed in and out) the error would be several times the initial one."""
    opt, th, T_true, T_init = R.recovery_pair()
    H, W = th.shape
    o, t = torch.from_numpy(opt).to(DEV), torch.from_numpy(th).to(DEV)
    params = {'alignment/bin_sizes': [16, 32, 64], 'alignment/normalized_mi': True, 'alignment/smoothing_sigma': 0,
              'alignment/check/both/max_diff_mi': 0.5, 'alignment/accept_init': False, 'alignment/ranking_method': 'sum'}
    T, kind, cands = A.align_images(o, t, T_init, params)
    e0, e1 = R.corner_error(T_init, T_true, H, W), R.corner_error(T, T_true, H, W)
    print('four-corner error: initial %.3f px, %s %.3f px; candidates %s' % (
        e0, kind, e1, [(c['type'], round(R.corner_error(c['transform'], T_true, H, W), 3), c['nit']) for c in cands]))
    assert re.fullmatch(r'bin(16|32|64)_normalized_s0', kind)
    assert e1 < 0.5 * e0
    for c in cands:
        assert c['value'] <= c['init_value']                      # at the bin size it was optimised for
        n = int(re.match(r'bin(\d+)_', c['type']).group(1))
        assert c['value'] == A.calculate_negative_mutual_information(c['transform'], o, t, T_init, n, normalized_mi=True)
    # the batched form returns the same for each pair of a batch of two
    T2, kind2, _ = A.align_images(torch.stack([o, o])[:, None], torch.stack([t, t])[:, None], T_init, params)
    assert kind2 == [kind, kind] and np.array_equal(T2[0], T) and np.array_equal(T2[1], T)
    # accept_init puts the start among the candidates
    _, _, c3 = A.align_images(o, t, T_init, dict(params, **{'alignment/accept_init': True, 'alignment/ranking_method': 'order'}))
    assert c3[0]['type'] == 'init' and np.array_equal(c3[0]['transform'], T_init) and len(c3) == len(cands) + 1


def test_cli_estimate_direction(A):
    """The CLI's estimate maps optical pixels to thermal ones (its aligned image is cv2.warpPerspective(optical, H_est)); the
    transform of utils.alignment maps thermal pixels to optical ones.  estimate_to_transform must turn one into the other: the
    MI warp under it is the CLI's aligned image, and a pair that is exactly aligned by H_est scores best under it."""
    sys.path.insert(0, ROOT)
    import predict_align_image_pair as cli
    from multipoint_amd.datasets.augmentation import warp_perspective_cv
    opt = R.blob_image(21, 48, 64, 40, 2.0, 6.0)
    o = torch.from_numpy(opt).to(DEV)[None, None]
    H_est = np.array([[1.0, 0.0, 5.0], [0.0, 1.0, -3.0], [0.0, 0.0, 1.0]])        # optical (x, y) -> thermal (x + 5, y - 3)
    aligned = warp_perspective_cv(o, H_est[None], border_reflect=False)[0, 0].cpu().numpy()
    assert np.array_equal(aligned[0:40, 10:60], opt[3:43, 5:55])                 # thermal (x, y) shows optical (x - 5, y + 3)
    T = cli.estimate_to_transform(H_est)
    assert np.allclose(T, [[1, 0, -5], [0, 1, 3], [0, 0, 1]])
    w = A.warp_image(o, T, 48, 64)[0, 0].cpu().numpy()
    inside = w != -1.0
    assert inside.mean() > 0.8 and np.array_equal(w[inside], aligned[inside])
    # thermal = a non-monotone map of the aligned image: the estimate's transform scores better than the identity and than
    # the estimate taken the wrong way round
    th = torch.from_numpy((4.0 * (aligned.astype(np.float64) - 0.45) ** 2).astype(np.float32)).to(DEV)
    v = [A.calculate_negative_mutual_information(M, o[0, 0], th, np.eye(3), 100, normalized_mi=True)
         for M in (T, np.eye(3), H_est)]
    print('negative normalised MI: transform %.4f, identity %.4f, flipped %.4f' % tuple(v))
    assert v[0] < v[1] and v[0] < v[2]
    assert np.allclose(cli.estimate_to_transform(T), H_est)                       # what --mi-refine prints is turned back
    assert np.array_equal(cli.estimate_to_transform(np.zeros((3, 3))), np.eye(3))


def test_cli_mi(tmp_path):
    d = tmp_path / 'multipoint'
    d.mkdir()
    with open(os.path.join(ROOT, 'model_weights', 'multipoint', 'params.yaml')) as f:
        (d / 'params.yaml').write_text(f.read())
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'config_image_pair_dataset_prediction.yaml')))
    cfg['dataset'].update({'num_samples': 2, 'height': 120, 'width': 160})
    cfg['dataset']['augmentation']['homographic']['enable'] = False
    cfg['prediction'].update({'topk': 300, 'batchsize': 1, 'num_worker': 0,
                              'mi_alignment': {'alignment/bin_sizes': [16, 32], 'alignment/ranking_method': 'sum'}})
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    base = [sys.executable, os.path.join(ROOT, 'predict_align_image_pair.py'), '-y', str(tmp_path / 'cfg.yaml'), '-m', str(d),
            '-v', 'none']
    runs = [subprocess.Popen(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
            for extra in (['-p'], ['--mi', '--mi-refine'])]
    (plain, perr), (mi, merr) = [r.communicate() for r in runs]
    assert runs[0].returncode == 0, perr[-2000:]
    assert runs[1].returncode == 0, merr[-2000:]
    num = r'-?\d+\.\d+'
    lines = mi.split('\n')
    report = [l for l in lines if l.startswith('Negative normalised MI')]
    assert len(report) == 1 and re.fullmatch(r'Negative normalised MI \(100 bins\): identity %s, estimated %s' % (num, num), report[0])
    refined = [i for i, l in enumerate(lines) if l.startswith('MI alignment:')]
    assert len(refined) == 1
    print(report[0]); print(lines[refined[0]])
    m = re.fullmatch(r'MI alignment: (init|bin(16|32)_normalized_s0) negative normalised MI \(100 bins\) (%s)' % num, lines[refined[0]])
    assert m, lines[refined[0]]
    assert lines[refined[0] + 1] == 'MI-aligned Homography:'
    matrix = np.array([[float(v) for v in l.strip(' []').split()] for l in lines[refined[0] + 2:refined[0] + 5]])
    assert matrix.shape == (3, 3) and np.all(np.isfinite(matrix))
    # the flags add lines only
    assert 'MI' not in plain

    def stable(text):
        return [l for l in text.split('\n') if not re.search(r'took:|Box nms:', l)]
    new = set(range(refined[0], refined[0] + 5)) | {lines.index(report[0])}
    assert stable('\n'.join(l for i, l in enumerate(lines) if i not in new)) == stable(plain)
