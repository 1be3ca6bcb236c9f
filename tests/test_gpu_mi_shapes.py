"""GPU: the mutual-information kernels (csrc/mutual_info.hip, csrc/align_api.hip) on every frame shape, bin count and bin
edge at which they take another path, against the numpy restatement tests/mi_restatement.py.  tests/mi_shape_cases.py builds
the inputs and the restatement's answers (once per process); tests/test_mi_shapes_host.py checks their premises on the CPU.

What each test reaches that tests/test_gpu_mi.py does not:

  test_frames[0]  9x250 -> 5x230     bh0 = H < 16 (so bw0 = 1024 // 5 = 204 < W): warp_kernel's block start xb = 204 for 26
                                     pixels; four x-blocks of the warp grid, a partial row block (H % 4 = 1)
  test_frames[1]  45x150 -> 37x131   bw0 = 64 < W: xb = 0 / 64 / 128, the last block 3 pixels wide; H % 4 = 1
  test_frames[2]  20x70 -> 16x65     bw0 = 64 < W with a one-pixel last block
  test_frames[3]  3x80 -> 1x70       bh0 = 1: a single row, three of four rows of every warp workgroup idle
  test_frames[4]  80x3 -> 70x1       a single column: 63 of 64 lanes idle in the min / max fold
  test_frames[5]  2x2 -> 1x1         one sample: a == b on the thermal axis as well (make_axis' +-0.5 rule in
                                     thermal_map_kernel), one wave with a single live lane
  test_frames[6]  300x500 -> 264x512 135168 pixels: launch_mi_thermal's cap at 64 workgroups and a second trip of the
                                     grid-stride loops of minmax_kernel and thermal_map_kernel; 66 hist_kernel workgroups,
                                     8 x-blocks of the warp grid
                  all of them        B = 3 with the pairs listed as 2, 0, 1, 0 (a thermal-map slot used twice, slots in another
                                     order than the pairs); 65 bins next to 16 (global atomics next to LDS copies); a transform
                                     for which the split sum X0 + h[0] * (x - xb) and the unsplit one round to different
                                     1/32 px coordinates
  test_bin_counts                    one packed launch over 1 .. 256 bins, in both orders: hist_kernel's LDS / global
                                     boundary at 64 / 65 with the full 32 KiB of dynamic LDS, strategy 1 at 64; zero_kernel
                                     on histograms of 2 to 131072 counters at packed offsets
  test_samples_on_the_edges          bin_of's walk with samples that ARE an edge or a float32 next to one, on both axes,
                                     in hist_kernel (both strategies) and thermal_map_kernel
  test_objective[sigma]              partial_kernel with fewer row blocks than MI_PARTS (n < 16: whole workgroups return
                                     early; 17, 33) and a partial last block (17, 31, 63, 127, 255), final_kernel's nb for
                                     them; smooth_kernel at radius 0 (sigma 0.1), at radius 20 (sigma 5: larger than the
                                     histograms up to 16 x 32, every outer tap clipped) and at MI_MAX_RADIUS = 64 (sigma 16:
                                     129 weights)
  test_mixed_launch[sigma]           small histograms inside the 2 * 256^2 stride of a launch whose largest is 256 bins,
                                     LDS copies of 64 bins (32 KiB) next to global-atomic evaluations, every entry compared
  test_nelder_mead_beyond_one_workgroup   70 problems: a second workgroup of nm_begin / nm_decide / nm_result, 700
                                     evaluations on the grid's z axis (warp) and y axis (the others), chunk 1, 7 and 16
  test_limits                        bins 1 and 256, radius 64 from sigma 16.1, the refusal of radius 65
"""
import numpy as np
import pytest
import torch

import mi_restatement as R
import mi_shape_cases as C

pytestmark = pytest.mark.gpu
DEV = 'cuda'
BOUND = 1e-9          # tests/test_gpu_mi.py::test_objective_against_the_restatement derives it for every n <= 256


@pytest.fixture(scope='module')
def A():
    from multipoint_amd.utils import alignment
    return alignment


def _device(case):
    return torch.from_numpy(case['optical']).to(DEV), torch.from_numpy(case['thermal']).to(DEV)


def _histograms_equal(A, case, ref, order=None, check_warp=True):
    """one joint_histograms launch of the case's evaluations (in `order`) against the restatement; returns the counts per
    evaluation of the case"""
    o, t = _device(case)
    H, W = case['thermal'].shape[1:]
    order = list(range(len(case['pair']))) if order is None else list(order)
    counts, minmax, warped = A.joint_histograms(o, t, [case['pair'][e] for e in order], [case['bins'][e] for e in order],
                                                case['transforms'][order], return_warped=True)
    minmax, warped = minmax.cpu().numpy(), warped.cpu().numpy()
    out = {}
    for j, e in enumerate(order):
        w, want = ref[e]
        if check_warp:
            assert np.array_equal(warped[j].view(np.uint32), w.view(np.uint32)), (e, 'warped frame')
        assert minmax[j, 0] == w.min() and minmax[j, 1] == w.max(), (e, 'min / max')
        got = counts[j].numpy()
        assert got.shape == want.shape and got.sum() == H * W, e
        assert np.array_equal(got, want), (e, case['bins'][e], 'differing counters: %d' % (got != want).sum())
        out[e] = counts[j]
    return out


def _strategies_agree(A, case, counts, strategies=(1, 2)):
    o, t = _device(case)
    for strategy in strategies:
        sel = [e for e in range(len(case['pair'])) if strategy == 2 or case['bins'][e] <= 64]
        assert sel
        c2, _, _ = A.joint_histograms(o, t, [case['pair'][e] for e in sel], [case['bins'][e] for e in sel],
                                      case['transforms'][sel], strategy=strategy)
        for e, c in zip(sel, c2):
            assert torch.equal(c, counts[e]), (strategy, e, case['bins'][e])


# ---- 1. frames ----
@pytest.mark.parametrize('i', range(len(C.FRAMES)))
def test_frames(A, i):
    """warped bits, min / max and counts of every evaluation of a frame; strategies 1 and 2 give strategy 0's counts"""
    case = C.frame_case(i)
    counts = _histograms_equal(A, case, C.frame_reference(i))
    _strategies_agree(A, case, counts)


# ---- 2. bin counts ----
def test_bin_counts(A):
    case, ref = C.bins_case(), C.bins_reference()
    E = len(case['pair'])
    counts = _histograms_equal(A, case, ref)
    _histograms_equal(A, case, ref, order=range(E - 1, -1, -1))             # other packed offsets
    _strategies_agree(A, case, counts, strategies=(1,))


# ---- 3. samples on the edges ----
def test_samples_on_the_edges(A):
    """the identity copies the frames (checked bit for bit), so every sample that is an edge reaches bin_of as that edge"""
    case = C.edge_case()
    counts = _histograms_equal(A, case, C.edge_reference())
    _strategies_agree(A, case, counts)


# ---- 4. the objective ----
def _objective(A, case, o, t, normalized, regularize, sigma):
    return A.negative_mutual_information_batch(o, t, case['transforms'], case['bins'], init_transforms=case['init'],
                                               regularize=regularize, normalized_mi=normalized, smoothing_sigma=sigma)


@pytest.mark.parametrize('sigma', C.SIGMAS)
def test_objective(A, sigma):
    """|device - restatement| <= 1e-9 at every bin count of C.BIN_COUNTS, not normalised with the regulariser and normalised
    without it.  The bound is that of tests/test_gpu_mi.py (fp64 sums over at most 131072 terms); the smoothing adds at most
    129 + 129 products per entry, summed in the restatement's order.
    Measured on an MI355X, largest |difference| (not normalised / normalised): sigma 0 and 0.1: 1.95e-14 / 2.66e-15,
    0.6: 9.77e-15 / 1.11e-15, 5: 5.33e-15 / 1.11e-15, 16: 3.55e-15 / 4.44e-16; the largest ones at 255 and 256 bins."""
    case, ref = C.objective_case(), C.objective_reference(sigma)
    o, t = _device(case)
    worst = 0.0
    for normalized, regularize in ((False, True), (True, False)):
        got = _objective(A, case, o, t, normalized, regularize, sigma).cpu().numpy()
        assert got.shape == (2, len(case['bins'])) and got.dtype == np.float64
        d = np.abs(got - ref[normalized, regularize])
        b, i = np.unravel_index(np.argmax(np.where(np.isnan(d), np.inf, d)), d.shape)
        print('sigma %s, normalised %d: largest |device - restatement| = %.3g at %d bins (pair %d): device %.17g, restatement %.17g'
              % (sigma, normalized, d[b, i], case['bins'][i], b, got[b, i], ref[normalized, regularize][b, i]))
        worst = max(worst, float(np.where(np.isnan(d), np.inf, d).max()))
    assert worst <= BOUND


# ---- 5. every entry of a mixed launch ----
@pytest.mark.parametrize('sigma', C.MIXED_SIGMAS)
def test_mixed_launch(A, sigma):
    case, ref = C.mixed_case(), C.mixed_reference(sigma)
    o, t = _device(case)
    for normalized, regularize in ((False, True), (True, False)):
        batch = _objective(A, case, o, t, normalized, regularize, sigma)
        for b in range(2):
            for i, n in enumerate(case['bins']):
                alone = A.negative_mutual_information_batch(o[b:b + 1], t[b:b + 1], case['transforms'][b, i][None, None], [n],
                                                           init_transforms=case['init'][b:b + 1], regularize=regularize,
                                                           normalized_mi=normalized, smoothing_sigma=sigma)
                assert alone.item() == batch[b, i].item(), (n, b, normalized)
        d = np.abs(batch.cpu().numpy() - ref[normalized, regularize])
        print('sigma %s, normalised %d: largest |device - restatement| = %.3g' % (sigma, normalized, d.max()))
        assert np.all(d <= BOUND), [case['bins'][i] for i in np.argwhere(~(d <= BOUND))[:, 1]]


# ---- 6. Nelder-Mead beyond one workgroup ----
def test_nelder_mead_beyond_one_workgroup(A):
    case = C.nm_case()
    o, t = _device(case)
    problems, kinds, x0 = case['problems'], case['kinds'], case['x0']
    P, K = len(problems), len(kinds)
    fields = ('transform', 'value', 'nit', 'nfev', 'success')
    runs = {}
    for chunk in C.NM_CHUNKS:
        runs[chunk] = A.refine_alignment_batch(o, t, [p[0] for p in problems], [p[1] for p in problems], np.stack([x0] * P),
                                               normalized_mi=True, maxiter=[p[2] for p in problems],
                                               maxfun=[p[3] for p in problems], xatol=[p[4] for p in problems],
                                               fatol=[p[5] for p in problems], chunk=chunk)
    dev = runs[1]
    print('rounds', {chunk: r['rounds'] for chunk, r in runs.items()})
    for chunk, r in runs.items():
        # the count of running problems is read after every chunk: the first multiple of chunk at which none is left
        assert r['rounds'] % chunk == 0 and r['rounds'] == -(-dev['rounds'] // chunk) * chunk
        for k in fields:
            assert np.array_equal(r[k], dev[k]), (chunk, k)
    for k in fields:
        for q in range(K, P):
            assert np.array_equal(dev[k][q], dev[k][q % K]), (k, q)
    for q, (b, n, maxiter, maxfun, xatol, fatol) in enumerate(kinds):
        def f(x):
            return A.calculate_negative_mutual_information(x, o[b], t[b], x0, n, normalized_mi=True)
        host = R.nelder_mead(f, x0.ravel(), xatol=xatol, fatol=fatol, maxiter=maxiter, maxfun=maxfun)
        print(q, host['nit'], host['nfev'], host['success'], host['fun'])
        assert np.array_equal(dev['transform'][q].ravel(), host['x']), q
        assert dev['value'][q] == host['fun']
        assert (dev['nit'][q], dev['nfev'][q], bool(dev['success'][q])) == (host['nit'], host['nfev'], host['success']), q
    assert dev['nfev'][4] == 23 and not dev['success'][4] and dev['nfev'][6] == 7 and not dev['success'][6]
    assert dev['nit'][5] == 1 and dev['nfev'][5] == 10 and dev['success'][5]
    assert all(dev['nit'][q] == 25 and not dev['success'][q] for q in range(4))


# ---- 7. limits ----
def test_limits(A):
    case = C.mixed_case()
    o, t = _device(case)
    opt, th = case['optical'], case['thermal']
    H, W = th.shape[1:]
    eye = np.eye(3)
    for n in (1, 256):
        counts, _, _ = A.joint_histograms(o, t, [1], [n], eye[None])
        assert counts[0].shape == (n, 2 * n) and counts[0].sum() == H * W
        v = A.calculate_negative_mutual_information(eye, o[1], t[1], eye, n)
        assert abs(v - R.negative_mi(eye, opt[1], th[1], eye, n)) <= BOUND
        r = A.refine_alignment_batch(o, t, [1], [n], eye[None], maxiter=2)
        assert r['nit'][0] == 2 and r['nfev'][0] >= 10
    assert int(4.0 * 16.1 + 0.5) == 64 and int(4.0 * 16.125 + 0.5) == 65
    v = A.calculate_negative_mutual_information(eye, o[0], t[0], eye, 16, smoothing_sigma=16.1)
    assert abs(v - R.negative_mi(eye, opt[0], th[0], eye, 16, smoothing_sigma=16.1)) <= BOUND
    with pytest.raises(ValueError, match=r'smoothing sigma must be in \[0, 16\]'):
        A.calculate_negative_mutual_information(eye, o[0], t[0], eye, 16, smoothing_sigma=16.125)
    with pytest.raises(ValueError, match=r'smoothing sigma must be in \[0, 16\]'):
        A.refine_alignment_batch(o, t, [0], [16], eye[None], smoothing_sigma=16.125)
