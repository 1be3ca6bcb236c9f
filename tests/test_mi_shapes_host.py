"""CPU: the premises of the inputs tests/mi_shape_cases.py builds for tests/test_gpu_mi_shapes.py, on the numpy restatement
tests/mi_restatement.py alone: the frames have the block structure they are chosen for, OpenCV's block-wise coordinate sum
decides a pixel of each frame wider than a block, the edge frames hold every edge and both its neighbours and numpy bins
them as the restatement does, and no objective value is infinite or undefined."""
import numpy as np
import pytest

import mi_restatement as R
import mi_shape_cases as C

SPLIT = [i for i, s in enumerate(C.FRAMES) if R.block_width(s[2], s[3]) < s[3]]


def test_block_structure_of_the_frames():
    """what the frames are chosen for, from the launch arithmetic of launch_mi_histograms / launch_mi_thermal"""
    got = [(min(16, H), R.block_width(H, W)) for _, _, H, W in C.FRAMES]
    assert got == [(5, 204), (16, 64), (16, 64), (1, 70), (16, 1), (1, 1), (16, 64)]
    assert SPLIT == [0, 1, 2, C.LARGE]
    assert 230 - 204 == 26 and 131 - 2 * 64 == 3 and 65 - 64 == 1           # the last blocks
    assert [H % 4 for _, _, H, W in C.FRAMES[:3]] == [1, 1, 0] and [-(-W // 64) for _, _, H, W in C.FRAMES[:3]] == [4, 3, 2]
    H, W = C.FRAMES[C.LARGE][2:]
    assert H * W == 135168 > 64 * 2048 and -(-H * W // 2048) == 66           # a second grid-stride trip; 66 histogram workgroups
    for i in range(len(C.FRAMES)):
        c = C.frame_case(i)
        B = c['optical'].shape[0]
        assert c['optical'].shape[1:] == C.FRAMES[i][:2] and c['thermal'].shape == (B,) + C.FRAMES[i][2:]
        assert B == (1 if i == C.LARGE else 3)
        assert c['pair'][:8] == ([0] * 8 if B == 1 else [2, 2, 0, 0, 1, 1, 0, 0]) and set(c['bins']) == {16, 65}
        assert len(c['pair']) == len(c['bins']) == len(c['transforms']) == 6 * 2 * (1 if B == 1 else 4)
        assert np.all(c['thermal'].reshape(B, -1).min(1) < c['thermal'].reshape(B, -1).max(1)) or C.FRAMES[i][2:] == (1, 1)


@pytest.mark.parametrize('i', SPLIT)
def test_the_split_sum_decides_a_pixel(i):
    """For at least one pixel behind the first block, the fixed-point coordinate of the block-wise sum is not the one of the
    sum taken with xb = 0 -- and the warped frames of every pair differ there, so a kernel with bw0 = W cannot pass."""
    c = C.frame_case(i)
    H, W = c['shape'][2:]
    T = C.perspective_transform(H, W)
    assert abs(T[2, 0]) >= 1e-4 and abs(T[2, 1]) >= 1e-4                       # a noticeable perspective row
    assert any(np.array_equal(T, t) for t in c['transforms'])
    Mi = R.cv_invert3(R.cv_invert3(T))
    X, Y = R.fixed_point(Mi, H, W)
    X0, Y0 = R.fixed_point(Mi, H, W, split=False)
    differ = (X != X0) | (Y != Y0)
    bw0 = R.block_width(H, W)
    assert differ.any() and not differ[:, :bw0].any()
    print('%d x %d: pixels %s' % (H, W, np.argwhere(differ).tolist()))
    for p in range(c['optical'].shape[0]):
        a, b = R.warp_image(c['optical'][p], T, H, W), R.warp_image(c['optical'][p], T, H, W, split=False)
        assert np.any(a.view(np.uint32) != b.view(np.uint32)), p


def test_frame_references_see_every_kind_of_frame():
    for i in range(len(C.FRAMES)):
        c, ref = C.frame_case(i), C.frame_reference(i)
        H, W = c['shape'][2:]
        assert all(h.sum() == H * W and h.shape == (n, 2 * n) for (_, h), n in zip(ref, c['bins']))
        assert any(w.min() == -1.0 and w.max() > -1.0 for w, _ in ref) or H * W == 1          # a border inside the frame
        assert any(w.min() == w.max() for w, _ in ref)                                         # a constant frame: the +-0.5 rule
    # the single sample: both axes take the +-0.5 rule, the one count lies in the middle of the histogram
    c, ref = C.frame_case(5), C.frame_reference(5)
    for (w, h), n in zip(ref, c['bins']):
        assert h[(n - 1) // 2:n // 2 + 1, n - 1:n + 1].sum() == 1


def test_bin_count_case():
    c, ref = C.bins_case(), C.bins_reference()
    assert c['bins'] == C.BIN_COUNTS * 2 and set(c['pair']) == {0, 1, 2}
    assert all(w.min() >= 0.0 for w, _ in ref[:16]) and all(w.min() == -1.0 and w.max() > 0 for w, _ in ref[16:])
    # partial_kernel's row blocks of ceil(n / MI_PARTS) rows: fewer than MI_PARTS = 16 of them below 16 bins and at 17 (9) and
    # 33 (11), a partial last one at 17, 31, 63, 127 and 255
    rows = lambda n: -(-n // 16)
    assert all(-(-n // rows(n)) < 16 for n in (1, 2, 3, 15, 17, 33)) and all(n % rows(n) != 0 for n in (17, 31, 63, 127, 255))


def test_identity_warp_copies_the_edge_frames():
    c, ref = C.edge_case(), C.edge_reference()
    assert c['shape'][:2] == c['shape'][2:]
    for (w, _), p in zip(ref, c['pair']):
        assert np.array_equal(w.view(np.uint32), c['optical'][p].view(np.uint32))


@pytest.mark.parametrize('e', range(len(C.EDGE_BINS) + len(C.LEVEL_BINS)))
def test_edge_frames(e):
    c = C.edge_case()
    p, n = c['pair'][e], c['bins'][e]
    x, y = c['optical'][p].ravel(), c['thermal'][p].ravel()
    got = C.edge_reference()[e][1]
    assert np.array_equal(got, np.histogram2d(x, y, bins=(n, 2 * n))[0].astype(np.int64))
    if e < len(C.EDGE_BINS):
        assert n == C.EDGE_BINS[p]
        for v, m in ((x, n), (y, 2 * n)):
            edges = C.intended_edges(m)
            assert (edges[0], edges[m]) == C.EDGE_RANGE and np.all(np.diff(edges) > 0)
            assert np.array_equal(R.bin_edges(v, m), edges)                    # the frame's own edges are the intended ones
            inner = edges[1:m]
            for w in (inner, np.nextafter(inner, np.float32(-np.inf)), np.nextafter(inner, np.float32(np.inf))):
                assert w.dtype == np.float32 and np.all(np.isin(w, v))
            # an edge opens its bin, the float32 below it closes the one before
            k = R.bin_index(v, m)
            for i in range(1, m):
                assert np.all(k[v == edges[i]] == i) and np.all(k[v == np.nextafter(edges[i], np.float32(-np.inf))] == i - 1)
            assert np.all(k[v == edges[m]] == m - 1)
    else:
        lv = C.levels()
        assert np.all(np.isin(lv, x)) and np.all(np.isin(lv, y))
        if n == 255:
            # step = 1 / 255 in float32: 130 levels are an edge, the others lie one ulp from one
            edges = R.bin_edges(x, n)
            on = np.isin(lv, edges)
            assert on.sum() == 130
            off = np.abs(lv[~on, None].astype(np.float64) - edges[None].astype(np.float64)).min(1)
            assert np.all(off <= np.spacing(lv[~on]))


@pytest.mark.parametrize('sigma', C.SIGMAS)
def test_objective_reference_is_finite(sigma):
    c, ref = C.objective_case(), C.objective_reference(sigma)
    assert [int(4.0 * s + 0.5) for s in C.SIGMAS[1:]] == [0, 2, 20, 64]
    for key, v in ref.items():
        assert v.shape == (2, len(C.BIN_COUNTS)) and np.all(np.isfinite(v)), key
    # the composition is R.negative_mi's
    for b, i in ((0, 0), (1, 4), (0, 9), (1, 11)):
        n, T = c['bins'][i], c['transforms'][b, i]
        assert ref[False, True][b, i] == R.negative_mi(T, c['optical'][b], c['thermal'][b], c['init'][b], n, True, False, sigma)
        assert ref[True, False][b, i] == R.negative_mi(T, c['optical'][b], c['thermal'][b], c['init'][b], n, False, True, sigma)
    # every bin count meets two of the four transforms, one per pair
    assert set(c['tindex'][:, 0]) == {0, 2} and set(c['tindex'][:, 1]) == {1, 3}


@pytest.mark.parametrize('sigma', C.MIXED_SIGMAS)
def test_mixed_reference_is_finite(sigma):
    ref = C.mixed_reference(sigma)
    assert C.mixed_case()['bins'] == [100, 32, 1, 64, 65, 17, 256, 16]
    assert all(np.all(np.isfinite(v)) for v in ref.values())


def test_nelder_mead_case():
    c = C.nm_case()
    assert len(c['problems']) == 70 > 64 and len(c['kinds']) == 7
    assert all(c['problems'][q] == c['kinds'][q % 7] for q in range(70))
    assert c['optical'].shape == (2, 48, 64) and c['thermal'].shape == (2, 40, 56)
