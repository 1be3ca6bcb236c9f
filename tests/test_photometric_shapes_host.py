"""Photometric shape cases, host side (no GPU): the premises of tests/test_gpu_photometric_shapes.py.

  * the restated mean (R.image_mean) is numpy's on every batch of tests/photometric_shape_cases.py, and every batch can tell
    numpy's summation order from the other orders a wrong kernel could follow;
  * the leaf count and the stack depth of the pairwise walk stay inside what photo_mean_kernel reserves;
  * R.gaussian_blur and R.filter2d, which follow the kernels' own float32 arithmetic, agree with a float64 evaluation written
    here from the border rule alone, on every blur and motion-blur case;
  * R.cv_ellipse_fill leaves a frame untouched by an ellipse outside it, and does not depend on the frame's size inside;
  * R.apply_plan composes the ops of a chain one after the other.
"""
import numpy as np
import pytest

import photometric_restatement as R
import photometric_shape_cases as C
from multipoint_amd.datasets import augmentation as A

F32 = np.float32
EPS = 2.0 ** -23


# ---- the mean ----
@pytest.mark.parametrize('H,W', C.MEAN_SHAPES)
def test_restated_mean_is_numpys(H, W):
    """the contiguous image and the same pixels as a strided crop of a larger array"""
    batch = C.mean_batch(H, W)
    assert batch.shape == (C.MEAN_BATCH, H, W) and batch.dtype == np.float32
    assert float(batch.min()) >= 0.0 and float(batch.max()) < 1.0
    big = np.zeros((H + 2, W + 3), np.float32)
    for img in batch:
        want = R.image_mean(img)
        assert want == img.mean()
        big[1:1 + H, 2:2 + W] = img
        crop = big[1:1 + H, 2:2 + W]
        assert not crop.flags.c_contiguous or H == 1
        assert crop.mean() == want and R.image_mean(crop) == want


@pytest.mark.parametrize('H,W', [s for s in C.MEAN_SHAPES if s[0] * s[1] >= 127])
def test_mean_batches_tell_orders_apart(H, W):
    """A mean summed in another order differs from numpy's by about one ulp, and on a given image often not at all.  For
    every order of C.alternative_orders (left-to-right float32 summation, one un-chunked pairwise sum, chunks of 4096 and of
    16384, and the two slips closest to the kernel: leaves whose accumulators are added left to right, groups whose chunk
    sums are added last to first) at least one image of the batch must give another float32 mean than numpy's.  The seeds of
    C.MEAN_SEEDS were chosen for that.  An order that performs numpy's very additions at this length is no alternative
    (C.alternative_orders says which and why)."""
    n = H * W
    batch = C.mean_batch(H, W).reshape(C.MEAN_BATCH, n)
    want = [a.mean() for a in batch]
    orders = C.alternative_orders(n)
    assert 'left to right' in orders and 'leaves left to right' in orders
    if n > 24576:
        assert len(orders) == 6
    for name, total in orders.items():
        assert any(F32(total(a) / F32(n)) != m for a, m in zip(batch, want)), (name, H, W)


def _walk(n):
    """pairwise_leaves and pairwise_combine of csrc/photometric.hip with their explicit stacks: (leaves, recursion depth,
    highest stack pointer of the leaf walk, of the combine walk, of its value stack)"""
    stack, leaves, sp_leaves, depth = [(0, n, 0)], [], 1, 0
    while stack:
        o, m, d = stack.pop()
        depth = max(depth, d)
        if m <= 128:
            leaves.append((o, m))
        else:
            m2 = m // 2
            m2 -= m2 % 8
            stack += [(o + m2, m - m2, d + 1), (o, m2, d + 1)]
            sp_leaves = max(sp_leaves, len(stack))
    st, vals, sp_combine, sp_vals, nxt = [n], 0, 1, 0, 0
    while st:
        m = st.pop()
        if m < 0:
            vals -= 1
        elif m <= 128:
            vals += 1
            nxt += 1
            sp_vals = max(sp_vals, vals)
        else:
            m2 = m // 2
            m2 -= m2 % 8
            st += [-1, m - m2, m2]
            sp_combine = max(sp_combine, len(st))
    assert vals == 1 and nxt == len(leaves)
    return leaves, depth, sp_leaves, sp_combine, sp_vals


def test_leaf_and_stack_bounds():
    """For every chunk length 1 .. 8192: the leaves tile the chunk in order, none longer than 128; at most 65 of them (first at
    n = 7689; the kernel reserves MEAN_LEAVES = 160 per chunk); the tree is at most 7 splits deep, so the leaf walk holds at
    most depth + 1 = 8 entries (each split pops one and pushes two), the combine walk at most 2 depth + 1 = 15 (pops one,
    pushes three) and its values at most depth + 1 (the kernel reserves STACK = 64 for each).  A chunk of 8192 is the balanced
    tree of FULL_LEAVES = 64 leaves of 128 that the level-by-level reduction assumes."""
    worst_leaves, worst_depth = (0, 0), 0
    for n in range(1, C.MEAN_CHUNK + 1):
        leaves, depth, sp_leaves, sp_combine, sp_vals = _walk(n)
        pos = 0
        for o, m in leaves:
            assert o == pos and 1 <= m <= 128
            pos += m
        assert pos == n
        assert sp_leaves <= depth + 1 and sp_combine <= 2 * depth + 1 and sp_vals <= depth + 1
        if len(leaves) > worst_leaves[0]:
            worst_leaves = (len(leaves), n)
        worst_depth = max(worst_depth, depth)
    assert worst_leaves == (65, 7689) and worst_depth == 7
    assert _walk(C.MEAN_CHUNK)[0] == [(128 * i, 128) for i in range(64)]


# ---- blur and motion blur against a float64 evaluation ----
def _index(n, r):
    return [R.border_interpolate(p, n) for p in range(-r, n + r)]


def _blur64(mask, k):
    """GaussianBlur from its definition: out[y, x] = sum_i sum_j w[i] w[j] mask[reflect(y + i - r), reflect(x + j - r)] with
    the float32 weights of getGaussianKernel, every product and sum in float64, rows then columns"""
    H, W = mask.shape
    w = R.gaussian_kernel(k).astype(np.float64)
    r = k // 2
    m = mask.astype(np.float64)
    cols, rows = _index(W, r), _index(H, r)
    t = np.zeros((H, W))
    for x in range(W):
        t[:, x] = m[:, cols[x:x + k]] @ w
    out = np.zeros((H, W))
    for y in range(H):
        out[y] = w @ t[rows[y:y + k]]
    return out


@pytest.mark.parametrize('H,W', C.BLUR_FRAMES)
def test_restated_blur_against_float64(H, W):
    """The restatement sums k float32 products per pass.  With u = 2^-24 the computed sum of k terms w_j x_j differs from the
    exact one by at most gamma_k sum|w_j x_j|, gamma_k = k u / (1 - k u): each term passes through one rounded product and at
    most k - 1 rounded additions (the column pass adds S[+j] + S[-j] first: one more rounding, one addition fewer in the
    chain, r + 2 <= k in all).  The weights are positive and sum to 1 within k u, so sum|w_j x_j| <= (1 + k u) max|x| and
    each pass is within k 2^-23 max|x| for k <= 801 (k u (1 + 2 k u) < 2 k u).  The column pass carries the row pass's error
    on with weights that sum to 1, so both passes together stay within 2 k 2^-23 max|x| of the float64 evaluation.
    k = 1 has the single weight 1.0: the identity, exactly.  A constant mask c gives c times the weights' sums, within the
    same bound of c."""
    ks = C.blur_ksizes(H, W)
    assert ks[:2] == [1, 3] and ks[-1] == C.MAX_BLUR and 2 * max(H, W) + 1 in ks and 2 * min(H, W) - 1 in ks
    masks = C.blur_masks(H, W)
    assert set(np.unique(masks)) <= {0.0, 1.0}
    if H * W > 1:
        assert any(m.any() and not m.all() for m in masks)
    for (k, _), mask in zip(C.blur_case(H, W), masks):
        got = R.gaussian_blur(mask, k)
        assert got.dtype == np.float32 and got.shape == (H, W)
        if k == 1:
            assert np.array_equal(got, mask)
        bound = 2 * k * EPS * float(mask.max())
        assert float(np.abs(got - _blur64(mask, k)).max()) <= bound, k
        const = np.full((H, W), 0.75, np.float32)
        assert float(np.abs(R.gaussian_blur(const, k) - 0.75).max()) <= 2 * k * EPS * 0.75, k


def test_blur_masks_reach_every_border():
    """on the frames with room for it (both sides >= 15) both values occur on each of the four borders of the masks with and
    without the corner ellipses, and the two differ"""
    for H, W in C.BLUR_FRAMES:
        masks = C.blur_masks(H, W)
        if min(H, W) >= 15:
            assert not np.array_equal(masks[0], masks[1])
            for m in masks[:2]:
                for border in (m[0], m[-1], m[:, 0], m[:, -1]):
                    assert border.min() == 0.0 and border.max() == 1.0, (H, W)


def test_blur_ksizes_fit_the_lds():
    """C.photometric_lds_bytes is the check's formula: 801 fits every BLUR_FRAMES frame; a row wider than 14783 pixels does
    not fit with it; the spans of shade_ellipse_kernel fit up to H = 7870 next to its static arrays"""
    for H, W in C.BLUR_FRAMES:
        assert C.photometric_lds_bytes(H, W, C.MAX_BLUR) == 4 * (801 + (64 + 800) * 16) <= C.LDS_LIMIT
    assert C.photometric_lds_bytes(8, 14783, 801) == 65536 and C.photometric_lds_bytes(8, 14784, 801) > C.LDS_LIMIT
    assert C.blur_ksizes(8, 14784)[-1] < 801
    assert C.SHADE_STATIC_LDS >= 4 * 80 * 8 + 3 * 4
    assert C.photometric_lds_bytes(7870, 2, 1) == 65536 and C.photometric_lds_bytes(7871, 2, 1) > C.LDS_LIMIT


def _filter64(img, mode, k):
    """filter2D from its definition: the motion-blur kernel of the reference (R.motion_taps, float32 weights) correlated
    with the image in float64, BORDER_REFLECT_101"""
    H, W = img.shape
    out = np.zeros((H, W))
    x64 = img.astype(np.float64)
    for dy, dx, w in R.motion_taps(C.MOTION_MODES[mode], k):
        rows = [R.border_interpolate(y + dy, H) for y in range(H)]
        cols = [R.border_interpolate(x + dx, W) for x in range(W)]
        out += float(w) * x64[rows][:, cols]
    return out


@pytest.mark.parametrize('H,W', C.MOTION_FRAMES)
def test_restated_motion_blur_against_float64(H, W):
    """One pass of k taps: within k 2^-23 max|x| (the derivation of test_restated_blur_against_float64; the taps are
    positive and sum to 1 within k u).  k = 1 is the identity, exactly.  The taps and offsets that R.apply_plan takes from the
    plan (A._motion_taps, mode 0 .. 3) are those of R.motion_taps."""
    imgs = C.motion_batch(H, W)
    for (mode, k), img in zip(C.MOTION_PARAMS, imgs):
        taps = R.motion_taps(C.MOTION_MODES[mode], k)
        assert len(taps) == k and [float(w) for _, _, w in taps] == A._motion_taps(C.MOTION_MODES[mode], k)
        got = R.filter2d(img, taps)
        if k == 1:
            assert np.array_equal(got, img)
        assert float(np.abs(got - _filter64(img, mode, k)).max()) <= k * EPS * float(img.max()), (mode, k)
        plan = A.PhotometricPlan((H, W), 'host', C.plan_ops([('m', mode, k)], A._motion_taps))
        assert np.array_equal(R.apply_plan(img, plan), got), (mode, k)
        const = np.full((H, W), 0.75, np.float32)
        assert float(np.abs(R.filter2d(const, taps) - 0.75).max()) <= k * EPS * 0.75


# ---- ellipses ----
def test_ellipse_outside_the_frame():
    for H, W in C.BLUR_FRAMES:
        for x, y, ax, ay, angle in C.blur_ellipses(H, W)[-2:] + [(W + 3, 0, 2, 2, 0), (0, -4, 3, 3, 37), (-5, H // 2, 1, 4, 90),
                                                                   (W // 2, H + 4, 3, 3, 0)]:
            m = np.zeros((H, W), np.float32)
            R.cv_ellipse_fill(m, (x, y), (ax, ay), angle)
            assert not m.any(), (H, W, x, y)


def test_interior_ellipse_does_not_depend_on_the_frame():
    for x, y, ax, ay, angle in ((20, 12, 3, 2, 37), (9, 9, 8, 5, 90), (15, 20, 1, 1, 0), (30, 14, 12, 9, 37)):
        small = np.zeros((32, 48), np.float32)
        R.cv_ellipse_fill(small, (x, y), (ax, ay), angle)
        assert small.any() and not (small[0].any() or small[-1].any() or small[:, 0].any() or small[:, -1].any())
        for H, W in ((41, 55), (32, 49), (200, 48)):
            large = np.zeros((H, W), np.float32)
            R.cv_ellipse_fill(large, (x, y), (ax, ay), angle)
            assert np.array_equal(large[:32, :48], small) and large.sum() == small.sum()


# ---- chains ----
def _step(x, op):
    """one op on its own, from its definition (numpy's mean, the reference's motion-blur kernel)"""
    if op[0] == 'b':
        return np.clip(x + F32(op[1]), 0.0, 1.0).astype(np.float32)
    if op[0] == 'c':
        m = x.mean()
        return np.clip((x - m) * F32(op[1]) + m, 0.0, 1.0).astype(np.float32)
    return R.filter2d(x, R.motion_taps(C.MOTION_MODES[op[1]], op[2]))


@pytest.mark.parametrize('H,W', C.PARITY_FRAMES)
def test_chains_compose(H, W):
    assert [len(p) for p in C.PARITY_PLANS] == [1, 2, 4, 2, 4, 0, C.MAX_OPS]
    blurs = [sum(op[0] == 'm' for op in p) for p in C.PARITY_PLANS]
    assert [b % 2 for b in blurs] == [1, 0, 1, 1, 0, 0, 0]                # images end in either buffer
    for spec, img in zip(C.PARITY_PLANS, C.parity_batch(H, W)):
        plan = A.PhotometricPlan((H, W), 'host', C.plan_ops(spec, A._motion_taps))
        want = np.array(img)
        for op in spec:
            want = _step(want, op)
        got = R.apply_plan(img, plan)
        assert got.dtype == np.float32 and np.array_equal(got, want), spec
        if spec:
            assert not np.array_equal(got, img)
