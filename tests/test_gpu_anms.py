"""GPU: spatially uniform top-k (keypoints_spread.hip) against its numpy restatement, byte for byte: the radii of
keypoint lists around every chunk and tile edge of the kernel, the fused entries on small frames, bit stability across runs,
batches and batch order, and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import anms_restatement as A

pytestmark = pytest.mark.gpu

SIZE, THR = 4, 0.015
ROBUST = (1.0, 0.9, 0.5)
# one below, at and above the kernel's candidate chunk (256) and LDS tile (1024); 2500 spans three tiles
N_VALUES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2500)
MP_EINVAL = -1


@pytest.fixture(scope='module')
def U():
    import __graft_entry__ as g
    g.build()
    import multipoint_amd.utils as utils
    return utils


def make_list(rng, n, H=24, W=32, kind='random'):
    """n candidates in row-major order inside H x W (distinct pixels while they fit), scores in (0, 1]"""
    idx = np.sort(rng.choice(H * W, n, replace=n > H * W))
    if kind == 'pow2':
        s = np.ldexp(np.float32(1), -rng.integers(0, 8, n)).astype(np.float32)
    else:
        s = rng.random(n, dtype=np.float32) * np.float32(0.9) + np.float32(0.05)
        if kind == 'quantised':
            s = (np.floor(s * 8) + 1).astype(np.float32) / np.float32(8)          # 8 levels: many exact ties
    return idx // W, idx % W, s


def pack_lists(lists, K):
    B = len(lists)
    kp, sc, cnt = np.zeros((B, K, 2), np.int32), np.zeros((B, K), np.float32), np.zeros(B, np.int32)
    for b, (y, x, s) in enumerate(lists):
        n = len(s)
        kp[b, :n, 0], kp[b, :n, 1], sc[b, :n], cnt[b] = y, x, s, n
    return torch.from_numpy(kp).cuda(), torch.from_numpy(sc).cuda(), torch.from_numpy(cnt).cuda()


def gpu_radii(U, lists, K, robust):
    return U.suppression_radii(*pack_lists(lists, K), robust=robust).cpu().numpy()


@pytest.mark.parametrize('n', N_VALUES)
def test_radii_of_a_list(U, n):
    rng = np.random.default_rng(100 + n)
    for kind in ('random', 'quantised'):
        lst = make_list(rng, n, kind=kind)
        for c in ROBUST:
            got = gpu_radii(U, [lst], n + 3, c)
            assert np.array_equal(got[0, :n], A.radii(*lst, c).astype(np.int64)), (kind, c)
            assert not got[0, n:].any()                              # rows beyond the count are not written


def test_radii_of_a_batch(U):
    rng = np.random.default_rng(7)
    lists = [make_list(rng, 257, kind='quantised'), make_list(rng, 0), make_list(rng, 1025)]
    for c in ROBUST:
        got = gpu_radii(U, lists, 1100, c)
        for b, lst in enumerate(lists):
            n = len(lst[2])
            assert np.array_equal(got[b, :n], A.radii(*lst, c).astype(np.int64)), (b, c)
            assert np.array_equal(gpu_radii(U, [lst], 1100, c)[0], got[b])          # alone == in the batch
    # a count above K is clamped to the stored rows
    kp, sc, cnt = pack_lists(lists[:1], 257)
    big = U.suppression_radii(kp[:, :200].contiguous(), sc[:, :200].contiguous(), cnt, 1.0).cpu().numpy()
    y, x, s = lists[0]
    assert np.array_equal(big[0], A.radii(y[:200], x[:200], s[:200]).astype(np.int64))


def test_radii_exact_products_do_not_dominate(U):
    rng = np.random.default_rng(9)
    lst = make_list(rng, 300, kind='pow2')                           # s_i == 0.5 * s_j exactly between neighbouring levels
    got = gpu_radii(U, [lst], 300, 0.5)[0]
    want = A.radii(*lst, 0.5)
    assert np.array_equal(got, want.astype(np.int64))
    top2 = lst[2] >= 0.5
    assert top2.any() and (want[top2] == A.NONE).all() and (want[~top2] != A.NONE).all()


def test_radii_at_the_corners_of_the_largest_frame(U):
    E = 4095
    corners = (np.array([0, 0, E, E]), np.array([0, E, 0, E]), np.array([0.1, 0.05, 0.05, 0.9], np.float32))
    got = gpu_radii(U, [corners], 4, 1.0)[0]
    assert got.tolist() == [2 * E * E, E * E, E * E, A.NONE] == A.radii(*corners).tolist()
    rng = np.random.default_rng(4)
    y, x, s = make_list(rng, 300, 4096, 4096)
    lst = (np.concatenate([[0, 0], y, [E, E]]), np.concatenate([[0, E], x, [0, E]]),
           np.concatenate([[0.01, 0.02], s * np.float32(0.5), [0.03, 0.99]]).astype(np.float32))
    for c in ROBUST:
        assert np.array_equal(gpu_radii(U, [lst], 304, c)[0], A.radii(*lst, c).astype(np.int64))


# ---- the fused entries ----

def random_peaks(rng, B, H, W):
    m = rng.random((B, 1, H, W), dtype=np.float32)
    return np.where(rng.random((B, 1, H, W)) < 0.25, m, np.float32(0)).astype(np.float32)


def lattice(rng, B, H, W):
    """equal scores on a lattice: every (R, s) ties and the row-major index decides; images after the first get b higher peaks, so
    that rings of equal distance tie"""
    m = np.zeros((B, 1, H, W), np.float32)
    m[:, :, 2::4, 2::4] = 0.5
    for b in range(1, B):
        for _ in range(b):
            m[b, 0, 2 + 4 * rng.integers(0, (H - 2) // 4), 2 + 4 * rng.integers(0, (W - 2) // 4)] = 0.75
    return m


def planted(rng, B, H, W):
    return np.stack([A.planted_map(int(rng.integers(0, 5)))[None] for _ in range(B)])


CASES = [(24, 32, random_peaks), (33, 47, random_peaks), (96, 128, random_peaks), (96, 128, planted),
         (24, 32, lattice), (33, 47, lattice), (96, 128, lattice)]


def check_fused(U, maps, mask, k, K, robust=1.0):
    B, _, H, W = maps.shape
    t = torch.from_numpy(maps).cuda()
    tm = None if mask is None else torch.from_numpy(mask).cuda()
    kp0, sc0, cnt0 = (a.cpu().numpy() for a in U.detect_keypoints(t, SIZE, THR, capacity=H * W, valid_mask=tm))      # the existing path
    kp, sc, cnt, r2 = U.detect_keypoints(t, SIZE, THR, keep_top_k=k, capacity=K, valid_mask=tm, topk_mode='anms',
                                         anms_robust=robust, return_radius=True)
    dense = U.box_nms(t, SIZE, THR, keep_top_k=k, valid_mask=tm, topk_mode='anms', anms_robust=robust).cpu().numpy()
    kp, sc, cnt, r2 = kp.cpu().numpy(), sc.cpu().numpy(), cnt.cpu().numpy(), r2.cpu().numpy()
    for b in range(B):
        y, x, s0 = kp0[b, :cnt0[b], 0], kp0[b, :cnt0[b], 1], sc0[b, :cnt0[b]]
        kept, R = A.select(y, x, s0, k, robust)
        wkp, wsc, wr = kp0[b, kept], s0[kept], R[kept]
        wdense = np.zeros((H, W), np.float32)
        wdense[y[kept], x[kept]] = wsc
        m = len(wsc)
        assert cnt[b] == m, (b, k)
        s = min(m, K)                                                # rows at or beyond K are not stored
        assert np.array_equal(kp[b, :s], wkp[:s].astype(np.int32)), (b, k)
        assert sc[b, :s].tobytes() == wsc[:s].tobytes(), (b, k)
        assert np.array_equal(r2[b, :s], wr[:s].astype(np.int64)), (b, k)
        assert dense[b, 0].tobytes() == wdense.tobytes(), (b, k)


@pytest.mark.parametrize('H,W,make', CASES, ids=['%dx%d-%s' % (h, w, f.__name__) for h, w, f in CASES])
def test_fused_entries_equal_the_restatement(U, H, W, make):
    rng = np.random.default_rng(H * 1000 + W)
    for B in (1, 3):
        maps = make(rng, B, H, W)
        for mask in (None, (rng.random((B, 1, H, W)) < 0.8).astype(np.uint8)):
            tm = None if mask is None else torch.from_numpy(mask).cuda()
            n = int(U.detect_keypoints(torch.from_numpy(maps).cuda(), SIZE, THR, capacity=H * W, valid_mask=tm)[2][0])
            assert n > 2
            for k in sorted({1, 2, n - 1, n, n + 1, 64}):
                check_fused(U, maps, mask, k, k)
            check_fused(U, maps, mask, 64, 10)                       # K < k
            check_fused(U, maps, mask, max(n // 2, 1), max(n // 2, 1), robust=0.9)


def test_short_lists_equal_the_score_mode(U):
    rng = np.random.default_rng(12)
    maps = torch.from_numpy(random_peaks(rng, 3, 33, 47)).cuda()
    a = U.detect_keypoints(maps, SIZE, THR, keep_top_k=2000, capacity=2000)
    b = U.detect_keypoints(maps, SIZE, THR, keep_top_k=2000, capacity=2000, topk_mode='anms')
    n = a[2].cpu().numpy()
    assert np.array_equal(n, b[2].cpu().numpy()) and n.min() > 0
    for i in range(3):
        assert torch.equal(a[0][i, :n[i]], b[0][i, :n[i]]) and torch.equal(a[1][i, :n[i]], b[1][i, :n[i]])
    assert torch.equal(U.box_nms(maps, SIZE, THR, keep_top_k=2000), U.box_nms(maps, SIZE, THR, keep_top_k=2000, topk_mode='anms'))


def test_planted_map_spreads_on_the_gpu(U):
    maps = torch.from_numpy(np.stack([A.planted_map(s)[None] for s in range(5)])).cuda()
    kp_s, _, cnt_s = U.detect_keypoints(maps, SIZE, THR, keep_top_k=64)
    kp_a, _, cnt_a = U.detect_keypoints(maps, SIZE, THR, keep_top_k=64, topk_mode='anms')
    assert cnt_s.tolist() == cnt_a.tolist() == [64] * 5
    for b in range(5):
        assert A.occupied_cells(kp_s[b].cpu().numpy()) == 4 and A.occupied_cells(kp_a[b].cpu().numpy()) >= 15


# ---- bits ----

def _outputs(U, maps, **kw):
    kp, sc, cnt, r2 = U.detect_keypoints(maps, SIZE, THR, keep_top_k=64, topk_mode='anms', return_radius=True, **kw)
    dense = U.box_nms(maps, SIZE, THR, keep_top_k=64, topk_mode='anms', **kw)
    return [t.cpu().numpy() for t in (kp, sc, cnt, r2, dense)]


def test_bits_do_not_depend_on_the_run_the_batch_or_its_order(U):
    rng = np.random.default_rng(3)
    maps = np.concatenate([np.stack([A.planted_map(s)[None] for s in range(3)]), random_peaks(rng, 2, 96, 128)])
    t = torch.from_numpy(maps).cuda()
    for robust in (1.0, 0.9):
        first = _outputs(U, t, anms_robust=robust)
        assert (first[2] == 64).all()
        again = _outputs(U, t, anms_robust=robust)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
        for b in range(len(maps)):                                   # each image alone
            alone = _outputs(U, t[b:b + 1].contiguous(), anms_robust=robust)
            assert all(a[0].tobytes() == f[b].tobytes() for a, f in zip(alone, first)), b
        perm = [3, 0, 4, 2, 1]
        shuffled = _outputs(U, t[perm].contiguous(), anms_robust=robust)
        assert all(s.tobytes() == f[perm].tobytes() for s, f in zip(shuffled, first))


def test_score_mode_is_the_call_without_the_argument(U):
    rng = np.random.default_rng(8)
    t = torch.from_numpy(random_peaks(rng, 3, 96, 128)).cuda()
    for k in (0, 64):
        a = U.detect_keypoints(t, SIZE, THR, keep_top_k=k, capacity=4096)
        b = U.detect_keypoints(t, SIZE, THR, keep_top_k=k, capacity=4096, topk_mode='score', anms_robust=0.7)
        n = a[2].cpu().numpy()
        assert np.array_equal(n, b[2].cpu().numpy())
        for i in range(3):
            assert torch.equal(a[0][i, :n[i]], b[0][i, :n[i]]) and torch.equal(a[1][i, :n[i]], b[1][i, :n[i]])
        assert torch.equal(U.box_nms(t, SIZE, THR, keep_top_k=k), U.box_nms(t, SIZE, THR, keep_top_k=k, topk_mode='score'))


# ---- refusals ----

def test_refusals_leave_the_outputs_untouched(U):
    from multipoint_amd import _lib
    dev = torch.device('cuda:0')
    h = _lib.get_handle(dev)
    rng = np.random.default_rng(1)
    B, H, W, K = 2, 24, 32, 16
    prob = torch.from_numpy(random_peaks(rng, B, H, W)).cuda()
    kp = torch.full((B, K, 2), -7, dtype=torch.int32, device=dev)
    sc = torch.full((B, K), -7.0, device=dev)
    cnt = torch.full((B,), -7, dtype=torch.int32, device=dev)
    r2 = torch.full((B, K), -7, dtype=torch.int32, device=dev)
    dense = torch.full((B, 1, H, W), -7.0, device=dev)
    stream = _lib.stream_ptr(dev)
    p = _lib.ptr

    def detect(size=4.0, topk=8, robust=1.0, b=B):
        return h.lib.mp_detect_keypoints_spread(h.ptr, p(prob), None, b, H, W, size, THR, 0.1, topk, K, p(kp), p(sc), p(cnt), 0,
                                                robust, p(r2), stream)

    def nms(size=4.0, topk=8, robust=1.0, b=B):
        return h.lib.mp_box_nms_spread(h.ptr, p(prob), None, b, H, W, size, THR, 0.1, topk, p(dense), 0, robust, stream)

    def radii(robust=1.0, b=B, k=K):
        return h.lib.mp_suppression_radii(h.ptr, p(kp), p(sc), p(cnt), b, k, robust, p(r2), stream)

    bad_robust = (0.0, -0.5, 1.0000001, 2.0, float('nan'), float('inf'), -float('inf'))
    for call in (detect, nms, radii):
        for c in bad_robust:
            assert call(robust=c) == MP_EINVAL, (call.__name__, c)
        assert call(b=0) == MP_EINVAL
    for call in (detect, nms):
        assert call(topk=0) == MP_EINVAL and call(topk=-3) == MP_EINVAL
        assert call(size=17.0) == MP_EINVAL                           # an existing refusal: the footprint limit
    assert radii(k=0) == MP_EINVAL
    assert h.lib.mp_detect_keypoints_spread(h.ptr, p(prob), None, B, H, W, 4.0, THR, 0.1, 8, 0, p(kp), p(sc), p(cnt), 0, 1.0,
                                            p(r2), stream) == MP_EINVAL          # K = 0
    assert h.lib.mp_suppression_radii(h.ptr, p(kp), None, p(cnt), B, K, 1.0, p(r2), stream) == MP_EINVAL
    torch.cuda.synchronize()
    for t in (kp, sc, cnt, r2, dense):
        assert bool((t == -7).all())
    # and the Python mirror raises ValueError
    with pytest.raises(ValueError):
        U.detect_keypoints(prob, SIZE, THR, keep_top_k=8, topk_mode='anms', anms_robust=0.0)
    with pytest.raises(ValueError):
        U.box_nms(prob, SIZE, THR, keep_top_k=0, topk_mode='anms')
    with pytest.raises(ValueError):
        U.suppression_radii(kp, sc, cnt, robust=1.5)
    # a valid call still works afterwards, and the radii are optional
    assert detect() == 0 and int(cnt.min()) > 0
    assert h.lib.mp_detect_keypoints_spread(h.ptr, p(prob), None, B, H, W, 4.0, THR, 0.1, 8, K, p(kp), None, p(cnt), 0, 1.0,
                                            None, stream) == 0
    torch.cuda.synchronize()
