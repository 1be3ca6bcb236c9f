"""TEST INFRASTRUCTURE: the named cases that tests/test_sampling_host.py (CPU) and tests/test_gpu_sampling_shapes.py (MI355X)
share for the warp, adaptation and descriptor-sampling kernels: seeds, shapes, matrices.  They are the smallest shapes at which
the kernels can go wrong; the host test checks the premises (tile edges on both sides, caps on near-tie and vacuous pixels,
every mutant of tests/sampling_restatement.py told apart).  Nothing here is larger than 50 x 200 pixels, 7 maps or 128 keypoints."""
import numpy as np

# H x W; warp, accumulate and filter kernels run 64 pixels x 4 rows per block
FRAMES = [(1, 1), (3, 63), (4, 64), (5, 65), (37, 129), (33, 200)]
# valid mask: 32 x 32 tiles, halo up to 16
MASK_FRAMES = [(31, 33), (32, 32), (33, 65), (5, 3)]
MASK_RADII = [0, 1, 16]
MASK_G = 5

WARP_VARIANTS = [(m, p) for m in ('bilinear', 'nearest') for p in ('zeros', 'reflection')]


def _shift(tx, ty):
    return np.array([[1.0, 0, tx], [0, 1.0, ty], [0, 0, 1.0]])


def exact_matrices(H, W):
    """destination -> source, third row 0 0 1, entries multiples of 1/4: identity, an integer shift, shifts by exactly 0.5 and
    1.5 (ties to even), the two flips, a shift that puts the whole output outside the source, and one of several frame widths
    (multiple reflections)."""
    return np.stack([np.eye(3), _shift(5, -3), _shift(0.5, 1.5),
                     np.array([[-1.0, 0, W - 1], [0, 1.0, 0], [0, 0, 1.0]]), np.array([[1.0, 0, 0], [0, -1.0, H - 1], [0, 0, 1.0]]),
                     _shift(1000, 0), _shift(3 * W + 2.5, -2 * H - 1)])


Z0_MATRIX = np.array([[1.0, 0, 0], [0, 1.0, 0], [-0.125, 0, 1.0]])       # Z = 0 on the column x = 8
FAR_MATRIX = _shift(2.0 ** 31, 0)                                        # |u| >= 1e9: zeros


def sampled_homographies(seed, n, H, W, **kw):
    """drawn as tests/test_gpu_ha.py draws them (the product's host sampler, numpy's global generator)"""
    from multipoint_amd.utils.homographies import sample_homography
    state = np.random.get_state()
    np.random.seed(seed)
    try:
        return np.stack([sample_homography(np.array([H, W]), **kw) for _ in range(n)])
    finally:
        np.random.set_state(state)


MODERATE = dict(perspective_amplitude_x=0.2, perspective_amplitude_y=0.2, max_angle=1.57)


def projective_matrices(seed, H, W):
    """three sampled homographies, their inverses and the matrix with Z = 0 on a column: 7 destination -> source matrices"""
    m = sampled_homographies(seed, 3, H, W, **MODERATE)
    return np.concatenate([m, np.linalg.inv(m), Z0_MATRIX[None]])


def noise(seed, *shape):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


# ---- warp ----
def warp_cases():
    """dicts: name, src (n_src,H,W) float32, hom (n_out,3,3) destination -> source, dsize, exact (all matrices exact), route
    ('tensor': through warp_perspective_tensor with the source -> destination matrices 'M', whose host inverse is 'hom';
    '_warp': hom handed over),
    paddings (the padding modes the case runs under)."""
    out = []

    def add(name, src, hom, dsize, exact, route, paddings=('zeros', 'reflection')):
        c = dict(name=name, src=src, hom=np.asarray(hom, np.float64), dsize=dsize, exact=exact, route=route, paddings=paddings)
        if route == 'tensor':
            c['M'] = np.linalg.inv(c['hom'])              # source -> destination, what the public function takes ...
            c['hom'] = np.linalg.inv(c['M'])              # ... and inverts on the host in just this way
        out.append(c)

    for i, (H, W) in enumerate(FRAMES):
        add('exact_%dx%d' % (H, W), noise(10 + i, 7, H, W), exact_matrices(H, W), (H, W), True, 'tensor')
        add('proj_%dx%d' % (H, W), noise(20 + i, 3, H, W), projective_matrices(30 + i, H, W), (H, W), False, '_warp')
    H, W = 37, 129
    for Ho, Wo in ((20, 70), (50, 140)):
        add('exact_37x129_to_%dx%d' % (Ho, Wo), noise(41, 3, H, W), exact_matrices(H, W), (Ho, Wo), True, '_warp')
        add('proj_37x129_to_%dx%d' % (Ho, Wo), noise(42, 7, H, W), projective_matrices(43, H, W), (Ho, Wo), False, 'tensor')
    corner = np.zeros((3, 5, 65), np.float32)
    corner[0, 0, 0] = corner[1, 4, 64] = corner[2, 0, 64] = 1.0
    add('corner_exact_5x65', corner, exact_matrices(5, 65), (5, 65), True, '_warp')
    add('corner_proj_5x65', corner, projective_matrices(44, 5, 65), (5, 65), False, '_warp')
    add('far_5x65', noise(45, 1, 5, 65), FAR_MATRIX[None], (5, 65), False, '_warp', ('zeros',))
    return out


# ---- accumulate ----
AGGREGATIONS = [0, 1, 2]
GB = [(1, 1), (3, 2), (4, 3), (1, 5)]


def accumulate_cases():
    """dicts: name, agg, G, B, H, W, pa, pb (G*B,H,W), mask (G,H,W) uint8, hom (G,3,3), prob0, count0 (B,H,W): a state that
    is not begin's, so a kernel that overwrites instead of adding is seen.  Views: a sampled homography, the matrix with a
    column at infinity, an exact shift, an inverse."""
    out = []
    for fi, (H, W) in enumerate(FRAMES):
        for gi, (G, B) in enumerate(GB):
            for agg in AGGREGATIONS:
                seed = 100 + 20 * fi + 4 * gi + agg
                m = sampled_homographies(seed, 2, H, W, **MODERATE)
                views = [m[0], Z0_MATRIX, _shift(2, -1), np.linalg.inv(m[1])]
                hom = np.stack(views[:G]) if (G, B) != (1, 1) else Z0_MATRIX[None]
                rng = np.random.default_rng(seed)
                mask = (rng.random((G, H, W)) < 0.7).astype(np.uint8)
                mask[:, H // 3:H // 3 + max(1, H // 8), :] = 0      # a zero band
                mask[:, 0, 0] = 1
                out.append(dict(name='acc%d_G%dB%d_%dx%d' % (agg, G, B, H, W), agg=agg, G=G, B=B, H=H, W=W,
                                pa=rng.random((G * B, H, W), dtype=np.float32) + np.float32(0.25),
                                pb=rng.random((G * B, H, W), dtype=np.float32) + np.float32(0.25),
                                mask=mask, hom=hom, prob0=rng.random((B, H, W), dtype=np.float32),
                                count0=rng.integers(0, 4, (B, H, W)).astype(np.float32)))
    return out


# ---- begin / finalize ----
POINTWISE_SHAPES = [(1, 1, 1), (1, 5, 51), (1, 16, 16), (1, 1, 257)]     # n = 1, 255, 256, 257 (256 threads per block)
MIN_COUNTS = [0.0, 1.0, 2.5]


def pointwise_case(shape, agg):
    """pa, pb for begin; prob, count for finalize: counts 0, 1, 2, 2.5, 3 (0 and the values equal to min_count included),
    prob with zeros (0 / 0) and a few negative values (sqrt of a negative)."""
    rng = np.random.default_rng(1000 + shape[1] * shape[2] + agg)
    n = int(np.prod(shape))
    count = np.array([0.0, 1.0, 2.0, 2.5, 3.0], np.float32)[(np.arange(n) + agg) % 5].reshape(shape)
    prob = (rng.random(shape, dtype=np.float32) * 3).astype(np.float32)
    prob.reshape(-1)[::7] = 0.0
    prob.reshape(-1)[3::11] *= -1.0
    return dict(pa=rng.random(shape, dtype=np.float32), pb=rng.random(shape, dtype=np.float32) - np.float32(0.3), prob=prob,
                count=count)


# ---- gaussian filter ----
FILTER_SIZES = [1, 3, 9, 31]
FILTER_WEIGHTS = ['gaussian', 'random', 'one_hot']


def filter_frames(k):
    """the smallest legal frames, H = r + 1 at W = 64 and W = r + 1 at H = 5 (at H = r + 1 where r >= 5 makes H = 5 illegal), and
    every frame of FRAMES with r < H, W"""
    r = (k - 1) // 2
    out = [(r + 1, 64), (5, r + 1) if r < 5 else (r + 1, r + 1)] + [(H, W) for H, W in FRAMES if r < H and r < W]
    return list(dict.fromkeys(out))


def one_hot_position(k):
    return (0, k - 1) if k > 1 else (0, 0)


def filter_weights(kind, k):
    """(k,k) float32; 'gaussian' is the project's own table"""
    if kind == 'gaussian':
        from multipoint_amd.utils.homographies import get_gaussian_filter
        return get_gaussian_filter(k)[0, 0].numpy().astype(np.float32)
    if kind == 'random':
        return (np.random.default_rng(50 + k).random((k, k), dtype=np.float32) - np.float32(0.3)).astype(np.float32)
    w = np.zeros((k, k), np.float32)
    w[one_hot_position(k)] = 1.0
    return w


def filter_input(k, H, W):
    return noise(60 + k + H + W, 2, H, W)


# ---- valid mask ----
def mask_homographies(H, W):
    """MASK_G destination -> source matrices: three sampled, one inverse, the column at infinity"""
    m = sampled_homographies(70 + H + W, 4, H, W, perspective_amplitude_x=0.2, perspective_amplitude_y=0.2, patch_ratio=0.85)
    return np.stack([np.linalg.inv(m[0]), np.linalg.inv(m[1]), np.linalg.inv(m[2]), m[3], Z0_MATRIX])


# ---- descriptor sampling ----
DESC_D = [64, 128, 192, 256, 320, 384]
DESC_BK = [(1, 1), (1, 5), (3, 7), (2, 64)]
DESC_GEOMETRY = [(12, 20, 96, 160), (1, 9, 8, 72), (7, 1, 56, 8), (5, 6, 37, 53)]       # Hc, Wc, H, W
INT_MIN = -2 ** 31


def _keypoints(rng, B, K, H, W, rot):
    special = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H, W), (H // 2, -1), (H // 3, 2 * W)]
    kp = np.zeros((B, K, 2), np.int32)
    for b in range(B):
        pts = special[(rot + b) % 7:] + special[:(rot + b) % 7]
        pts += [(int(rng.integers(0, H)), int(rng.integers(0, W))) for _ in range(max(0, K - 7))]
        kp[b] = np.array(pts[:K], np.int32)
    return kp


def _desc_case(name, D, B, K, geom, idx, counts=None, scale=1.0, zero_cell=False, stale=False):
    Hc, Wc, H, W = geom
    rng = np.random.default_rng(2000 + idx)
    desc = (rng.standard_normal((B, Hc, Wc, D)) * scale).astype(np.float32)
    kp = _keypoints(rng, B, K, H, W, idx)
    pool = [0, 1, K - 1, K, K + 3]
    cnt = np.array(counts if counts is not None else [pool[(idx + 3 * b) % 5] for b in range(B)], np.int32)
    zero_rows = []
    if zero_cell:                     # keypoint (b=0, k=1) sits in an all-zero neighbourhood: sqrt(ss) == 0, the floor decides
        kp[0, 1] = (H // 2, W // 2)
        cy, cx = (H // 2) * (Hc - 1) // H, (W // 2) * (Wc - 1) // W
        desc[0, max(cy - 1, 0):cy + 3, max(cx - 1, 0):cx + 3] = 0.0
        zero_rows = [(0, 1)]
    for b in range(B):                # what lies beyond the count is never read: INT_MIN, or (stale) an earlier call's keypoints
        if not (stale and b > 0 and cnt[b - 1] > K):
            kp[b, max(min(int(cnt[b]), K), 0):] = INT_MIN
    # every tap of a keypoint at x = 2W lies outside the map (Wc > 1): sqrt(ss) is exactly 0 there, not merely small
    low = [(b, k) for b in range(B) for k in range(min(int(cnt[b]), K)) if not (kp[b, k, 1] == 2 * W and Wc > 1)] if scale != 1.0 else []
    return dict(name=name, desc=desc, H=H, W=W, kp=kp, count=cnt, low_norm_rows=low, zero_rows=zero_rows)


def desc_cases():
    """dicts: name, desc (B,Hc,Wc,D) channels-last float32, H, W, kp (B,K,2) int32 (y,x) with INT_MIN beyond the count (in the
    'spill' cases: plausible keypoints behind an image whose count exceeds K),
    count (B,), low_norm_rows: the (b,k) whose sqrt(ss) is below 1e-6 without being 0 (only 'finite, norm <= 1' holds there),
    zero_rows: valid rows whose taps are all 0."""
    out = []
    idx = 0
    for di, D in enumerate(DESC_D):
        for bi, (B, K) in enumerate(DESC_BK):
            geom = DESC_GEOMETRY[(di + bi) % 4]
            out.append(_desc_case('D%d_B%dK%d_%dx%d' % (D, B, K, geom[0], geom[1]), D, B, K, geom, idx))
            idx += 1
    out.append(_desc_case('spill_D64_B3K7', 64, 3, 7, DESC_GEOMETRY[0], 90, counts=[10, 1, 7], stale=True))
    out.append(_desc_case('spill_D192_B2K64', 192, 2, 64, DESC_GEOMETRY[3], 91, counts=[67, 0], stale=True))
    out.append(_desc_case('zero_cell_D128_B3K7', 128, 3, 7, DESC_GEOMETRY[0], 92, counts=[7, 6, 10], zero_cell=True))
    out.append(_desc_case('tiny_D128_B3K7', 128, 3, 7, DESC_GEOMETRY[0], 93, counts=[7, 6, 10], scale=1e-20))
    return out
