"""Inputs of the photometric shape tests (tests/test_photometric_shapes_host.py on the CPU, tests/test_gpu_photometric_shapes.py
on the kernels of csrc/photometric.hip).  Plain numpy, seeded; every batch is built once per process (functools.lru_cache) and
is read-only.

  MEAN_SHAPES / mean_batch              frames at every length at which photo_mean_kernel takes another path, eight images each
  sum_left_to_right / sum_chunked       other summation orders a wrong mean kernel could follow
  BLUR_FRAMES / blur_ksizes / blur_ellipses   frames around the 16 x 64 tile of blur_cols_kernel, blur sizes from 1 to 801,
                                        ellipses on every border of the frame and outside it
  MOTION_FRAMES / MOTION_PARAMS / motion_batch   frames smaller than the motion-blur kernel, every mode at sizes 1, 3 and 11
  PARITY_PLANS / plan_ops / parity_batch   chains whose images end in either ping-pong buffer
"""
import functools

import numpy as np

import photometric_restatement as R

F32 = np.float32

# ---- 1. image.mean() ----
MEAN_CHUNK, MEAN_GROUP = 8192, 16          # csrc/photometric.hip
MEAN_SHAPES = [(1, 1), (1, 7),                                         # the n < 8 leaf
               (1, 8), (1, 9), (1, 127), (1, 128), (1, 129),           # the first split
               (1, 7689),                                              # 65 leaves, the maximum for a tail
               (1, 8191),                                              # the longest partial chunk
               (1, 8192),                                              # one chunk with tail == MEAN_CHUNK
               (1, 8193),                                              # one full chunk and a tail of 1
               (2, 8192),                                              # two full chunks
               (16, 8192),                                             # exactly one full group
               (1, 131073),                                            # a second group that holds only a 1-pixel tail
               (17, 8192),                                             # a second group of one full chunk
               (33, 8192),                                             # three groups
               (1, 270337),                                            # 33 full chunks and a tail of 1
               (75, 4099),                                             # 37 full chunks and an unbalanced tail
               (8192, 1), (4099, 3),                                   # H is the long side (H <= 8192 is the API's limit)
               (240, 320)]                                             # a training size
MEAN_BATCH = 8
MEAN_FAMILIES = ('uniform', 'wide', 'ramp', 'uniform', 'wide', 'ramp', 'uniform', 'wide')      # of image 0 .. 7
# One seed per shape.  The default is 1000 + the shape's index; the shapes listed here need another one for the batch to tell
# every alternative order from numpy's (tests/test_photometric_shapes_host.py::test_mean_batches_tell_orders_apart asserts it).
MEAN_SEEDS = {(1, 7689): 2701, (2, 8192): 3101, (16, 8192): 3201, (1, 131073): 3301, (17, 8192): 3403, (33, 8192): 3502,
              (8192, 1): 3801, (240, 320): 4002}


def mean_seed(shape):
    return MEAN_SEEDS.get(tuple(shape), 1000 + MEAN_SHAPES.index(tuple(shape)))


def _field(rng, family, H, W):
    if family == 'uniform':                                  # [0, 1)
        return rng.random((H, W), dtype=np.float32)
    if family == 'wide':                                     # twelve decades: most addends far below the running sum's ulp
        return (rng.random((H, W)) ** 12).astype(np.float32)
    return np.sort(rng.random(H * W, dtype=np.float32)).reshape(H, W)      # ramp: the running sum's exponent keeps growing


def _frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def mean_batch(H, W):
    """(8, H, W) float32 in [0, 1): image i of family MEAN_FAMILIES[i]"""
    rng = np.random.default_rng(mean_seed((H, W)))
    return _frozen(np.stack([_field(rng, f, H, W) for f in MEAN_FAMILIES]))


def sum_left_to_right(a):
    """float32 sum of a 1-D array, one element after the other (np.add.accumulate is sequential)"""
    return np.add.accumulate(np.asarray(a, np.float32), dtype=np.float32)[-1]


def sum_chunked(a, chunk):
    """numpy's order with another buffer size: pairwise sums of `chunk` elements accumulated in order"""
    s = F32(0.0)
    for i in range(0, a.size, chunk):
        s = F32(s + R.pairwise_sum(a[i:i + chunk]))
    return s


def _pairwise_flat_leaf(a):
    """R.pairwise_sum with the eight accumulators of a leaf added left to right instead of as a tree"""
    n = a.shape[0]
    if n < 8:
        return R.pairwise_sum(a)
    if n <= 128:
        r = a[:8].copy()
        i = 8
        while i < n - n % 8:
            r = (r + a[i:i + 8]).astype(np.float32)
            i += 8
        res = r[0]
        for v in list(r[1:]) + list(a[i:]):
            res = F32(res + v)
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return F32(_pairwise_flat_leaf(a[:n2]) + _pairwise_flat_leaf(a[n2:]))


def sum_flat_leaves(a):
    """numpy's order except inside the leaves (a slip in leaf_sum's final expression)"""
    s = F32(0.0)
    for i in range(0, a.size, MEAN_CHUNK):
        s = F32(s + _pairwise_flat_leaf(a[i:i + MEAN_CHUNK]))
    return s


def sum_groups_reversed(a):
    """numpy's order except that the chunk sums of each group of MEAN_GROUP chunks are accumulated last to first"""
    sums = [R.pairwise_sum(a[i:i + MEAN_CHUNK]) for i in range(0, a.size, MEAN_CHUNK)]
    s = F32(0.0)
    for g in range(0, len(sums), MEAN_GROUP):
        for v in reversed(sums[g:g + MEAN_GROUP]):
            s = F32(s + v)
    return s


def alternative_orders(n):
    """{name: sum function} of the orders that are another sequence of additions than numpy's for n elements.  Where an
    order performs numpy's very additions no data can tell it apart, and it is left out:
      * pairwise_sum of 8192 elements splits into 4096 + 4096, and a running total that starts at 0 adds the first two
        chunks of 4096 as that split does.  So chunks of 4096 are numpy's order up to 4096 elements, at 8192, and while the
        elements behind the first 8192 fit one chunk of 4096 (n <= 12288);
      * likewise pairwise_sum of 16384 elements is the sum of two chunks of 8192: chunks of 16384 are numpy's order up to
        8192 elements, at 16384, and while the rest fits one chunk of 8192 (n <= 24576); the un-chunked pairwise sum up to
        8192 elements and at 16384;
      * reversing the first group changes nothing for at most two chunks (0 + a + b = 0 + b + a)."""
    orders = {'left to right': sum_left_to_right, 'leaves left to right': sum_flat_leaves}
    chunks = -(-n // MEAN_CHUNK)
    if chunks > 2:
        orders['groups reversed'] = sum_groups_reversed
    if 4096 < n < 8192 or n > 12288:
        orders['chunks of 4096'] = lambda a: sum_chunked(a, 4096)
    if n > MEAN_CHUNK and n != 16384:
        orders['un-chunked pairwise'] = R.pairwise_sum
    if 8192 < n < 16384 or n > 24576:
        orders['chunks of 16384'] = lambda a: sum_chunked(a, 16384)
    return orders


# ---- 2. blur tiles ----
COL_TX, COL_TY, MAX_BLUR, LDS_LIMIT = 16, 64, 801, 65536          # csrc/photometric.hip, csrc/post_api.hip
SHADE_STATIC_LDS = (4 * 80 * 8 + 3 * 4 + 15) & ~15                # shade_ellipse_kernel: four long long[80] and three ints
# H in {1, 2, 63, 64, 65, 129} x W in {1, 15, 16, 17, 33}, thinned
BLUR_FRAMES = [(1, 1), (1, 16), (1, 33), (2, 1), (2, 17), (63, 15), (63, 33), (64, 16), (64, 17), (65, 1), (65, 17),
               (129, 1), (129, 33)]


def photometric_lds_bytes(H, W, k, ellipses=True):
    """photometric_lds_bytes of csrc/photometric.hip for one shade step whose largest blur size is k"""
    r = k // 2
    b = max(4 * (k + W + 2 * r), 4 * (k + (COL_TY + 2 * r) * COL_TX))
    return max(b, 8 * H + SHADE_STATIC_LDS) if ellipses else b


def blur_ksizes(H, W):
    """1, 3, 2 min(H, W) - 1, 2 max(H, W) + 1 (a radius >= the frame: the reflection repeats) and MP_PHOTO_MAX_BLUR where
    the launch fits the LDS limit of photometric_check"""
    ks = {1, 3, 2 * min(H, W) - 1, 2 * max(H, W) + 1, MAX_BLUR}
    return sorted(k for k in ks if k <= MAX_BLUR and photometric_lds_bytes(H, W, k) <= LDS_LIMIT)


def blur_ellipses(H, W, variant=0):
    """Hand-placed (x, y, ax, ay, angle) with axes >= 1 and angles 0 / 37 / 90: one centred on each corner, one on each
    edge midpoint, three small ones inside, one with its centre outside that reaches into the frame, and two wholly outside
    (below right, above left).  Odd variants leave the corner ellipses out; variants 2, 5, .. have only one ellipse that
    touches the frame, from a centre one row above it (so that a frame of two rows gets a mask that is not constant)."""
    corners = [(0, 0, 2, 1, 37), (W - 1, 0, 1, 2, 0), (0, H - 1, 1, 1, 90), (W - 1, H - 1, 2, 2, 37)]
    edges = [(W // 2, 0, 3, 1, 0), (W // 2, H - 1, 1, 2, 90), (0, H // 2, 1, 3, 37), (W - 1, H // 2, 2, 1, 90)]
    inside = [(W // 3, H // 3, 1, 1, 0), ((2 * W) // 3, H // 2, 2, 3, 37), (W // 4, (3 * H) // 4, 3, 1, 90)]
    reaching = [(-2, H // 4, 4, 2, 0)]
    outside = [(W + 10, H + 10, 3, 2, 37), (-9, -9, 2, 3, 90)]
    if variant % 3 == 2:
        return [(0, -1, 1, 1, 0)] + outside
    return (corners if variant % 2 == 0 else []) + edges + inside + reaching + outside


def blur_case(H, W):
    """[(ksize, ellipses)] of the images of the frame's batch: one image per blur size"""
    return [(k, blur_ellipses(H, W, j)) for j, k in enumerate(blur_ksizes(H, W))]


@functools.lru_cache(maxsize=None)
def blur_masks(H, W):
    """the raw 0 / 1 masks of blur_case(H, W) by the restatement: (n, H, W) float32"""
    out = []
    for _, ells in blur_case(H, W):
        m = np.zeros((H, W), np.float32)
        for x, y, ax, ay, angle in ells:
            R.cv_ellipse_fill(m, (x, y), (ax, ay), angle)
        out.append(m)
    return _frozen(np.stack(out))


# ---- 3. motion blur ----
MOTION_FRAMES = [(1, 1), (1, 5), (5, 1), (2, 3), (7, 7), (31, 45)]
MOTION_MODES = ['h', 'v', 'diag_down', 'diag_up']                  # mode 0 .. 3
MOTION_KSIZES = [1, 3, 11]                                         # 11 = MP_PHOTO_MAX_TAPS
MOTION_PARAMS = [(mode, k) for mode in range(4) for k in MOTION_KSIZES]


@functools.lru_cache(maxsize=None)
def motion_batch(H, W):
    """one uniform image per entry of MOTION_PARAMS: (12, H, W) float32"""
    rng = np.random.default_rng(500 + 64 * H + W)
    return _frozen(rng.random((len(MOTION_PARAMS), H, W), dtype=np.float32))


# ---- 4. parity of the ping-pong buffer ----
# ('m', mode, ksize) motion blur, ('b', value) brightness, ('c', strength) contrast
_M = [('m', 0, 3), ('m', 2, 5), ('m', 1, 11), ('m', 3, 3), ('m', 0, 7), ('m', 3, 9), ('m', 1, 1), ('m', 2, 3)]
PARITY_PLANS = [
    [_M[0]],
    [_M[1], _M[3]],
    [_M[2], ('b', 0.1), _M[3], _M[4]],
    [_M[5], ('c', 1.3)],
    [('b', -0.07), _M[1], ('c', 0.6), _M[0]],
    [],
    [op for i in range(8) for op in (_M[i], ('b', 0.03 * (-1) ** i))],          # MP_PHOTO_MAX_OPS = 16
]
PARITY_FRAMES = [(31, 45), (2, 3)]
MAX_OPS = 16


def plan_ops(spec, taps):
    """the op dicts of a PhotometricPlan from a chain of PARITY_PLANS; taps(mode name, ksize) gives the motion-blur weights
    (multipoint_amd.datasets.augmentation._motion_taps)"""
    ops = []
    for op in spec:
        if op[0] == 'm':
            ops.append({'name': 'motion_blur', 'mode': op[1], 'ksize': op[2], 'taps': taps(MOTION_MODES[op[1]], op[2])})
        else:
            ops.append({'name': 'random_brightness' if op[0] == 'b' else 'random_contrast', 'value': op[1]})
    return ops


@functools.lru_cache(maxsize=None)
def parity_batch(H, W):
    """one uniform image per chain of PARITY_PLANS: (7, H, W) float32"""
    rng = np.random.default_rng(900 + 64 * H + W)
    return _frozen(rng.random((len(PARITY_PLANS), H, W), dtype=np.float32))
