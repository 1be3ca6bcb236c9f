"""Inputs of the mutual-information shape tests (tests/test_mi_shapes_host.py on the CPU, tests/test_gpu_mi_shapes.py on the
kernels of csrc/mutual_info.hip) and the answers of the numpy restatement tests/mi_restatement.py for them.  Plain numpy,
seeded; every case and every answer is built once per process (functools.lru_cache) and must not be written to.

  frame_case / frame_reference          destination frames wider than one of OpenCV's blocks, lower than 16 rows, a single
                                        row / column / pixel, and one above 64 * 2048 pixels
  bins_case / bins_reference            one packed launch over bin counts from 1 to 256 on the 37 x 131 frame
  edge_case / edge_reference            frames made of the float32 bin edges and their neighbours, and of the 256 8-bit levels
  objective_case / objective_reference  the objective over those bin counts and the smoothing radii 0, 2, 20 and 64
  mixed_case / mixed_reference          eight bin counts inside one objective launch
  nm_case                               70 Nelder-Mead problems, seven distinct
"""
import functools

import numpy as np

import mi_restatement as R

# (source Ho, Wo, destination H, W)
FRAMES = [(9, 250, 5, 230),        # bh0 = 5, bw0 = 204: a second block of 26 pixels
          (45, 150, 37, 131),      # bw0 = 64: blocks at 0 / 64 / 128, the last 3 pixels wide; H % 4 = 1
          (20, 70, 16, 65),        # a one-pixel last block
          (3, 80, 1, 70),          # a single row
          (80, 3, 70, 1),          # a single column
          (2, 2, 1, 1),            # one sample: a == b on both axes
          (300, 500, 264, 512)]    # 135168 pixels > 64 * 2048
LARGE = 6
FRAME_BINS = (16, 65)
PAIR_ORDER = (2, 0, 1, 0)
BIN_COUNTS = [1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 255, 256]
SIGMAS = [0, 0.1, 0.6, 5, 16]      # radii int(4 sigma + 0.5) = -, 0, 2, 20, 64
MIXED_BINS = [100, 32, 1, 64, 65, 17, 256, 16]
MIXED_SIGMAS = [0, 1.5]
EDGE_BINS = [3, 16, 64, 65, 100, 256]
EDGE_RANGE = (np.float32(-0.3), np.float32(0.9))
EDGE_ROLL = 1013
LEVEL_BINS = [51, 85, 128, 255, 256]
MID = 1                            # the 37 x 131 frame of the bin-count, edge, objective and mixed cases


def pairs(shape, B, seed):
    """B pairs: optical frames of 8-bit levels (blobs plus noise, so that neighbouring pixels differ), thermal frames that
    depend on them"""
    Ho, Wo, H, W = shape
    rng = np.random.default_rng(seed + 100)
    blobs = [R.blob_image(seed + b, max(Ho, H), max(Wo, W), 25) for b in range(B)]
    opt = np.stack([np.round((0.75 * blobs[b][:Ho, :Wo] + 0.25 * rng.random((Ho, Wo))) * 255) / 255
                    for b in range(B)]).astype(np.float32)
    th = np.stack([(1.0 - blobs[b][:H, :W]) ** 2 + 0.05 * rng.random((H, W)) for b in range(B)]).astype(np.float32)
    return opt, th


def histogram_transforms():
    """those of tests/test_gpu_mi.py::_histogram_transforms"""
    return [np.eye(3),
            np.array([[1, 0, 0.37], [0, 1, -0.81], [0, 0, 1.0]]),                           # a fractional translation
            np.array([[0.8, 0.1, -6.0], [-0.12, 1.1, 4.0], [1e-3, -5e-4, 1.0]]),           # part of the frame outside: min = -1
            np.array([[1, 0, 1000.0], [0, 1, 1000.0], [0, 0, 1.0]]),                        # everything outside: min = max = -1
            np.zeros((3, 3))]                                                               # singular: every pixel reads (0, 0)


def _perspective(c):
    return np.array([[1.02, -0.03, c], [0.02, 0.97, 1.5], [2e-4, -1e-4, 1.0]])


@functools.lru_cache(maxsize=None)
def perspective_transform(H, W):
    """A transform with a noticeable perspective row whose x translation is chosen so that OpenCV's block-wise coordinate
    sum decides a pixel: the sums X0 + h[0] * (x - xb) with the block start xb > 0 and with xb = 0 differ in the last bit
    of a float64 for many pixels, but the 1/32 px coordinate only where the value lies that close to a rounding tie.  The
    translation is bisected (between 2 and 2 + 1/16 px, a shift of two units of 1/32 px) down to the two neighbouring
    float64 between which the coordinate of one pixel behind the first block changes; pixels are tried until the split
    sum and the unsplit one fall on different sides there.  Frames of one block get the translation 2."""
    bw0 = R.block_width(H, W)
    if bw0 >= W:
        return _perspective(2.0)
    h = min(H, 16)                 # (the rows of the first block row: the same arithmetic as in the whole frame)

    def coords(c, split=True):
        return R.fixed_point(R.cv_invert3(R.cv_invert3(_perspective(c))), h, W, split)[0]
    for y in range(h):
        for x in range(W - 1, bw0 - 1, -1):
            lo, hi = 2.0, 2.0 + 1.0 / 16
            k = coords(lo)[y, x]
            assert coords(hi)[y, x] > k
            while np.nextafter(lo, hi) < hi:
                mid = 0.5 * (lo + hi)
                if coords(mid)[y, x] > k:
                    hi = mid
                else:
                    lo = mid
            for c in (lo, hi):
                if coords(c)[y, x] != coords(c, False)[y, x]:
                    return _perspective(c)
    raise AssertionError('no pixel of a %d x %d frame separates the split sum from the unsplit one' % (H, W))


def frame_transforms(H, W):
    return histogram_transforms() + [perspective_transform(H, W)]


# ---- 1. frames ----
@functools.lru_cache(maxsize=None)
def frame_case(i):
    """dict(shape, optical (B, Ho, Wo), thermal (B, H, W), pair, bins, transforms (E, 3, 3), tindex): every transform at 16
    and 65 bins for the pairs 2, 0, 1, 0 in that order (B = 3), for pair 0 alone in the large frame (B = 1)"""
    shape = FRAMES[i]
    H, W = shape[2:]
    B = 1 if i == LARGE else 3
    opt, th = pairs(shape, B, 20 + i)
    Ts = frame_transforms(H, W)
    pair, bins, tindex = [], [], []
    for k in range(len(Ts)):
        for p in ((0,) if B == 1 else PAIR_ORDER):
            for n in FRAME_BINS:
                pair.append(p); bins.append(n); tindex.append(k)
    return {'shape': shape, 'optical': opt, 'thermal': th, 'pair': pair, 'bins': bins, 'tindex': tindex,
            'transforms': np.stack([Ts[k] for k in tindex])}


def _histogram_reference(case):
    """per evaluation (warped frame, counts); a (pair, transform) is warped once"""
    H, W = case['thermal'].shape[1:]
    warps, out = {}, []
    for p, n, k, T in zip(case['pair'], case['bins'], case['tindex'], case['transforms']):
        if (p, k) not in warps:
            warps[p, k] = R.warp_image(case['optical'][p], T, H, W)
        w = warps[p, k]
        out.append((w, R.joint_histogram(w.ravel(), case['thermal'][p].ravel(), n)))
    return out


@functools.lru_cache(maxsize=None)
def frame_reference(i):
    return _histogram_reference(frame_case(i))


# ---- 2. bin counts ----
def inside_transform():
    """keeps the 37 x 131 frame inside its 45 x 150 source"""
    return np.array([[1.0, 0.01, 3.2], [-0.01, 1.0, 2.7], [0.0, 0.0, 1.0]])


@functools.lru_cache(maxsize=None)
def bins_case():
    """the 37 x 131 pairs under a transform that stays inside the source and one that leaves a border of -1, at every bin count"""
    f = frame_case(MID)
    Ts = [inside_transform(), histogram_transforms()[2]]
    pair, bins, tindex = [], [], []
    for k in range(2):
        for j, n in enumerate(BIN_COUNTS):
            pair.append((2, 0, 1)[(j + k) % 3]); bins.append(n); tindex.append(k)
    return {'shape': f['shape'], 'optical': f['optical'], 'thermal': f['thermal'], 'pair': pair, 'bins': bins, 'tindex': tindex,
            'transforms': np.stack([Ts[k] for k in tindex])}


@functools.lru_cache(maxsize=None)
def bins_reference():
    return _histogram_reference(bins_case())


# ---- 3. samples on the edges ----
def intended_edges(n):
    return R.bin_edges(np.array(EDGE_RANGE, np.float32), n)


def edge_values(n):
    """every edge of n bins over EDGE_RANGE, both float32 neighbours of each (clipped to the range), and the range's ends"""
    a, b = EDGE_RANGE
    e = intended_edges(n)
    v = np.concatenate([e, np.nextafter(e, np.float32(-np.inf)), np.nextafter(e, np.float32(np.inf)), [a, b]]).astype(np.float32)
    return np.clip(v, a, b)


def levels():
    return (np.arange(256) / 255.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def edge_case():
    """Frames the size of their source, for the identity transform.  Pairs 0 .. 5: the edge values of EDGE_BINS[p] bins tiled
    over the optical frame, those of twice as many bins, rolled, over the thermal one.  Pair 6: the 256 levels k / 255 tiled
    over the optical frame and in a seeded order over the thermal one, counted at each of LEVEL_BINS."""
    H, W = FRAMES[MID][2:]
    opt = [np.resize(edge_values(n), H * W) for n in EDGE_BINS]
    th = [np.roll(np.resize(edge_values(2 * n), H * W), EDGE_ROLL) for n in EDGE_BINS]
    lv = np.resize(levels(), H * W)
    opt.append(lv)
    th.append(np.random.default_rng(7).permutation(lv))
    pair = list(range(len(EDGE_BINS))) + [len(EDGE_BINS)] * len(LEVEL_BINS)
    return {'shape': (H, W, H, W), 'optical': np.stack(opt).reshape(-1, H, W), 'thermal': np.stack(th).reshape(-1, H, W),
            'pair': pair, 'bins': EDGE_BINS + LEVEL_BINS, 'tindex': [0] * len(pair), 'transforms': np.stack([np.eye(3)] * len(pair))}


@functools.lru_cache(maxsize=None)
def edge_reference():
    return _histogram_reference(edge_case())


# ---- 4. / 5. the objective ----
def objective_transforms():
    """for the 37 x 131 frame in its 45 x 150 source: inside, a fractional translation, partly outside, a mild perspective"""
    return [inside_transform(),
            np.array([[1, 0, 0.37], [0, 1, -0.81], [0, 0, 1.0]]),
            np.array([[0.8, 0.1, -6.0], [-0.12, 1.1, 4.0], [1e-3, -5e-4, 1.0]]),
            np.array([[1.03, -0.02, 1.5], [0.015, 0.97, -0.7], [-2e-5, 3e-5, 1.0]])]


def _objective_case(bins):
    """B = 2 pairs of the 37 x 131 frame, one entry per bin count: entry i of pair b has the transform (i + 2 b) % 4"""
    f = frame_case(MID)
    Ts = objective_transforms()
    init = np.stack([np.eye(3), np.array([[1.01, 0, 0.5], [0, 0.99, -0.5], [0, 0, 1.0]])])
    tindex = np.array([[(i + 2 * b) % 4 for i in range(len(bins))] for b in range(2)])
    return {'shape': f['shape'], 'optical': f['optical'][:2], 'thermal': f['thermal'][:2], 'bins': list(bins), 'tindex': tindex,
            'transforms': np.stack([np.stack([Ts[k] for k in row]) for row in tindex]), 'init': init}


def _objective_reference(case, sigma):
    """{(normalized, regularize): (B, E) values} for (False, True) and (True, False), the two combinations the tests run:
    R.negative_mi's composition with the warp, the histogram and the smoothing of an entry computed once"""
    B, E = case['tindex'].shape
    H, W = case['thermal'].shape[1:]
    out = {(False, True): np.empty((B, E)), (True, False): np.empty((B, E))}
    warps = {}
    for b in range(B):
        for i, n in enumerate(case['bins']):
            k, T = case['tindex'][b, i], case['transforms'][b, i]
            if (b, k) not in warps:
                warps[b, k] = R.warp_image(case['optical'][b], T, H, W)
            jh = R.joint_histogram(warps[b, k].ravel(), case['thermal'][b].ravel(), n).astype(np.float64)
            if sigma > 0:
                jh = R.gaussian_smooth(jh, sigma)
            out[False, True][b, i] = -R.score(jh, False) + np.sqrt(np.sum((case['init'][b] - T) ** 2))
            out[True, False][b, i] = -R.score(jh, True)
    return out


@functools.lru_cache(maxsize=None)
def objective_case():
    return _objective_case(BIN_COUNTS)


@functools.lru_cache(maxsize=None)
def objective_reference(sigma):
    return _objective_reference(objective_case(), sigma)


@functools.lru_cache(maxsize=None)
def mixed_case():
    return _objective_case(MIXED_BINS)


@functools.lru_cache(maxsize=None)
def mixed_reference(sigma):
    return _objective_reference(mixed_case(), sigma)


# ---- 6. Nelder-Mead ----
NM_COPIES = 10
NM_CHUNKS = (1, 7, 16)


@functools.lru_cache(maxsize=None)
def nm_case():
    """70 problems on the 40 x 56 pairs of tests/test_gpu_mi.py (objective_inputs): its seven kinds -- four plain ones, stopped
    by maxiter = 25, one that stops on maxfun, one finished by loose tolerances at the first check, one whose maxfun ends the
    initial simplex -- ten times, interleaved (problem q is of kind q % 7)."""
    Ho, Wo, H, W = 48, 64, 40, 56
    opt = np.stack([np.round(R.blob_image(3 + b, Ho, Wo, 25) * 255) / 255 for b in range(2)]).astype(np.float32)
    rng = np.random.default_rng(13)
    th = np.stack([(1.0 - R.blob_image(3 + b, Ho, Wo, 25)[:H, :W]) ** 2 + 0.05 * rng.random((H, W))
                   for b in range(2)]).astype(np.float32)
    x0 = np.array([[1.02, 0.01, 1.2], [-0.01, 0.98, -0.9], [1e-5, 0.0, 1.0]])
    # (pair, bins, maxiter, maxfun, xatol, fatol)
    kinds = [(0, 16, 25, 10 ** 6, 1e-6, 1e-6), (0, 100, 25, 10 ** 6, 1e-6, 1e-6), (1, 16, 25, 10 ** 6, 1e-6, 1e-6),
             (1, 100, 25, 10 ** 6, 1e-6, 1e-6), (0, 16, 10 ** 6, 23, 1e-6, 1e-6), (1, 100, 25, 10 ** 6, 10.0, 10.0),
             (1, 16, 10 ** 6, 7, 1e-6, 1e-6)]
    return {'optical': opt, 'thermal': th, 'x0': x0, 'kinds': kinds, 'problems': kinds * NM_COPIES}
