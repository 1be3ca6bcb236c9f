"""Inputs of the loss shape tests (tests/test_loss_shapes_host.py on the CPU, tests/test_gpu_loss_shapes.py on the kernels of
csrc/losses.hip) and the float64 answers of tests/loss_restatement.py and tests/loss_grad_restatement.py for them.  Plain
numpy, seeded (the host label noise alone is torch's CPU draw, as the loss makes it); every case and every answer is built
once per process (functools.lru_cache) and must not be written to.

  GRIDS                                   cell grids whose N = Hc * Wc lie one below, at and one above every multiple the kernels
                                          tile by (32, 64, 128, 256), with N = 1, single rows and single columns
  descriptor_case / descriptor_reference  exact-arithmetic descriptor inputs: entries k / 4, margins on the dot lattice, weights
                                          0 / 1, integer warped centres, upstream gradients that make the coefficients powers
                                          of two -- every sum the kernels form is exact in fp32, so they must equal float64
  random_case / descriptor_answers        the same descriptors under random homographies; the answers take the kernel's centres
  threshold_case                          pairs at squared distances 64 and 128 for the descriptor_loss_threshold sweep
  detector_case / detector_reference      logits, keypoints and masks for the detector kernels (expf / logf: a tolerance)
  detector_tolerance                      max(HEADROOM x the float32 restatement's own error, 8 fp32 ulps), relative
"""
import functools

import numpy as np

import loss_grad_restatement as RG
import loss_restatement as R

EPS32 = float(np.finfo(np.float32).eps)
GRANULES = (32, 64, 128, 256)      # other-side tile rows (D = 256 / D <= 128), forward tile edge and own cells, per-cell kernels
GRIDS = [(1, 1), (1, 31), (4, 8), (3, 11), (7, 9), (8, 8), (13, 5), (5, 19), (97, 1), (1, 127), (8, 16), (3, 43), (15, 17),
         (16, 16), (257, 1), (1, 257), (5, 77), (19, 27)]
DIMS = (64, 128, 256)

# ---- descriptor loss: exact arithmetic ----
# dots are multiples of 1/16 with |dot| <= 9/16 D <= 144; both margins lie on that lattice, so exact hinge ties occur
EXACT_CONFIG = {'detector_loss': False, 'descriptor_loss': True, 'positive_margin': 1.0, 'negative_margin': 0.25,
                'lambda_d': 256, 'descriptor_loss_threshold': 8.0, 'descriptor_loss_use_mask': True}
KEYS = ('descriptor_loss', 'positive_dist', 'negative_dist')
KA, KB = -2.0 ** -3, 2.0 ** -1     # the gradient kernel's coefficients ka = -alpha lambda_d / (B norm), kb = beta / (B norm)
LAYOUTS = ('all_valid', 'tile_edges', 'last_tile', 'empty_side', 'mask_unused')
HOMS = ('none', 'identity', 'translation', 'none_translation')
# (tx, ty) in pixels, multiples of 4; the differences between any two are (+-4, +-4), (+-4, 0) or (0, +-4), so single rows and
# single columns keep corresponding pairs
SHIFTS = [(4, 0), (0, 4), (4, 4)]
RANDOM_GRIDS = [(3, 11), (3, 43), (19, 27)]
THRESHOLDS = [0.0, -1.0, float('inf'), 8.0, float(np.sqrt(np.float32(128.0))),
              float(np.nextafter(np.sqrt(np.float32(128.0)), np.float32(0.0)))]
# (grid, layout, homography): every one has pairs at squared distance 64 and at 128 (the diagonal neighbour)
THRESHOLD_CASES = [((3, 11), 'all_valid', 'identity'), ((3, 43), 'tile_edges', 'none_shift8'),
                   ((1, 257), 'tile_edges', 'shift8_identity')]
# (grid, D) of the backward's direct C-ABI calls: one own workgroup with one live lane, a second and a third own workgroup of
# one cell behind full other-side tiles, and the 32-row tiles of D = 256 with one row in the second
STALE_CASES = [((1, 1), 64), ((3, 43), 128), ((257, 1), 64), ((3, 11), 256)]


def tile_edge_cells(N):
    """{0, N - 1} and, for every multiple m of 32 with 0 < m < N, m itself and both its neighbours (below N)"""
    s = {0, N - 1}
    for m in range(32, N, 32):
        s.update(i for i in (m - 1, m, m + 1) if i < N)
    return np.array(sorted(s))


def last_tile_cells(N):
    """the cells of the last (partial or full) 128-cell tile"""
    return np.arange(128 * ((N - 1) // 128), N)


def layout_cells(layout, N, B, rng):
    """(valid1, valid2), each (B, N) bool.  Apart from 'mask_unused' (whose mask the loss ignores) and the empty image, every
    image has the same product of valid-cell counts: one norm per case."""
    v1, v2 = np.ones((B, N), bool), np.ones((B, N), bool)
    if layout in ('tile_edges', 'empty_side'):
        for b in range(B):
            (v1 if b % 2 == 0 else v2)[b] = np.isin(np.arange(N), tile_edge_cells(N))
        if layout == 'empty_side':
            v1[1] = np.isin(np.arange(N), tile_edge_cells(N))
            v2[1] = False
    elif layout == 'last_tile':
        a = last_tile_cells(N)
        for b in range(B):
            full, half = (v1, v2) if b % 2 == 0 else (v2, v1)
            full[b] = np.isin(np.arange(N), a)
            half[b] = np.isin(np.arange(N), a[::2])
    elif layout == 'mask_unused':
        v1, v2 = rng.uniform(size=(B, N)) < 0.7, rng.uniform(size=(B, N)) < 0.5
    return v1, v2


def pixel_mask(cells, Hc, Wc):
    """(B, N) cell validity -> (B, 1, H, W) bool: an invalid cell has ONE invalid pixel, at a position that moves with the cell"""
    B, N = cells.shape
    m = np.ones((B, Hc, 8, Wc, 8), bool)
    for b, n in np.argwhere(~cells):
        p = (7 * n + 3 * b) % 64
        m[b, n // Wc, p // 8, n % Wc, p % 8] = False
    return m.reshape(B, 1, 8 * Hc, 8 * Wc)


def translation(tx, ty):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float32)


def homographies(kind, B):
    """{homography1, homography2} (absent: None).  Translations differ from image to image and side to side; a common offset of
    whole cells per image moves the centres off the frame, which the dense loss does not mind."""
    def shifts(side):
        return np.stack([translation(SHIFTS[(b + side) % 3][0] + 8 * b, SHIFTS[(b + side) % 3][1] - 16) for b in range(B)])
    eye = np.broadcast_to(np.eye(3, dtype=np.float32), (B, 3, 3)).copy()
    shift8 = np.stack([translation(8, 8)] * B)
    return {'none': {}, 'identity': {'homography1': eye, 'homography2': eye.copy()},
            'translation': {'homography1': shifts(0), 'homography2': shifts(1)},
            'none_translation': {'homography2': np.stack([translation(*SHIFTS[b % 3]) for b in range(B)])},
            'none_shift8': {'homography2': shift8}, 'shift8_identity': {'homography1': shift8, 'homography2': eye}}[kind]


def _descriptor_inputs(grid, D, layout, hom, seed):
    Hc, Wc = grid
    N = Hc * Wc
    B = 3 if layout == 'empty_side' else 2
    rng = np.random.RandomState(seed)
    inputs = {'desc%d' % s: (rng.randint(-3, 4, size=(B, D, Hc, Wc)) / 4.0).astype(np.float32) for s in (1, 2)}
    v1, v2 = layout_cells(layout, N, B, rng)
    inputs['valid_mask1'], inputs['valid_mask2'] = pixel_mask(v1, Hc, Wc), pixel_mask(v2, Hc, Wc)
    if hom == 'random':
        for s in (1, 2):
            inputs['homography%d' % s] = np.stack([R.random_homography(rng, 8 * Hc, 8 * Wc) for _ in range(B)])
    else:
        inputs.update(homographies(hom, B))
    cfg = dict(EXACT_CONFIG, descriptor_loss_use_mask=layout != 'mask_unused')
    if cfg['descriptor_loss_use_mask']:
        norms = v1.sum(1) * v2.sum(1)
        norm = int(norms[0])
    else:
        norms = np.full(B, N * N)
        norm = N * N
    # alpha = B norm 2^-11 and beta = B norm 2^-1: ka = -alpha lambda_d / (B norm) = -2^-3 and kb = 2^-1
    return {'grid': grid, 'N': N, 'B': B, 'D': D, 'layout': layout, 'hom': hom, 'inputs': inputs, 'config': cfg,
            'valid': (v1, v2), 'norms': norms, 'norm': norm, 'alpha': B * norm * 2.0 ** -11, 'beta': B * norm * 2.0 ** -1}


def descriptor_names():
    """'HcxWc-D': every grid at every D"""
    return ['%dx%d-%d' % (g + (D,)) for g in GRIDS for D in DIMS]


def _assignment(name):
    """layout and homography of a grid at a D: both rotate, so that every layout meets every D and every tile class"""
    g, D = tuple(int(v) for v in name.split('-')[0].split('x')), int(name.split('-')[1])
    gi, di = GRIDS.index(g), DIMS.index(D)
    return g, D, LAYOUTS[(gi + 2 * di) % len(LAYOUTS)], HOMS[(gi + di) % len(HOMS)], 1000 + 10 * gi + di


@functools.lru_cache(maxsize=None)
def descriptor_case(name):
    g, D, layout, hom, seed = _assignment(name)
    return _descriptor_inputs(g, D, layout, hom, seed)


def random_names():
    return ['%dx%d-%d' % (g + (D,)) for g in RANDOM_GRIDS for D in DIMS]


@functools.lru_cache(maxsize=None)
def random_case(name):
    """random homographies on a layout that keeps one norm, so that the gradient coefficients stay powers of two"""
    g, D = tuple(int(v) for v in name.split('-')[0].split('x')), int(name.split('-')[1])
    gi, di = RANDOM_GRIDS.index(g), DIMS.index(D)
    return _descriptor_inputs(g, D, LAYOUTS[(gi + di) % 2], 'random', 2000 + 10 * gi + di)


@functools.lru_cache(maxsize=None)
def threshold_case(i):
    g, layout, hom = THRESHOLD_CASES[i]
    return _descriptor_inputs(g, 64, layout, hom, 3000 + i)


@functools.lru_cache(maxsize=None)
def stale_case(i):
    g, D = STALE_CASES[i]
    return _descriptor_inputs(g, D, 'tile_edges', 'translation', 4000 + i)


def exact_centres(case):
    """(w1, w2) float64 (B, N, 2): the restatement's warped centres, WITHOUT the kernel's output"""
    Hc, Wc = case['grid']
    return tuple(R.warp_centres(case['inputs'].get('homography%d' % s), case['B'], Hc, Wc) for s in (1, 2))


def cell_valid(case):
    Hc, Wc = case['grid']
    return tuple(R.cell_valid(case['inputs']['valid_mask%d' % s], case['B'], 8 * Hc, 8 * Wc) for s in (1, 2))


def descriptor_answers(case, w1, w2, config=None, gradients=True):
    """dict(sums (B, 4), g1, g2 (B, D, Hc, Wc)) in float64 from the restatements, for the fp32 centres w1 / w2 (B, N, 2)"""
    cfg = dict(case['config'], **(config or {}))
    inp = case['inputs']
    v1, v2 = cell_valid(case)
    w1, w2 = np.asarray(w1, np.float32), np.asarray(w2, np.float32)
    out = {'sums': R.descriptor_loss_sums(inp['desc1'], inp['desc2'], w1, w2, v1, v2, cfg)[0]}
    if gradients:
        out['g1'], out['g2'] = RG.descriptor_grad(inp['desc1'], inp['desc2'], w1, w2, v1, v2, cfg, case['alpha'], case['beta'])
    return out


def _reference(case):
    w1, w2 = exact_centres(case)
    return dict(descriptor_answers(case, w1, w2), warped=np.stack([w1, w2]).astype(np.float32))


@functools.lru_cache(maxsize=None)
def descriptor_reference(name):
    """sums, g1, g2 and warped (2, B, N, 2) fp32 of an exact case"""
    return _reference(descriptor_case(name))


@functools.lru_cache(maxsize=None)
def stale_reference(i):
    return _reference(stale_case(i))


@functools.lru_cache(maxsize=None)
def threshold_reference(i, t):
    case = threshold_case(i)
    w1, w2 = exact_centres(case)
    return descriptor_answers(case, w1, w2, {'descriptor_loss_threshold': THRESHOLDS[t]}, gradients=False)['sums']


def upstream(case):
    """the gradient of evaluate()'s values [total, descriptor_loss, positive_dist, negative_dist] to call backward with"""
    return np.array([0.0, 0.0, case['alpha'], case['beta']])


def kernel_coefficients(case, norm=None):
    """(ka, kb) as desc_loss_grad_kernel evaluates them: in double, rounded to float once"""
    inv = 1.0 / (float(case['B']) * float(case['norm'] if norm is None else norm))
    return (np.float32(-case['alpha'] * float(np.float32(case['config']['lambda_d'])) * inv),
            np.float32(case['beta'] * inv))


def pair_terms(case, w1, w2, config=None):
    """(dot, corr, weight, positive term, negative term), each (B, N, N) float64 / bool: the pairs of the forward"""
    cfg = dict(case['config'], **(config or {}))
    inp = case['inputs']
    B, D, N = case['B'], case['D'], case['N']
    d1 = inp['desc1'].reshape(B, D, N).astype(np.float64)
    d2 = inp['desc2'].reshape(B, D, N).astype(np.float64)
    dot = np.matmul(d2.transpose(0, 2, 1), d1)
    corr = R.correspondence(np.asarray(w1, np.float32), np.asarray(w2, np.float32), cfg['descriptor_loss_threshold'])[0]
    v1, v2 = cell_valid(case)
    w = (v2.reshape(B, N, 1) & v1.reshape(B, 1, N)) if cfg['descriptor_loss_use_mask'] else np.ones((B, N, N), bool)
    pos = corr * w * np.maximum(0.0, cfg['positive_margin'] - dot)
    neg = (~corr) * w * np.maximum(0.0, dot - cfg['negative_margin'])
    return dot, corr, w, pos, neg


def tile_sums(x, T=128):
    """(B, N, N) -> (B, nt, nt): the sum of |x| over every T x T tile"""
    B, N, _ = x.shape
    nt = -(-N // T)
    p = np.zeros((B, nt * T, nt * T))
    p[:, :N, :N] = np.abs(x)
    return p.reshape(B, nt, T, nt, T).sum((2, 4))


# ---- detector loss ----
HEADROOM = 4.0
DETECTOR_MODES = ('ce_host', 'ce_device', 'bce')
DEVICE_SEED = 5
CLAMP_GAP = 128.0                  # expf(-128) is 0 in fp32: p = 1 for the top channel, p = 0 for the others


def detector_names():
    return ['%dx%d-%s' % (g + (m,)) for g in GRIDS for m in DETECTOR_MODES] + ['sweep-%s' % m for m in DETECTOR_MODES]


def clamp_cells(N):
    return sorted({0, N // 2, N - 1})


def _cells_to_pixels(x):
    """(B, 64, Hc, Wc) -> (B, 8 Hc, 8 Wc), the inverse of space_to_depth"""
    B, _, Hc, Wc = x.shape
    return x.reshape(B, 8, 8, Hc, Wc).transpose(0, 3, 1, 4, 2).reshape(B, 8 * Hc, 8 * Wc)


def _grid_detector_inputs(grid, mode, seed):
    """B = 2.  Logits k / 8 in [-5, 5] (every gap <= 10, every cell's loss above 1); keypoints at 2 % of the pixels, 2 to 4 of
    them in a third of the cells; a quarter of the cells invalid by one pixel, never the last cell.  BCE: image 0 holds the
    clamp cells -- one keypoint, and a top logit 128 above the largest other on a channel without one, so p is 1 there and 0
    elsewhere in fp32: both max(log, -100) and max(p (1 - p), 1e-12) act."""
    Hc, Wc = grid
    N, B = Hc * Wc, 2
    rng = np.random.RandomState(seed)
    out = {}
    for side in (1, 2):
        logits = (rng.randint(-40, 41, size=(B, 65, Hc, Wc)) / 8.0).astype(np.float32)
        kp = R.space_to_depth(rng.uniform(size=(B, 8 * Hc, 8 * Wc)) < 0.02)
        cells = rng.uniform(size=(B, N)) < 0.75
        cells[:, N - 1] = True
        for b in range(B):
            for n in rng.choice(N, size=N // 3, replace=False):
                kp[b, :, n // Wc, n % Wc] = False
                kp[b, rng.choice(64, size=rng.randint(2, 5), replace=False), n // Wc, n % Wc] = True
        if mode == 'bce':
            for n in clamp_cells(N):
                c1 = (5 * n + 3 * side) % 64
                c0 = (c1 + 1 + n) % 65
                c0 = c0 if c0 != c1 else 64
                kp[0, :, n // Wc, n % Wc] = False
                kp[0, c1, n // Wc, n % Wc] = True
                logits[0, c0, n // Wc, n % Wc] = np.delete(logits[0, :, n // Wc, n % Wc], c0).max() + CLAMP_GAP
                cells[0, n] = True
        out['logits%d' % side] = logits
        out['keypoints%d' % side] = _cells_to_pixels(kp)
        out['valid_mask%d' % side] = pixel_mask(cells, Hc, Wc)
    return out


def _sweep_detector_inputs(mode, seed):
    """B = 3 on the 8 x 8 grid.  Image 0: cell k holds its one keypoint at pixel position k of the cell (side 2: 63 - k), so
    its label is channel k.  Image 1: cell k holds its one invalid pixel at position k -- no cell is valid, the count is 0 and
    the image's loss and gradient are NaN, as the reference's.  Image 2: the cells with k % 3 == 0 are invalid by the pixel
    63 - k, and cell 5 holds all 64 keypoints."""
    Hc = Wc = 8
    rng = np.random.RandomState(seed)
    out = {}
    for side in (1, 2):
        logits = (rng.randint(-40, 41, size=(3, 65, Hc, Wc)) / 8.0).astype(np.float32)
        kp = R.space_to_depth(rng.uniform(size=(3, 64, 64)) < 0.02)
        valid = np.ones((3, 64, Hc, Wc), bool)
        kp[0] = False
        for k in range(64):
            pos = k if side == 1 else 63 - k
            kp[0, pos, k // 8, k % 8] = True
            valid[1, pos, k // 8, k % 8] = False
            if k % 3 == 0:
                valid[2, 63 - k, k // 8, k % 8] = False
        kp[2, :, 0, 5] = True
        out['logits%d' % side] = logits
        out['keypoints%d' % side] = _cells_to_pixels(kp)
        out['valid_mask%d' % side] = _cells_to_pixels(valid)[:, None]
    return out


@functools.lru_cache(maxsize=None)
def detector_case(name):
    """dict(grid, B, mode, use_ce, inputs, noise (per side: fp32 (B, 64, Hc, Wc) or None)); 'ce_host' draws the noise as the
    loss does under torch.manual_seed(seed): image 1, then image 2"""
    g, mode = name.split('-')
    gi = len(GRIDS) if g == 'sweep' else GRIDS.index(tuple(int(v) for v in g.split('x')))
    seed = 5000 + 10 * gi + DETECTOR_MODES.index(mode)
    if g == 'sweep':
        grid, inputs = (8, 8), _sweep_detector_inputs(mode, seed)
    else:
        grid = GRIDS[gi]
        inputs = _grid_detector_inputs(grid, mode, seed)
    B = inputs['logits1'].shape[0]
    noise = (None, None)
    if mode == 'ce_host':
        import torch
        state = torch.get_rng_state()
        torch.manual_seed(seed)
        noise = tuple(torch.rand((B, 64) + grid).numpy() for _ in (1, 2))
        torch.set_rng_state(state)
    elif mode == 'ce_device':
        # SuperPointLoss hashes side s (0, 1) with the seed 2 * label_noise_seed + s
        noise = tuple(RG.device_noise(2 * DEVICE_SEED + s, B, grid[0], grid[1]) for s in (0, 1))
    return {'grid': grid, 'B': B, 'mode': mode, 'use_ce': mode != 'bce', 'seed': seed, 'inputs': inputs, 'noise': noise}


def _detector_answers(case, dtype):
    out = {}
    inp = case['inputs']
    for s in (1, 2):
        args = (inp['logits%d' % s], inp['keypoints%d' % s], inp['valid_mask%d' % s], case['use_ce'])
        out['sum%d' % s], out['count%d' % s] = R.detector_loss_sums(*args, noise=case['noise'][s - 1], dtype=dtype)
        out['grad%d' % s] = RG.detector_grad(*args, 1.0, noise=case['noise'][s - 1], dtype=dtype)
    return out


@functools.lru_cache(maxsize=None)
def detector_reference(name):
    """per side: sum, count (B,), grad (B, 65, Hc, Wc) of the total loss (gamma = 1), float64"""
    return _detector_answers(detector_case(name), np.float64)


def cell_losses(case, side):
    """(B, N) float64 losses of the single cells (each cell restated as an image of its own), and their validity"""
    inp = case['inputs']
    Hc, Wc = case['grid']
    B, N = case['B'], Hc * Wc
    lg = inp['logits%d' % side].reshape(B, 65, N).transpose(0, 2, 1).reshape(B * N, 65, 1, 1)
    kp = R.space_to_depth(inp['keypoints%d' % side]).reshape(B, 64, N).transpose(0, 2, 1).reshape(B * N, 8, 8)
    noise = case['noise'][side - 1]
    if noise is not None:
        noise = noise.reshape(B, 64, N).transpose(0, 2, 1).reshape(B * N, 64, 1, 1)
    loss = R.detector_loss_sums(lg, kp, None, case['use_ce'], noise=noise)[0].reshape(B, N)
    return loss, R.cell_valid(inp['valid_mask%d' % side], B, 8 * Hc, 8 * Wc).reshape(B, N)


def _finite_max(x):
    x = np.abs(x[np.isfinite(x)])
    return float(x.max()) if x.size else 0.0


@functools.lru_cache(maxsize=None)
def detector_floor():
    """{'sum', 'grad'}: the largest difference between the restatement's float32 mode and its float64 mode over all detector
    cases, relative to the case's largest float64 value"""
    floor = {'sum': 0.0, 'grad': 0.0}
    for name in detector_names():
        ref, f32 = detector_reference(name), _detector_answers(detector_case(name), np.float32)
        for s in (1, 2):
            for kind in floor:
                a, b = ref['%s%d' % (kind, s)], f32['%s%d' % (kind, s)]
                assert np.array_equal(np.isfinite(a), np.isfinite(b))
                scale = _finite_max(a)
                if scale:
                    floor[kind] = max(floor[kind], _finite_max(a - b) / scale)
    return floor


def detector_tolerance(kind, ref):
    """The absolute tolerance for the kernel's 'sum' or 'grad' against `ref`: max(HEADROOM x the float32 restatement's own
    relative error, 8 fp32 ulps) of the largest finite reference value (sift_cases.HEADROOM, test_gpu_loss_grad.tolerance)."""
    return max(HEADROOM * detector_floor()[kind], 8.0 * EPS32) * _finite_max(np.asarray(ref, np.float64))
