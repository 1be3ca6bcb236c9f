"""Float64 numpy restatement of SuperPointLoss (reference multipoint/utils/losses.py:85-122, 207-272), written from the
reference's definition, and the deterministic inputs of the loss golden cases (tests/golden/make_golden_loss.py).

The descriptor loss can take given warped cell centres: fed the fp32 centres the kernel returns, it takes the
correspondence decisions the kernel must take (dist = sqrt_rn(dy*dy + dx*dx) in fp32, each operation rounded)."""
import numpy as np

# the five components of a pair, in the order the golden file stores them
COMPONENTS = ('detector_loss1', 'detector_loss2', 'descriptor_loss', 'positive_dist', 'negative_dist')
DEFAULTS = {'detector_loss': True, 'detector_use_cross_entropy': True, 'descriptor_loss': True,
            'descriptor_loss_threshold': 8.0, 'descriptor_loss_use_mask': True, 'positive_margin': 1.0,
            'negative_margin': 0.2, 'lambda_d': 250, 'lambda': 0.0001}


def space_to_depth(x):
    """(B, H, W) -> (B, 64, Hc, Wc), channel 8*dy + dx (utils.py:71-76)."""
    B, H, W = x.shape
    return x.reshape(B, H // 8, 8, W // 8, 8).transpose(0, 2, 4, 1, 3).reshape(B, 64, H // 8, W // 8)


def cell_valid(valid_mask, B, H, W):
    """(B, Hc, Wc) bool: every pixel of the cell valid; None -> all cells."""
    if valid_mask is None:
        return np.ones((B, H // 8, W // 8), bool)
    return space_to_depth(np.asarray(valid_mask).reshape(B, H, W) != 0).all(1)


def _sum(x, axis, keepdims=False):
    """float64: numpy's sum.  float32: the terms added one after the other in float32, as a loop over them does."""
    if x.dtype == np.float64:
        return x.sum(axis, keepdims=keepdims)
    s = np.take(np.cumsum(x, axis, dtype=x.dtype), -1, axis)
    return np.expand_dims(s, axis) if keepdims else s


def _logsumexp(x, axis):
    m = x.max(axis, keepdims=True)
    return (m + np.log(_sum(np.exp(x - m), axis, keepdims=True))).squeeze(axis)


def detector_labels(keypoints, noise):
    """argmax([3 kp + noise, 2.0]) over the 65 channels in fp32 (first maximum), losses.py:103-108."""
    kp = space_to_depth(np.asarray(keypoints) != 0).astype(np.float32)
    v = np.float32(3.0) * kp + np.asarray(noise, np.float32)
    B, _, Hc, Wc = v.shape
    v = np.concatenate([v, np.full((B, 1, Hc, Wc), 2.0, np.float32)], 1)
    return v.argmax(1)


def detector_loss_sums(logits, keypoints, valid_mask, use_ce, noise=None, dtype=np.float64):
    """Per image (sum of loss * valid, count of valid cells) in float64.  dtype=np.float32 evaluates the same formulas in
    float32 with sequential sums (the measure of what float32 arithmetic alone costs); the result is widened at the end."""
    lg = np.asarray(logits, dtype)
    B, _, Hc, Wc = lg.shape
    valid = cell_valid(valid_mask, B, 8 * Hc, 8 * Wc)
    if use_ce:
        label = detector_labels(keypoints, noise)
        loss = _logsumexp(lg, 1) - np.take_along_axis(lg, label[:, None], 1)[:, 0]
    else:
        kp = space_to_depth(np.asarray(keypoints) != 0).astype(dtype)
        dust = 1.0 - np.minimum(kp.sum(1, keepdims=True), 1.0)
        y = np.concatenate([kp, dust], 1)
        y = y / y.sum(1, keepdims=True)
        p = np.exp(lg - _logsumexp(lg, 1)[:, None])
        with np.errstate(divide='ignore'):
            loss = -_sum(y * np.maximum(np.log(p), -100) + (1 - y) * np.maximum(np.log1p(-p), -100), 1)
    loss = np.where(valid, loss, 0.0).astype(dtype)
    return _sum(loss.reshape(B, -1), 1).astype(np.float64), valid.reshape(B, -1).sum(1).astype(np.float64)


def cell_centres(Hc, Wc):
    """(Hc*Wc, 2) cell centres (8h + 4, 8w + 4), row-major."""
    hh, ww = np.meshgrid(np.arange(Hc), np.arange(Wc), indexing='ij')
    return np.stack([hh * 8.0 + 4.0, ww * 8.0 + 4.0], -1).reshape(-1, 2)


def warp_centres(homography, B, Hc, Wc):
    """(B, N, 2) centres (y, x) warped by inverse(homography) in float64 (warp_points_pytorch, homographies.py:348-356)."""
    c = cell_centres(Hc, Wc)
    if homography is None:
        return np.broadcast_to(c, (B,) + c.shape).copy()
    hinv = np.linalg.inv(np.asarray(homography, np.float64))
    p = np.concatenate([c[:, ::-1], np.ones((len(c), 1))], 1)             # (x, y, 1)
    q = np.einsum('bij,nj->bni', hinv, p)
    return (q[..., :2] / q[..., 2:])[..., ::-1]


def correspondence(w1, w2, threshold):
    """corr[b, i, j] = |w1[j] - w2[i]| <= threshold; fp32 centres are compared as fp32 arithmetic (rounded products and
    sum, correctly rounded sqrt), anything else in float64.  Also returns the distances."""
    if w1.dtype == np.float32 and w2.dtype == np.float32:
        d = w1[:, None, :, :] - w2[:, :, None, :]
        s = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        dist = np.sqrt(s)
        return dist <= np.float32(threshold), dist
    d = np.asarray(w1, np.float64)[:, None] - np.asarray(w2, np.float64)[:, :, None]
    dist = np.sqrt((d * d).sum(-1))
    return dist <= threshold, dist


def descriptor_loss_sums(desc1, desc2, w1, w2, valid1, valid2, config):
    """Per image (positive sum incl. lambda_d, negative sum, corresponding valid pairs, normalisation) in float64, plus
    the distances.  desc (B, D, Hc, Wc); w1 / w2 (B, N, 2) warped centres; valid (B, Hc, Wc) bool."""
    cfg = dict(DEFAULTS, **config)
    d1 = np.asarray(desc1, np.float64)
    B, D, Hc, Wc = d1.shape
    d1 = d1.reshape(B, D, -1)
    d2 = np.asarray(desc2, np.float64).reshape(B, D, -1)
    dot = np.einsum('bdi,bdj->bij', d2, d1)
    corr, dist = correspondence(w1, w2, cfg['descriptor_loss_threshold'])
    pos = cfg['lambda_d'] * corr * np.maximum(0.0, cfg['positive_margin'] - dot)
    neg = (~corr) * np.maximum(0.0, dot - cfg['negative_margin'])
    if cfg['descriptor_loss_use_mask']:
        m = valid2.reshape(B, -1, 1) & valid1.reshape(B, 1, -1)
        norm = valid1.reshape(B, -1).sum(1).astype(np.float64) * valid2.reshape(B, -1).sum(1)
    else:
        m = np.ones_like(corr)
        norm = np.full(B, float(Hc * Wc) ** 2)
    out = np.stack([(pos * m).reshape(B, -1).sum(1), (neg * m).reshape(B, -1).sum(1),
                    (corr & m).reshape(B, -1).sum(1).astype(np.float64), norm], 1)
    return out, dist, m


def components(det1, det2, desc):
    """The reference's batch means (losses.py:122, 270-272) of the per-image sums: (total, dict)."""
    comp = {}
    total = 0.0
    for k, d in (('detector_loss1', det1), ('detector_loss2', det2)):
        if d is not None:
            comp[k] = float(np.mean(d[0] / d[1]))
            total += comp[k]
    if desc is not None:
        comp['descriptor_loss'] = float(np.mean((desc[:, 0] + desc[:, 1]) / desc[:, 3]))
        comp['positive_dist'] = float(np.mean(desc[:, 0] / desc[:, 3]))
        comp['negative_dist'] = float(np.mean(desc[:, 1] / desc[:, 3]))
    return total, comp


def loss(inputs, config, noise1=None, noise2=None, warped=None):
    """(total, components, descriptor sums) of a pair; inputs as make_case_inputs returns them."""
    cfg = dict(DEFAULTS, **config)
    B, H, W = inputs['keypoints1'].shape
    Hc, Wc = H // 8, W // 8
    det1 = det2 = desc = None
    if cfg['detector_loss']:
        det1 = detector_loss_sums(inputs['logits1'], inputs['keypoints1'], inputs.get('valid_mask1'),
                                  cfg['detector_use_cross_entropy'], noise1)
        det2 = detector_loss_sums(inputs['logits2'], inputs['keypoints2'], inputs.get('valid_mask2'),
                                  cfg['detector_use_cross_entropy'], noise2)
    if cfg['descriptor_loss']:
        if warped is None:
            warped = (warp_centres(inputs.get('homography1'), B, Hc, Wc), warp_centres(inputs.get('homography2'), B, Hc, Wc))
        v1 = cell_valid(inputs.get('valid_mask1'), B, H, W)
        v2 = cell_valid(inputs.get('valid_mask2'), B, H, W)
        desc = descriptor_loss_sums(inputs['desc1'], inputs['desc2'], warped[0], warped[1], v1, v2, cfg)[0]
    total, comp = components(det1, det2, desc)
    if desc is not None:
        total += cfg['lambda'] * comp['descriptor_loss']
    return total, comp, desc


# ---- golden cases: inputs are exact fp32 values on coarse grids (logits k/8, descriptors k/64 with |k| <= 127), so every
# ---- dot product of D <= 256 terms is exact in fp32 whatever the summation order

CASES = [
    # name,              seed, B,  H,   W,   D,  ce,    mask,  hom,        thr, multi
    ('ce_mask_random',    11, 2,  64,  96,  64, True,  True,  'random',   4.0, False),
    ('bce_mask_identity', 12, 2,  64,  96,  64, False, True,  'identity', 8.0, False),
    ('ce_nomask_identity', 13, 2, 64,  96,  64, True,  False, 'identity', 8.0, False),
    ('bce_nomask_random', 14, 2,  64,  96,  64, False, False, 'random',   4.0, False),
    ('ce_d128_random',    15, 2,  64,  96, 128, True,  True,  'random',   4.0, False),
    ('ce_multi_keypoint', 16, 2,  64,  96,  64, True,  True,  'random',   8.0, True),
    ('ce_none_hom',       17, 2,  64,  96,  64, True,  True,  'none',     8.0, False),
    ('ce_240x320',        18, 1, 240, 320,  64, True,  True,  'random',   8.0, False),
]


def case_config(case):
    name, seed, B, H, W, D, ce, mask, hom, thr, multi = case
    return {'detector_use_cross_entropy': ce, 'descriptor_loss_use_mask': mask, 'descriptor_loss_threshold': thr}


def random_homography(rng, H, W):
    """A homography near the identity that moves points by a few cells (pixel coordinates (x, y, 1))."""
    c = np.array([[1, 0, -W / 2], [0, 1, -H / 2], [0, 0, 1]], np.float64)
    a = rng.uniform(-0.2, 0.2)
    s = rng.uniform(0.85, 1.15)
    r = np.array([[s * np.cos(a), -s * np.sin(a), rng.uniform(-10, 10)],
                  [s * np.sin(a), s * np.cos(a), rng.uniform(-10, 10)],
                  [rng.uniform(-4e-4, 4e-4), rng.uniform(-4e-4, 4e-4), 1]])
    return (np.linalg.inv(c) @ r @ c).astype(np.float32)


def make_case_inputs(case):
    """Deterministic inputs of one golden case (numpy's legacy RandomState: stable across versions)."""
    name, seed, B, H, W, D, ce, mask, hom, thr, multi = case
    rng = np.random.RandomState(seed)
    Hc, Wc = H // 8, W // 8
    out = {}
    for side in (1, 2):
        logits = rng.randint(-40, 41, size=(B, 65, Hc, Wc)).astype(np.int8)
        desc = rng.randint(-127, 128, size=(B, D, Hc, Wc)).astype(np.int8)
        kp = rng.uniform(size=(B, H, W)) < 0.01
        if multi:
            # cells holding 2-4 keypoints whose logits differ strongly: a wrong tie-break moves the loss
            for b in range(B):
                for cell in rng.choice(Hc * Wc, size=Hc * Wc // 3, replace=False):
                    hc, wc = divmod(int(cell), Wc)
                    kp[b, hc * 8:hc * 8 + 8, wc * 8:wc * 8 + 8] = False
                    for c in rng.choice(64, size=rng.randint(2, 5), replace=False):
                        kp[b, hc * 8 + c // 8, wc * 8 + c % 8] = True
                        logits[b, c, hc, wc] = rng.choice([-40, 40])
        valid = np.zeros((B, 1, H, W), bool)
        for b in range(B):
            t, l = rng.randint(0, 12), rng.randint(0, 12)
            bo, r = rng.randint(0, 12), rng.randint(0, 12)
            valid[b, 0, t:H - bo, l:W - r] = True
        out['logits%d_q' % side] = logits
        out['desc%d_q' % side] = desc
        out['keypoints%d' % side] = kp
        out['valid_mask%d' % side] = valid
        if hom == 'random':
            out['homography%d' % side] = np.stack([random_homography(rng, H, W) for _ in range(B)])
        elif hom == 'identity':
            out['homography%d' % side] = np.broadcast_to(np.eye(3, dtype=np.float32), (B, 3, 3)).copy()
    return out


def dequantize(q):
    """Stored golden inputs -> the fp32 inputs of the loss."""
    out = {}
    for k, v in q.items():
        if k.startswith('logits') and k.endswith('_q'):
            out[k[:-2]] = v.astype(np.float32) * np.float32(0.125)
        elif k.startswith('desc') and k.endswith('_q'):
            out[k[:-2]] = v.astype(np.float32) * np.float32(1 / 64)
        else:
            out[k] = v
    return out
