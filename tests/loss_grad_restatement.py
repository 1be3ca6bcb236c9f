"""Float64 numpy restatement of the gradient of SuperPointLoss, written from the definition of the loss (the batch means
of tests/loss_restatement.py), not from the reference's code.

Upstream gradients of values = [total, components...]: g_T and one per component key.  With lambda the descriptor
loss's weight in total:  alpha = lambda g_T + g_desc + g_pos,  beta = lambda g_T + g_desc + g_neg,  gamma_k = g_T + g_det_k.
h(x) = 1 for x > 0, 1/2 for x == 0 (torch's maximum backward at a tie), 0 for x < 0.

Fed the kernel's fp32 warped centres, the correspondence decisions are the kernel's (loss_restatement.correspondence)."""
import numpy as np

import loss_restatement as R


def hinge(x):
    return np.where(x > 0, 1.0, np.where(x == 0, 0.5, 0.0))


def upstream(keys, grads, lam):
    """(alpha, beta, gamma1, gamma2) from the upstream gradients `grads` (a dict over 'total' and the component keys;
    missing keys count 0)."""
    g = {k: float(grads.get(k, 0.0)) for k in ('total',) + tuple(keys)}
    gT = g['total']
    alpha = lam * gT + g.get('descriptor_loss', 0.0) + g.get('positive_dist', 0.0)
    beta = lam * gT + g.get('descriptor_loss', 0.0) + g.get('negative_dist', 0.0)
    return alpha, beta, gT + g.get('detector_loss1', 0.0), gT + g.get('detector_loss2', 0.0)


def softmax(lg):
    m = lg.max(1, keepdims=True)
    e = np.exp(lg - m)
    return e / R._sum(e, 1, keepdims=True)


def detector_grad(logits, keypoints, valid_mask, use_ce, gamma, noise=None, labels=None, dtype=np.float64):
    """d(mean_b(sum(loss * valid) / count))/d logits times gamma, float64 [B][65][Hc][Wc].  `labels` [B][Hc][Wc]
    overrides the labels drawn from `noise` (the device hash).  dtype=np.float32 evaluates the same formulas in float32
    with sequential sums (R.detector_loss_sums' float32 mode); the result is widened at the end."""
    lg = np.asarray(logits, dtype)
    B, _, Hc, Wc = lg.shape
    valid = R.cell_valid(valid_mask, B, 8 * Hc, 8 * Wc)
    count = valid.reshape(B, -1).sum(1).astype(np.float64)
    p = softmax(lg)
    if use_ce:
        lab = R.detector_labels(keypoints, noise) if labels is None else labels
        y = np.zeros_like(p)
        np.put_along_axis(y, lab[:, None], 1.0, 1)
        dz = p - y
    else:
        kp = R.space_to_depth(np.asarray(keypoints) != 0).astype(dtype)
        dust = 1.0 - np.minimum(kp.sum(1, keepdims=True), 1.0)
        y = np.concatenate([kp, dust], 1)
        y = y / y.sum(1, keepdims=True)
        gp = (p - y) / np.maximum(p * (1 - p), dtype(1e-12))
        dz = p * (gp - R._sum(p * gp, 1, keepdims=True))
    with np.errstate(divide='ignore', invalid='ignore'):
        scale = (gamma / (B * count)).astype(dtype)
        return (dz * valid[:, None] * scale[:, None, None, None]).astype(np.float64)


def descriptor_grad(desc1, desc2, w1, w2, valid1, valid2, config, alpha, beta):
    """(d desc1, d desc2) float64 [B][D][Hc][Wc] of alpha * (sum_pos / norm) + beta * (sum_neg / norm), batch means;
    w1 / w2 (B, N, 2) warped centres, valid (B, Hc, Wc) bool."""
    cfg = dict(R.DEFAULTS, **config)
    d1 = np.asarray(desc1, np.float64)
    B, D, Hc, Wc = d1.shape
    d1 = d1.reshape(B, D, -1)
    d2 = np.asarray(desc2, np.float64).reshape(B, D, -1)
    dot = np.einsum('bdi,bdj->bij', d2, d1)                              # [b][i side 2][j side 1]
    corr = R.correspondence(w1, w2, cfg['descriptor_loss_threshold'])[0]
    if cfg['descriptor_loss_use_mask']:
        w = (valid2.reshape(B, -1, 1) & valid1.reshape(B, 1, -1)).astype(np.float64)
        norm = valid1.reshape(B, -1).sum(1).astype(np.float64) * valid2.reshape(B, -1).sum(1)
    else:
        w = np.ones(dot.shape)
        norm = np.full(B, float(Hc * Wc) ** 2)
    c = w * corr
    with np.errstate(divide='ignore', invalid='ignore'):
        G = (-alpha * cfg['lambda_d'] * c * hinge(cfg['positive_margin'] - dot) +
             beta * (w - c) * hinge(dot - cfg['negative_margin'])) / (B * norm)[:, None, None]
    g1 = np.einsum('bij,bdi->bdj', G, d2)
    g2 = np.einsum('bij,bdj->bdi', G, d1)
    return g1.reshape(B, D, Hc, Wc), g2.reshape(B, D, Hc, Wc)


def grads(inputs, config, keys, upstream_grads, noise1=None, noise2=None, warped=None, labels=(None, None)):
    """{'logits1', 'logits2', 'desc1', 'desc2'} float64 gradients of a pair (None where the loss does not use it)."""
    cfg = dict(R.DEFAULTS, **config)
    B, H, W = inputs['keypoints1'].shape
    Hc, Wc = H // 8, W // 8
    alpha, beta, g1, g2 = upstream(keys, upstream_grads, float(cfg['lambda']))
    out = {'logits1': None, 'logits2': None, 'desc1': None, 'desc2': None}
    if cfg['detector_loss']:
        for side, gamma, noise in ((1, g1, noise1), (2, g2, noise2)):
            if 'logits%d' % side in inputs:
                out['logits%d' % side] = detector_grad(inputs['logits%d' % side], inputs['keypoints%d' % side],
                                                       inputs.get('valid_mask%d' % side),
                                                       cfg['detector_use_cross_entropy'], gamma, noise, labels[side - 1])
    if cfg['descriptor_loss']:
        if warped is None:
            warped = (R.warp_centres(inputs.get('homography1'), B, Hc, Wc), R.warp_centres(inputs.get('homography2'), B, Hc, Wc))
        v1 = R.cell_valid(inputs.get('valid_mask1'), B, H, W)
        v2 = R.cell_valid(inputs.get('valid_mask2'), B, H, W)
        out['desc1'], out['desc2'] = descriptor_grad(inputs['desc1'], inputs['desc2'], warped[0], warped[1], v1, v2, cfg,
                                                     alpha, beta)
    return out


# ---- label_noise 'device': the kernel's counter-based hash (splitmix64 finaliser) ----

_M = (1 << 64) - 1


def device_noise(seed, B, Hc, Wc):
    """The 'device' noise of one side: fp32 [B][64][Hc][Wc], u = (mix64(seed ^ mix64(idx)) >> 40) * 2^-24."""
    idx = np.arange(B * 64 * Hc * Wc, dtype=np.uint64)
    with np.errstate(over='ignore'):
        def mix(z):
            z = z + np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            return z ^ (z >> np.uint64(31))
        u = mix(np.uint64(seed & _M) ^ mix(idx)) >> np.uint64(40)
    return (u.astype(np.float64) * 2.0 ** -24).astype(np.float32).reshape(B, 64, Hc, Wc)
