#!/usr/bin/env python3
"""Device time of SuperPointLoss (multipoint_amd.utils.losses) at B = 32, D = 64, 240x320 and 480x640, in both label-noise
modes (warm-up, hipEvents on the stream, median of --reps), the descriptor kernel alone with its share of the fp32 MFMA
peak, and next to it an independently written torch-on-GPU restatement of the reference's dense formulation
(losses.py:207-272: B x N^2 tensors) with its time and peak memory.  The outputs of the two are checked to agree.

    python tools/bench_loss.py [--reps 20] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multipoint_amd.utils.losses import SuperPointLoss, descriptor_loss_sums  # noqa: E402

DEV = torch.device('cuda:0')
FP32_MFMA_PEAK = 157.3e12          # MI355X, v_mfma_f32_32x32x2_f32 (spec)


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def random_homographies(rng, B, H, W):
    out = []
    for _ in range(B):
        c = np.array([[1, 0, -W / 2], [0, 1, -H / 2], [0, 0, 1]], np.float64)
        a, s = rng.uniform(-0.2, 0.2), rng.uniform(0.85, 1.15)
        r = np.array([[s * np.cos(a), -s * np.sin(a), rng.uniform(-10, 10)],
                      [s * np.sin(a), s * np.cos(a), rng.uniform(-10, 10)],
                      [rng.uniform(-4e-4, 4e-4), rng.uniform(-4e-4, 4e-4), 1]])
        out.append(np.linalg.inv(c) @ r @ c)
    return torch.from_numpy(np.stack(out).astype(np.float32)).to(DEV)


def make_inputs(B, H, W, D, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rng = np.random.RandomState(seed)
    Hc, Wc = H // 8, W // 8
    pred, data = [], []
    for _ in range(2):
        desc = torch.randn((B, Hc, Wc, D), device=DEV, generator=g)
        desc = desc / desc.norm(dim=-1, keepdim=True)
        pred.append({'logits': torch.randn((B, 65, Hc, Wc), device=DEV, generator=g), 'desc': desc.permute(0, 3, 1, 2)})
        valid = torch.zeros((B, 1, H, W), dtype=torch.bool, device=DEV)
        valid[:, :, 8:H - 16, 16:W - 8] = True
        data.append({'keypoints': torch.rand((B, H, W), device=DEV, generator=g) < 0.005, 'valid_mask': valid,
                     'homography': random_homographies(rng, B, H, W)})
    return pred, data


def torch_dense(pred, data, cfg, warped=None):
    """The reference's dense descriptor loss restated with torch on the GPU: warped centres, the B x N x N distance,
    correspondence, dot-product, hinge and mask tensors, then the per-image sums (lambda_d * pos, neg, count, norm).
    `warped` (2, B, N, 2) replaces the warped centres (so that the correspondence decisions are the kernel's)."""
    d1, d2 = pred[0]['desc'], pred[1]['desc']
    B, D, Hc, Wc = d1.shape
    hh, ww = torch.meshgrid(torch.arange(Hc, device=DEV), torch.arange(Wc, device=DEV), indexing='ij')
    centres = torch.stack([hh * 8.0 + 4.0, ww * 8.0 + 4.0], -1).reshape(1, -1, 2).float()
    own, valid = [], []
    for d in data:
        xy1 = torch.cat([centres.flip(-1), torch.ones_like(centres[..., :1])], -1).expand(B, -1, -1)
        p = torch.bmm(torch.linalg.inv(d['homography']), xy1.transpose(1, 2)).transpose(1, 2)
        own.append((p[..., :2] / p[..., 2:]).flip(-1))
        v = d['valid_mask'].reshape(B, Hc, 8, Wc, 8).permute(0, 1, 3, 2, 4).reshape(B, Hc * Wc, 64).all(-1)
        valid.append(v.float())
    if warped is None:
        warped = own
    dist = (warped[0][:, None, :, :] - warped[1][:, :, None, :]).norm(dim=-1)
    corr = (dist <= cfg['descriptor_loss_threshold']).float()
    del dist
    dot = torch.bmm(d2.reshape(B, D, -1).transpose(1, 2), d1.reshape(B, D, -1))
    pos = cfg['lambda_d'] * corr * torch.clamp(cfg['positive_margin'] - dot, min=0)
    neg = (1 - corr) * torch.clamp(dot - cfg['negative_margin'], min=0)
    del dot
    mask = valid[1][:, :, None] * valid[0][:, None, :]
    out = torch.stack([(pos * mask).sum((1, 2)).double(), (neg * mask).sum((1, 2)).double(),
                       (corr * mask).sum((1, 2)).double(), valid[0].sum(1).double() * valid[1].sum(1).double()], 1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    B, D = args.batch, 64
    results = {}
    for H, W in ((240, 320), (480, 640)):
        pred, data = make_inputs(B, H, W, D)
        N = (H // 8) * (W // 8)
        r = {}
        for mode in ('host', 'device'):
            loss_fn = SuperPointLoss({'label_noise': mode})
            r['loss_ms_' + mode] = timed(lambda: loss_fn.evaluate(pred[0], data[0], pred[1], data[1]), args.reps)
        cfg = SuperPointLoss().config
        v1, v2 = data[0]['valid_mask'], data[1]['valid_mask']
        hom1, hom2 = data[0]['homography'], data[1]['homography']
        ws = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)
        r['descriptor_ms'] = timed(lambda: descriptor_loss_sums(pred[0]['desc'], pred[1]['desc'], hom1, hom2, v1, v2, cfg,
                                                                workspace=ws), args.reps)
        flop = 2.0 * B * N * N * D
        r['descriptor_gflop'] = flop / 1e9
        r['descriptor_mfma_peak_share'] = flop / (r['descriptor_ms'] * 1e-3) / FP32_MFMA_PEAK
        # the host noise draw alone (CPU wall time of the reference's two torch.rand calls, into pinned memory)
        buf = torch.empty((B, 64, H // 8, W // 8), pin_memory=True)
        t0 = time.perf_counter()
        for _ in range(5):
            torch.rand(buf.shape, out=buf)
            torch.rand(buf.shape, out=buf)
        r['host_noise_draw_ms'] = (time.perf_counter() - t0) / 5 * 1e3

        # the torch restatement of the reference's formulation: time, peak memory, agreement
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(DEV)
        torch.cuda.reset_peak_memory_stats(DEV)
        ref = torch_dense(pred, data, cfg)
        torch.cuda.synchronize()
        r['torch_dense_peak_mb'] = (torch.cuda.max_memory_allocated(DEV) - base) / 2 ** 20
        r['torch_dense_ms'] = timed(lambda: torch_dense(pred, data, cfg), max(3, args.reps // 4), warmup=1)
        own = ref.cpu().numpy()
        del ref
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(DEV)
        torch.cuda.reset_peak_memory_stats(DEV)
        warped = torch.empty((2, B, N, 2), dtype=torch.float32, device=DEV)
        got = descriptor_loss_sums(pred[0]['desc'], pred[1]['desc'], hom1, hom2, v1, v2, cfg, warped=warped)
        torch.cuda.synchronize()
        r['kernel_peak_mb'] = (torch.cuda.max_memory_allocated(DEV) - base) / 2 ** 20
        # agreement: with the kernel's warped centres the decisions are the same up to pairs at the threshold (torch's
        # GPU norm may round the distance differently); each such pair moves a sum by at most lambda_d * (1 + m_p)
        ref = torch_dense(pred, data, cfg, warped=(warped[0], warped[1])).cpu().numpy()
        got = got.cpu().numpy()
        flips = np.abs(got[:, 2] - ref[:, 2])
        r['count_diff_same_centres'] = float(flips.max())
        r['count_diff_own_centres'] = float(np.abs(got[:, 2] - own[:, 2]).max())
        rel = np.abs(got[:, :2] - ref[:, :2]) / np.abs(ref[:, :2])
        r['max_rel_diff_sums'] = float(rel.max())
        allow = 1e-5 + flips[:, None] * cfg['lambda_d'] * (1 + cfg['positive_margin']) / np.abs(ref[:, :2])
        assert np.all(rel <= allow), r
        assert r['count_diff_own_centres'] <= 1e-3 * own[:, 2].max() + 2, r
        assert np.array_equal(got[:, 3], ref[:, 3]), (got[:, 3], ref[:, 3])
        results['%dx%d' % (H, W)] = r
        print('B=%d %dx%d D=%d: loss host-noise %.3f ms, device-noise %.3f ms (host draw %.2f ms CPU); descriptor kernel '
              '%.3f ms = %.1f GFLOP, %.0f %% of the fp32 MFMA peak, %.0f MB; torch dense restatement %.2f ms, peak %.0f MB; '
              'agreement: sums %.1e rel, counts +-%d (own centres +-%d)'
              % (B, H, W, D, r['loss_ms_host'], r['loss_ms_device'], r['host_noise_draw_ms'], r['descriptor_ms'],
                 r['descriptor_gflop'], 100 * r['descriptor_mfma_peak_share'], r['kernel_peak_mb'], r['torch_dense_ms'],
                 r['torch_dense_peak_mb'], r['max_rel_diff_sums'], r['count_diff_same_centres'],
                 r['count_diff_own_centres']), flush=True)
        del pred, data, ws, warped
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
