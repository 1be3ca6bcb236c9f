#!/usr/bin/env python3
"""Device time of the batch-statistics (training-mode) forward (MultiPoint.set_batch_statistics(True), mp_forward_batch_stats)
next to the eval-mode forward (logits + descriptors, force_return_logits) of the shipped model at B = 32, 240x320 and
480x640 (warm-up, hipEvents on the stream, median of --reps).  A profiled run splits the batch-statistics forward into its
convolutions and the BatchNorm passes (bn.stats / bn.finalize / bn.apply), and the bytes the stats and apply passes move are
set against the HBM bandwidth.

    python tools/bench_batch_stats.py [--reps 10] [--json out.json]
"""
import argparse
import collections
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import mp_oracle as O  # noqa: E402
from multipoint_amd.models import MultiPoint  # noqa: E402

DEV = torch.device('cuda:0')
HBM_PEAK = 8.0e12                  # MI355X HBM3E, bytes/s (spec)


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


def bn_pass_bytes(cfg, B, H, W):
    """Bytes read + written by bn.stats and bn.apply over the forward's BatchNorm layers (the shipped layer walk of
    forward.hip: run_forward_batch_stats; channels padded to 32, the detector's 65 channels stored with a row of 80)."""
    stage = {0: [64, 64, 128, 128], 1: [32, 64, 96, 128], 2: [8, 16, 32, 64]}[cfg.get('channel_version', 0)]
    pad = [(c + 31) // 32 * 32 for c in stage]
    layers = []                     # (pixels, channels, pooled after)
    h, w = H, W
    for s in range(4):
        for k in range(2 if cfg['double_convolution'] else 1):
            last = k == (1 if cfg['double_convolution'] else 0)
            pool = last and s < 3
            layers.append((B * h * w, pad[s], pool))
        if s < 3:
            h, w = h // 2, w // 2
    hc = 256 if cfg.get('channel_version', 0) == 0 else cfg['descriptor_size']
    npx = B * (H // 8) * (W // 8)
    layers.append((npx, 2 * hc, False))
    if cfg['final_batchnorm']:
        layers += [(npx, 80, False), (npx, cfg['descriptor_size'], False)]
    stats = sum(p * c * 4 for p, c, _ in layers)
    apply = sum(p * c * 4 + (p // 4 if pool else p) * c * 4 for p, c, pool in layers)
    return stats, apply


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    cfg = dict(O.SHIPPED_MODEL_CONFIG)
    sd = O.make_weights(0, cfg)
    net = MultiPoint(cfg)
    net.load_state_dict(sd)
    net.to(DEV)
    net.set_force_return_logits(True)
    results = {}
    for H, W in ((240, 320), (480, 640)):
        B = args.batch
        data = {'image': O.make_images(1, B, H, W).to(DEV)}
        r = {}
        with torch.no_grad():
            net.set_batch_statistics(False)
            r['eval_ms'] = timed(lambda: net(data), args.reps)
            net.set_batch_statistics(True)
            r['batch_stats_ms'] = timed(lambda: net(data), args.reps)
            net.profile(True)
            net.profile_read()
            net(data)
            prof = net.profile_read()
            net.profile(False)
        groups = collections.OrderedDict()
        for name, ms, _ in prof:
            key = name if name.startswith('bn.') else 'convolutions' if ('conv' in name) else 'other'
            groups[key] = groups.get(key, 0.0) + ms
        total = sum(groups.values())
        r['profile_ms'] = groups
        r['bn_share'] = sum(v for k, v in groups.items() if k.startswith('bn.')) / total
        sb, ab = bn_pass_bytes(net.config, B, H, W)
        r['stats_bytes'], r['apply_bytes'] = sb, ab
        r['stats_hbm_share'] = sb / (groups.get('bn.stats', float('nan')) * 1e-3) / HBM_PEAK
        r['apply_hbm_share'] = ab / (groups.get('bn.apply', float('nan')) * 1e-3) / HBM_PEAK
        results['%dx%d' % (H, W)] = r
        print('B=%d %dx%d: eval forward %.2f ms, batch-statistics forward %.2f ms (%.2fx); profiled: %s; BatchNorm passes %.0f %% '
              'of the launches; bn.stats %.2f GB at %.0f %% of HBM peak, bn.apply %.2f GB at %.0f %%'
              % (B, H, W, r['eval_ms'], r['batch_stats_ms'], r['batch_stats_ms'] / r['eval_ms'],
                 ', '.join('%s %.2f ms' % kv for kv in groups.items()), 100 * r['bn_share'], sb / 1e9,
                 100 * r['stats_hbm_share'], ab / 1e9, 100 * r['apply_hbm_share']), flush=True)
        del data
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
