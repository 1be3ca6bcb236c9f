#!/usr/bin/env python3
"""Device time of SuperPointLoss forward + backward (the HIP gradient kernels) at B = 32, D = 64, 240x320 and 480x640,
in both label-noise modes (warm-up, hipEvents on the stream, median of --reps), the forward alone for comparison, the
descriptor backward's achieved FLOP/s (4 x the forward's 2 B N^2 D) against the fp32 MFMA peak (a lower bound: the time
includes the detector backward and the prologue), and next to it a torch autograd restatement of the reference's dense
formulation (B x N^2 tensors) with its time and peak memory.

    python tools/bench_loss_grad.py [--reps 20] [--json out.json] [--skip-torch]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_loss import DEV, FP32_MFMA_PEAK, make_inputs, timed  # noqa: E402
from multipoint_amd.utils.losses import SuperPointLoss  # noqa: E402


def with_grad(pred):
    """Leaves requiring grad in the layout the model returns (channels-last descriptors)."""
    out, leaves = [], []
    for p in pred:
        desc = p['desc'].permute(0, 2, 3, 1).detach().requires_grad_()
        logits = p['logits'].detach().requires_grad_()
        out.append({'logits': logits, 'desc': desc.permute(0, 3, 1, 2)})
        leaves += [desc, logits]
    return out, leaves


def torch_dense_autograd(pred, data, cfg):
    """The dense descriptor loss and the CE detector loss in torch autograd (fp32, identity-free warps as in
    bench_loss.torch_dense), forward + backward."""
    from bench_loss import torch_dense
    leaves = [p['desc'].detach().clone().requires_grad_() for p in pred]
    logits = [p['logits'].detach().clone().requires_grad_() for p in pred]
    p2 = [{'desc': leaves[s], 'logits': logits[s]} for s in range(2)]
    out = torch_dense(p2, data, cfg)
    loss = cfg['lambda'] * ((out[:, 0] + out[:, 1]) / out[:, 3]).mean()
    for s in range(2):
        B, _, Hc, Wc = logits[s].shape
        lab = torch.randint(0, 65, (B, Hc, Wc), device=DEV)
        loss = loss + torch.nn.functional.cross_entropy(logits[s], lab)
    loss.backward()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--torch-reps', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--json', default=None)
    ap.add_argument('--skip-torch', action='store_true', help='time the HIP loss only (e.g. under a profiler)')
    args = ap.parse_args()
    B, D = args.batch, 64
    results = {}
    for H, W in ((240, 320), (480, 640)):
        base, data = make_inputs(B, H, W, D)
        N = (H // 8) * (W // 8)
        r = {}
        for mode in ('host', 'device'):
            loss_fn = SuperPointLoss({'label_noise': mode})
            pred, leaves = with_grad(base)

            def step():
                loss, _ = loss_fn.evaluate(pred[0], data[0], pred[1], data[1])
                loss[0].backward()
                for t in leaves:
                    t.grad = None
            r['forward_ms_' + mode] = timed(lambda: loss_fn.evaluate(base[0], data[0], base[1], data[1]), args.reps)
            r['forward_backward_ms_' + mode] = timed(step, args.reps)
            r['backward_ms_' + mode] = r['forward_backward_ms_' + mode] - r['forward_ms_' + mode]
        flop = 4 * 2.0 * B * N * N * D
        r['backward_desc_gflop'] = flop / 1e9
        r['backward_mfma_peak_share_lower'] = flop / (r['backward_ms_device'] * 1e-3) / FP32_MFMA_PEAK
        cfg = SuperPointLoss().config
        if args.skip_torch:
            results['%dx%d' % (H, W)] = r
            print('%dx%d B=%d D=%d: %s' % (H, W, B, D, json.dumps({k: round(v, 4) for k, v in r.items()})), flush=True)
            continue
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base_mem = torch.cuda.memory_allocated(DEV)
        torch.cuda.reset_peak_memory_stats(DEV)
        try:
            r['torch_autograd_ms'] = timed(lambda: torch_dense_autograd(base, data, cfg), args.torch_reps, warmup=1)
            r['torch_autograd_peak_gb'] = (torch.cuda.max_memory_allocated(DEV) - base_mem) / 1e9
        except torch.cuda.OutOfMemoryError:
            r['torch_autograd_ms'] = None
            r['torch_autograd_peak_gb'] = 'out of memory'
        torch.cuda.empty_cache()
        results['%dx%d' % (H, W)] = r
        print('%dx%d B=%d D=%d: %s' % (H, W, B, D, json.dumps({k: (round(v, 4) if isinstance(v, float) else v)
                                                               for k, v in r.items()})), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
