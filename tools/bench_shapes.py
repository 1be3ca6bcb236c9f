#!/usr/bin/env python3
"""SyntheticShapes generation (mp_shapes_render + mp_shapes_finish) at the default 960x1280 -> 240x320: milliseconds per
image by primitive and over the nine together, for batches of 1 and 32 in both noise modes, and the host's plan-drawing
time separately.

The plans of a batch are drawn once (timed on the host: every random / np.random call of the reference, in 'host' mode
the 960x1280 float64 field too) and replayed: the device time is hipEvents on the stream around render + finish, after
warm-up, the median of --reps replays.  draw_checkerboard plans need the mean of their rendered background; the replay
reuses the plans drawn with it.  The upload of the host-mode noise fields (9.8 MB per image) is part of the timed replay.

    python tools/bench_shapes.py [--reps 10] [--batches 1 32] [--json out.json]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multipoint_amd.datasets import synthetic_shapes as SS  # noqa: E402

DEV = torch.device('cuda:0')


def measure(primitives, batch, noise, reps, warmup):
    cfg = {'primitives': primitives, 'generation': {'noise': noise},
           'augmentation': {'photometric': {'enable': False}, 'homographic': {'enable': False}}}
    ds = SS.SyntheticShapes(cfg)
    H, W = ds.config['generation_size']
    canvas = torch.empty((batch, H, W), dtype=torch.float32, device=DEV)
    mean = torch.zeros((batch,), dtype=torch.float64, device=DEV)
    random.seed(0)
    np.random.seed(0)
    plans, flags, t_draw = [], [], 0.0

    def background_mean(plan):                       # outside the host time: it waits for the device
        nonlocal t_draw
        t0 = time.perf_counter()
        SS.render(canvas[:1], mean[:1], [plan.commands], plan.fields)
        m = float(mean[0].item())
        t_draw -= time.perf_counter() - t0
        return m
    for _ in range(batch):
        t0 = time.perf_counter()
        plan, is_optical, _ = ds.draw_plan(background_mean)
        t_draw += time.perf_counter() - t0
        plans.append(plan)
        flags.append(is_optical)
    fields, base = [], []
    for p in plans:
        base.append(len(fields))
        fields.extend(p.fields)
    proc = ds.config['processing']
    blur2 = [proc['additional_ir_blur_size'] if not o else 0 for o in flags]
    cache = {}

    def replay():
        SS.render(canvas, mean, [p.commands for p in plans], fields, base, cache=cache)
        return SS.finish(canvas, [proc['blur_size']] * batch, blur2, ds.config['image_size'], cache=cache)
    for _ in range(warmup):
        replay()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        replay()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {'device_ms_per_image': float(np.median(ms)) / batch, 'device_ms_per_image_min': float(np.min(ms)) / batch,
            'host_plan_ms_per_image': t_draw * 1e3 / batch,
            'commands_per_image': sum(len(p.commands) for p in plans) / batch}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 32])
    ap.add_argument('--noise', nargs='+', default=['host', 'device'])
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    res = {}
    for noise in args.noise:
        for batch in args.batches:
            for prims in [[p] for p in SS.SyntheticShapes.all_primitives] + ['all']:
                name = prims if prims == 'all' else prims[0]
                r = measure(prims, batch, noise, args.reps, args.warmup)
                res['%s/%d/%s' % (noise, batch, name)] = r
                print('%-6s batch %2d %-24s device %8.3f ms / image (min %8.3f)  host plan %7.2f ms / image  %6.1f commands'
                      % (noise, batch, name, r['device_ms_per_image'], r['device_ms_per_image_min'],
                         r['host_plan_ms_per_image'], r['commands_per_image']), flush=True)
                if args.json:
                    with open(args.json, 'w') as f:
                        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
