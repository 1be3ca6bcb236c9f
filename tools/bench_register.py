#!/usr/bin/env python3
"""Time the Fourier-Mellin registration (multipoint_amd.utils.registration) on the GPU with device events: one
pooled estimate of a batch of pairs, and its stages.

    python tools/bench_register.py [--height 480 --width 640] [--thermal-height 384 --thermal-width 512] [--batch 32]
                                   [--runs 20] [--out profiles/register_bench.json]

`estimate` is estimate_similarity_fourier on the whole batch as ONE group: both stages, the host's table uploads, read-backs of
the peaks and output allocations included.  The stages are the calls it is made of, each timed alone on the buffers of the
first: prepare (both cameras, identity), FFT (the two N x N batches), log-polar (both), FFT of the log-polar planes, cross-power
(stage 1: B pairs into one A x R plane), inverse FFT + peak (stage 1), and stage 2 as a whole (thermal prepared twice, two FFTs,
two cross-powers, two inverse FFTs, two peaks).  Each figure is the median (min, max) of --runs timed calls after 3 warm-up
calls, in microseconds per CALL (the batch, not a pair).  Bytes: the least a stage must move (inputs read once, outputs written
once), for the achieved bandwidth.  Frames are the planted scenes of tests/registration_cases.py rendered at the asked sizes.
There is no CPU fallback: without a GPU this fails."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def median_us(fn, runs, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    t.sort()
    return {'min': t[0], 'median': t[len(t) // 2], 'max': t[-1]}


def frames(B, ohw, thw):
    """B planted pairs at the asked sizes: a random smooth-edged scene per pair (rectangles and ellipses), the thermal frame
    1 - scene^0.7 under one similarity (3 degrees, the ratio of the widths) plus a shift."""
    import registration_cases as C
    rng = np.random.RandomState(0)
    scale = thw[1] / ohw[1]
    a = np.radians(3.0)
    A = scale * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    co = np.array([(ohw[1] - 1) / 2.0, (ohw[0] - 1) / 2.0])
    ct = np.array([(thw[1] - 1) / 2.0, (thw[0] - 1) / 2.0])
    T = np.eye(3)
    T[:2, :2] = A
    T[:2, 2] = ct + np.array([9.0, -6.0]) - A @ co
    Ti = np.linalg.inv(T)
    k = ohw[1] / C.OPTICAL_HW[1]                  # the scenes are laid out for 96 x 128: sample them on a finer grid
    S = np.diag([1.0 / k, 1.0 / k, 1.0])
    optical, thermal = [], []
    saved = C.SUPER
    C.SUPER = 1
    try:
        for b in range(B):
            scene = C._scene(int(rng.randint(1 << 30)))
            optical.append(C._render(scene, ohw, S))
            thermal.append(1.0 - C._render(scene, thw, S @ Ti) ** 0.7)
    finally:
        C.SUPER = saved
    return np.stack(optical).astype(np.float32), np.stack(thermal).astype(np.float32), T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--thermal-height', type=int, default=384)
    ap.add_argument('--thermal-width', type=int, default=512)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_register.py measures on the GPU only')
    import registration_cases as C
    import multipoint_amd.utils.registration as G
    from multipoint_amd.models.classic_detectors import fft2d
    B, ohw, thw = args.batch, (args.height, args.width), (args.thermal_height, args.thermal_width)
    o, t, T_true = frames(B, ohw, thw)
    od, td = torch.from_numpy(o).cuda(), torch.from_numpy(t).cuda()
    gid = np.zeros(B, np.int64)
    est = G.FourierEstimator(ohw, thw, 1)
    N, A, R = est.N, est.A, est.R
    go = torch.tensor([0, B], dtype=torch.int32, device='cuda')
    po, pt = G.register_prepare(od, N), G.register_prepare(td, N)
    fo, ft = fft2d(po), fft2d(pt)
    lo, lt = G.register_logpolar(fo, A, R), G.register_logpolar(ft, A, R)
    flo, flt = fft2d(lo), fft2d(lt)
    x1 = G.register_cross_power(flo, flt, go)
    est.add_stage1(od, td)
    est.finish_stage1()

    def stage2():
        est.x2 = None
        est.add_stage2(od, td)
        return est.finish()
    T, rep = stage2()
    c8 = 8                                            # bytes of a complex value
    fbytes = 4 * B * (ohw[0] * ohw[1] + thw[0] * thw[1])
    stages = {
        'estimate': (lambda: G.estimate_similarity_fourier(od, td, gid), None),
        'prepare': (lambda: (G.register_prepare(od, N), G.register_prepare(td, N)), fbytes + 2 * B * N * N * c8),
        'fft': (lambda: (fft2d(po), fft2d(pt)), None),
        'log-polar': (lambda: (G.register_logpolar(fo, A, R), G.register_logpolar(ft, A, R)), 2 * B * A * R * c8),
        'fft log-polar': (lambda: (fft2d(lo), fft2d(lt)), None),
        'cross-power': (lambda: G.register_cross_power(flo, flt, go), 2 * B * A * R * c8 + A * R * c8),
        'inverse fft + peak': (lambda: G.register_peak(G._correlation_surface(x1)), None),
        'stage 2': (stage2, None),
    }
    res = {'device': torch.cuda.get_device_name(0), 'optical': list(ohw), 'thermal': list(thw), 'batch': B, 'runs': args.runs,
           'plane': N, 'angles': A, 'radii': R,
           'timing': 'median (min, max) of `runs` calls after 3 warm-up calls, device events around each call, microseconds per '
                     'CALL on the whole batch; whole Python calls, table uploads and output allocation included',
           'corner_error_px': C.corner_error(T[0], T_true, ohw),
           'ratios': [float(rep.peak1[0] / rep.second1[0]), float(rep.peak2[0] / rep.second2[0])], 'branch': int(rep.branch[0])}
    try:
        res['commit'] = subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, text=True, stderr=subprocess.DEVNULL).strip()
    except Exception:
        res['commit'] = None
    res['call_us'] = {}
    for k, (fn, nbytes) in stages.items():
        r = median_us(fn, args.runs)
        if nbytes:
            r['least_bytes'] = int(nbytes)
            r['gbytes_per_s'] = nbytes / r['median'] * 1e-3
        res['call_us'][k] = r
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
