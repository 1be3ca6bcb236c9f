#!/usr/bin/env python3
"""Time the ECC refinement (multipoint_amd.utils.ecc) on the GPU with device events, next to the existing
mutual-information search on the same pairs and starts in the same session, alternating.

    python tools/bench_ecc.py [--height 480 --width 640] [--thermal-height 384 --thermal-width 512] [--batch 32] [--runs 20]
                              [--mi-runs 20] [--bins 32] [--out profiles/ecc_bench.json]

Per model (similarity, homography):
  ecc.refine      refine_alignment_ecc_batch as a user calls it: blur, features, workspace, every iteration, read-backs
  ecc.iteration   16 iterations enqueued by one mp_ecc_step at eps = 0 (one sums launch and one solve launch each), divided by 16
  mi.refine       refine_alignment_batch(bins, model) from the same starts
Each figure is the median (min, max) of the timed calls after 3 warm-up calls (1 for the MI search), microseconds per CALL on
the whole batch; *_per_pair divides by the batch.  least_bytes: what one sums pass must move -- the template once (4 B per
pixel), the packed image once (16 B per pixel), the partial sums -- against the iteration time (solve launch included), so the
rate is a lower bound of the sums kernel's.  Frames are the planted scenes of tests/registration_cases.py at the asked sizes
(tools/bench_register.py); every start is the planted transform 6 px (corner error, thermal pixels) off.  The corner errors of
both engines' results are recorded.  There is no CPU fallback: without a GPU this fails."""
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--thermal-height', type=int, default=384)
    ap.add_argument('--thermal-width', type=int, default=512)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--mi-runs', type=int, default=20)
    ap.add_argument('--bins', type=int, default=32)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ecc.py measures on the GPU only')
    import ecc_cases as C
    import registration_cases as RC
    from bench_register import frames
    from multipoint_amd import _lib
    from multipoint_amd.utils import alignment as A
    from multipoint_amd.utils import ecc as U
    B, ohw, thw = args.batch, (args.height, args.width), (args.thermal_height, args.thermal_width)
    o, t, T_true = frames(B, ohw, thw)
    od, td = torch.from_numpy(o).cuda(), torch.from_numpy(t).cuda()
    T_align = np.linalg.inv(T_true)

    def err(T):
        return RC.corner_error(np.linalg.inv(np.asarray(T, np.float64).reshape(3, 3)), T_true, ohw)
    T0 = np.tile(C._start_at(T_align, thw, 6.0, err), (B, 1, 1))
    pair = list(range(B))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); out = fn(); b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3, out

    def stats(ts):
        ts = sorted(ts)
        return {'min': ts[0], 'median': ts[len(ts) // 2], 'max': ts[-1], 'n': len(ts)}

    res = {'device': torch.cuda.get_device_name(0), 'optical': list(ohw), 'thermal': list(thw), 'batch': B, 'bins': args.bins,
           'start_error_px': err(T0[0]),
           'timing': 'median (min, max) of the timed calls after warm-up, device events around each call, microseconds per CALL '
                     'on the whole batch; the two engines alternate call by call', 'models': {}}
    try:
        res['commit'] = subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, text=True,
                                                stderr=subprocess.DEVNULL).strip()
    except Exception:
        res['commit'] = None
    IT = 16
    for model in ('similarity', 'homography'):
        def ecc():
            return U.refine_alignment_ecc_batch(od, td, pair, T0, model)

        def mi():
            return A.refine_alignment_batch(od, td, pair, [args.bins] * B, T0, normalized_mi=True, model=model)
        c = U._Prepared(od, td, pair, 'gradient', 5)
        Td = torch.from_numpy(np.ascontiguousarray(U.ecc_start_transform(T0, model, c.dev).reshape(-1, 9))).to(c.dev)
        live = torch.zeros(1, dtype=torch.int32, device=c.dev)

        def iteration():
            c.h.check(c.h.lib.mp_ecc_begin(*c.head(), _lib.ptr(Td), c.P, U.ECC_MODELS[model][0], 0.0, 1000000, 0.25, *c.tail()))
            torch.cuda.synchronize()
            return timed(lambda: c.h.check(c.h.lib.mp_ecc_step(c.h.ptr, _lib.ptr(c.workspace), IT, _lib.ptr(live), c.stream)))[0]
        for _ in range(3):
            ecc(); iteration()
        mi()
        te, tm, ti = [], [], []
        re = rm = None
        for i in range(max(args.runs, args.mi_runs)):
            if i < args.runs:
                d, re = timed(ecc)
                te.append(d)
                ti.append(iteration() / IT)
            if i < args.mi_runs:
                d, rm = timed(mi)
                tm.append(d)
            print('%s run %d: ecc %.0f us, mi %.0f us' % (model, i, te[-1], tm[-1]), file=sys.stderr, flush=True)
        K = U.ECC_MODELS[model][1]
        chunks = (thw[0] * thw[1] + 4095) // 4096
        least = B * (4 * thw[0] * thw[1] + 16 * ohw[0] * ohw[1] + 8 * chunks * U.ecc_sum_count(model))
        e_ecc = [err(T) for T in re['transform']]
        e_mi = [err(T) for T in rm['transform']]
        it = stats(ti)
        res['models'][model] = {
            'parameters': K,
            'ecc': {'refine_us': stats(te), 'refine_us_per_pair': stats(te)['median'] / B, 'iteration_us': it,
                    'iteration_us_per_pair': it['median'] / B, 'least_bytes_per_iteration': int(least),
                    'gbytes_per_s': least / it['median'] * 1e-3, 'iterations': [int(v) for v in re['nit']],
                    'rounds': int(re['rounds']), 'success': int(re['success'].sum()), 'converged': int(re['converged'].sum()),
                    'corner_error_px': {'min': min(e_ecc), 'median': float(np.median(e_ecc)), 'max': max(e_ecc)}},
            'mi': {'refine_us': stats(tm), 'refine_us_per_pair': stats(tm)['median'] / B, 'rounds': int(rm['rounds']),
                   'round_us': stats(tm)['median'] / max(int(rm['rounds']), 1),
                   'iterations': {'min': int(rm['nit'].min()), 'max': int(rm['nit'].max())}, 'success': int(rm['success'].sum()),
                   'corner_error_px': {'min': min(e_mi), 'median': float(np.median(e_mi)), 'max': max(e_mi)}}}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
