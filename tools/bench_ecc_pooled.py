#!/usr/bin/env python3
"""Time the pooled ECC refinement (multipoint_amd.utils.ecc) on the GPU with device events: one group of 32 pairs
and one of 256, next to the per-pair refinement of 3.21 on the same 32 pairs in the same session, alternating call by call.

    python tools/bench_ecc_pooled.py [--height 480 --width 640] [--thermal-height 384 --thermal-width 512] [--runs 20]
                                     [--out profiles/ecc_pooled_bench.json]

Per group size and model (similarity, homography):
  pooled.refine      estimate_shared_transform_ecc as a user calls it: blur, features, workspace, every iteration, the rejection
                     round's bookkeeping, read-backs
  pooled.iteration   16 iterations enqueued by one mp_ecc_pooled_step at eps = 0 (a sums launch, a pair launch and a group launch
                     each), divided by 16
  bytes_resident     the planes and the workspace that stay on the device between iterations
and for the 32 pairs also
  pair.refine, pair.iteration   refine_alignment_ecc_batch and mp_ecc_step on the same pairs and starts (32 problems)
  iteration_ratio    pooled.iteration / pair.iteration, medians
Each figure is the median (min, max) of the timed calls after 3 warm-up calls, microseconds per CALL on the whole group.  Frames
are the planted scenes of tests/registration_cases.py at the asked sizes (tools/bench_register.py): 32 scenes, repeated eight
times for the group of 256; every start is the planted transform 6 px (corner error, thermal pixels) off.  There is no CPU
fallback: without a GPU this fails."""
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

SCENES = 32
IT = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--thermal-height', type=int, default=384)
    ap.add_argument('--thermal-width', type=int, default=512)
    ap.add_argument('--groups', type=int, nargs='+', default=[32, 256], help='pairs per group; multiples of 32')
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ecc_pooled.py measures on the GPU only')
    import ecc_cases as C
    import registration_cases as RC
    from bench_register import frames
    from multipoint_amd import _lib
    from multipoint_amd.utils import ecc as U
    ohw, thw = (args.height, args.width), (args.thermal_height, args.thermal_width)
    o, t, T_true = frames(SCENES, ohw, thw)
    o32, t32 = torch.from_numpy(o).cuda(), torch.from_numpy(t).cuda()
    T_align = np.linalg.inv(T_true)

    def err(T):
        return RC.corner_error(np.linalg.inv(np.asarray(T, np.float64).reshape(3, 3)), T_true, ohw)
    T0 = C._start_at(T_align, thw, 6.0, err)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); out = fn(); b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3, out

    def stats(ts):
        ts = sorted(ts)
        return {'min': ts[0], 'median': ts[len(ts) // 2], 'max': ts[-1], 'n': len(ts)}

    res = {'device': torch.cuda.get_device_name(0), 'optical': list(ohw), 'thermal': list(thw), 'start_error_px': err(T0),
           'timing': 'median (min, max) of %d timed calls after 3 warm-up calls, device events around each call, microseconds per '
                     'CALL on the whole group; pooled and per-pair calls alternate call by call' % args.runs, 'groups': {}}
    try:
        res['commit'] = subprocess.check_output(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, text=True,
                                                stderr=subprocess.DEVNULL).strip()
    except Exception:
        res['commit'] = None
    for P in args.groups:
        if P % SCENES:
            raise SystemExit('--groups: multiples of %d' % SCENES)
        od, td = o32.repeat(P // SCENES, 1, 1), t32.repeat(P // SCENES, 1, 1)
        entry = {}
        for model in ('similarity', 'homography'):
            mid = U.ECC_MODELS[model][0]

            def pooled():
                return U.estimate_shared_transform_ecc(od, td, T0, None, model)
            prob = U.SharedEccProblem().add(od, td).finish()
            Tg = torch.from_numpy(np.ascontiguousarray(U.ecc_start_transform(T0, model, prob.dev).reshape(-1, 9))).to(prob.dev)
            live = torch.zeros(1, dtype=torch.int32, device=prob.dev)

            def pooled_iteration():
                prob.h.check(prob.h.lib.mp_ecc_pooled_begin(*prob._head(), None, 1, _lib.ptr(Tg), *prob._masks(), mid, 0.0, 1000000,
                                                            0.25, _lib.ptr(prob.workspace), prob.workspace.numel(), prob.stream))
                torch.cuda.synchronize()
                return timed(lambda: prob.h.check(prob.h.lib.mp_ecc_pooled_step(prob.h.ptr, _lib.ptr(prob.workspace), IT,
                                                                                _lib.ptr(live), prob.stream)))[0]
            yard = P == SCENES
            if yard:
                pair = list(range(P))
                T0s = np.tile(T0, (P, 1, 1))

                def single():
                    return U.refine_alignment_ecc_batch(od, td, pair, T0s, model)
                c = U._Prepared(od, td, pair, 'gradient', 5)
                Td = torch.from_numpy(np.ascontiguousarray(U.ecc_start_transform(T0s, model, c.dev).reshape(-1, 9))).to(c.dev)

                def single_iteration():
                    c.h.check(c.h.lib.mp_ecc_begin(*c.head(), _lib.ptr(Td), c.P, mid, 0.0, 1000000, 0.25, *c.tail()))
                    torch.cuda.synchronize()
                    return timed(lambda: c.h.check(c.h.lib.mp_ecc_step(c.h.ptr, _lib.ptr(c.workspace), IT, _lib.ptr(live), c.stream)))[0]
            for _ in range(3):
                pooled(); pooled_iteration()
                if yard:
                    single(); single_iteration()
            tp, tpi, ts, tsi = [], [], [], []
            rp = rs = None
            for i in range(args.runs):
                d, rp = timed(pooled)
                tp.append(d)
                if yard:
                    d, rs = timed(single)
                    ts.append(d)
                tpi.append(pooled_iteration() / IT)
                if yard:
                    tsi.append(single_iteration() / IT)
                print('%d pairs %s run %d: pooled %.0f us, iteration %.1f us' % (P, model, i, tp[-1], tpi[-1]), file=sys.stderr, flush=True)
            it = stats(tpi)
            m = {'parameters': U.ECC_MODELS[model][1],
                 'pooled': {'refine_us': stats(tp), 'iteration_us': it, 'iteration_us_per_pair': it['median'] / P,
                            'bytes_resident': prob.bytes_resident(), 'iterations': int(rp.nit[0]), 'rounds': int(rp.rounds),
                            'success': bool(rp.success[0]), 'converged': bool(rp.converged[0]), 'rejected': int(rp.rejected.sum()),
                            'corner_error_px': err(rp.transform[0])}}
            if yard:
                e = [err(T) for T in rs['transform']]
                m['pair'] = {'refine_us': stats(ts), 'iteration_us': stats(tsi), 'iterations': [int(v) for v in rs['nit']],
                             'rounds': int(rs['rounds']), 'success': int(rs['success'].sum()),
                             'corner_error_px': {'min': min(e), 'median': float(np.median(e)), 'max': max(e)}}
                m['iteration_ratio'] = it['median'] / stats(tsi)['median']
            entry[model] = m
            del prob
        res['groups'][str(P)] = entry
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
