#!/usr/bin/env python3
"""Correct what one global transform leaves of the pairs align_images.py wrote: measure the local residual field of
every aligned pair, fit a smooth displacement field to it, sample the aligned optical image through the field, measure again and
iterate (multipoint_amd.utils.field.correct_locally).  An extension: the reference has no such step.

    correct_alignment.py -i DIR [-y configs/config_correct_alignment.yaml] [--rounds N]

For every <index>_optical.png of DIR/aligned/best that DIR/checked.log does not list, and only where the never-worse rule applies the
correction (the pair has enough confident windows, is measurably off, ends with a smaller median residual and keeps its windows):
    DIR/aligned/all/<index>_optical_<n>.png   the corrected optical image under the next free number n, 8 bit like its input: an
                                              ordinary alternative for check_alignment.py and its --auto proposal
    DIR/corrected/<index>_field.npz           U (gy, gx, 2) = (dy, dx) at the lattice nodes, geometry (y0, x0, step), summaries
                                              (JSON: one summary of the residual field per measurement)
    DIR/corrected/<index>_before.png, <index>_after.png   the needle maps of the first and the last measurement on the thermal image
and always
    DIR/corrected/report.json                 per pair: applied, the reason, the alternative's number, the summaries; the settings
No existing file is changed.  The corrected image is the ALIGNED image sampled once more (colour images channel by channel through
the one field measured on their grey version); a pixel with a tap outside the image is written as 0, as align_images.py writes it.
Every default of the config is a guess from one planted trial; nothing here is a claim about real recordings."""
import argparse
import json
import os
import sys

import numpy as np


def build_parser():
    parser = argparse.ArgumentParser(description='Fit and apply a smooth local correction to the aligned pairs of a directory')
    parser.add_argument('-i', '--input-dir', default='/tmp/data', help='Input directory (the output directory of align_images.py)')
    parser.add_argument('-y', '--yaml-config', default=None, help='yaml with the settings (configs/config_correct_alignment.yaml; '
                        'every value in it is a guess)')
    parser.add_argument('--rounds', type=int, default=None, help='measure-fit-warp rounds (overrides the config)')
    return parser


def load_config(path=None):
    """the settings: the defaults of multipoint_amd.utils.residual and utils.field, overridden by the yaml's sections"""
    from multipoint_amd.utils import field, residual
    t, d = residual.RESIDUAL_THRESHOLDS, field.FIELD_DEFAULTS
    cfg = {'residual': {'window': 32, 'stride': 16, 'radius': 8, 'feature': 'gradient', 'ksize': 5, 'min_valid': 0.5,
                        'var_floor': residual.VAR_FLOOR},
           'confidence': {k: t[k] for k in ('min_rho', 'min_margin', 'tol_px')},
           'fit': {'rounds': d['rounds'], 'smoothness': d['smoothness'], 'weights': 'binary', 'robust_px': None, 'robust_rounds': 2,
                   'extrapolate': d['extrapolate']},
           'rule': {'min_coverage': t['min_coverage'], 'min_initial_px': d['min_initial_px'], 'keep_confident': d['keep_confident']},
           'needle_scale': 4}
    if path is not None:
        import yaml
        with open(path, 'rt') as fh:
            given = yaml.safe_load(fh) or {}
        for key, value in given.items():
            if key not in cfg:
                raise ValueError('%s: unknown key %r' % (path, key))
            if isinstance(cfg[key], dict):
                unknown = set(value) - set(cfg[key])
                if unknown:
                    raise ValueError('%s: unknown keys %s under %s' % (path, sorted(unknown), key))
                cfg[key].update(value)
            else:
                cfg[key] = value
    return cfg


def _json_safe(v):
    """NaN and the infinities as null (JSON has neither)"""
    if isinstance(v, dict):
        return {str(k): _json_safe(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_json_safe(x) for x in v]
    if isinstance(v, float) and not (v == v and abs(v) != float('inf')):
        return None
    return v


def save_corrected(path, optical, U, geometry, extrapolate):
    """the aligned optical image (uint8, grey or BGR) sampled through U, as an 8-bit PNG (rounding as align_images.save_aligned)"""
    import torch
    from PIL import Image
    from multipoint_amd.utils import field
    channels = optical[None] if optical.ndim == 2 else np.ascontiguousarray(optical.transpose(2, 0, 1))
    x = torch.from_numpy(channels.astype(np.float32)).cuda()
    w, valid = field.warp_by_field(x, np.repeat(U[None], len(channels), 0), geometry, extrapolate=extrapolate, return_valid=True)
    # a tap outside the image makes the pixel invalid: written as 0, not as a blend with the zeros outside
    out = np.where(valid.cpu().numpy() == 0, 0, np.clip(np.rint(w.cpu().numpy()), 0, 255)).astype(np.uint8)
    Image.fromarray(out[0] if optical.ndim == 2 else np.ascontiguousarray(out.transpose(1, 2, 0)[:, :, ::-1])).save(path)


def main(argv=None):
    args = build_parser().parse_args(argv)
    cfg = load_config(args.yaml_config)
    if args.rounds is not None:
        cfg['fit']['rounds'] = args.rounds
    from align_images import read_pair
    from check_alignment import alternatives, pending_pairs
    from multipoint_amd.utils import alignment, drawing, field
    best = os.path.join(args.input_dir, 'aligned', 'best')
    all_dir = os.path.join(args.input_dir, 'aligned', 'all')
    out_dir = os.path.join(args.input_dir, 'corrected')
    os.makedirs(out_dir, exist_ok=True)
    r, c, f, rule = cfg['residual'], cfg['confidence'], cfg['fit'], cfg['rule']
    report = {}
    for name in pending_pairs(args.input_dir):
        index, optical, thermal, _ = read_pair(best, name)
        o = alignment.frames_to_float(optical, single_bgr=optical.ndim == 3)[None]
        t = alignment.frames_to_float(thermal[None])
        if o.shape != t.shape:
            raise ValueError('%s: the aligned optical image is %s, the thermal image %s' % (name, tuple(o.shape[1:]), tuple(t.shape[1:])))
        res = field.correct_locally(o, t, rounds=f['rounds'], window=r['window'], stride=r['stride'], radius=r['radius'],
                                    feature=r['feature'], ksize=r['ksize'], min_valid=r['min_valid'], var_floor=r['var_floor'],
                                    min_rho=c['min_rho'], min_margin=c['min_margin'], tol_px=c['tol_px'], weight_mode=f['weights'],
                                    smoothness=f['smoothness'], robust_px=f['robust_px'], robust_rounds=f['robust_rounds'],
                                    extrapolate=f['extrapolate'], min_coverage=rule['min_coverage'],
                                    min_initial_px=rule['min_initial_px'], keep_confident=rule['keep_confident'])
        summaries = [s[0] for s in res['summaries']]
        entry = {'applied': res['applied'][0], 'reason': res['reason'][0], 'alternative': None, 'summaries': summaries}
        if res['applied'][0]:
            taken = alternatives(args.input_dir, index)
            n = max(taken) + 1 if taken else 0
            os.makedirs(all_dir, exist_ok=True)
            save_corrected(os.path.join(all_dir, '%s_optical_%d.png' % (index, n)), optical, res['U'][0], res['geometry'],
                           f['extrapolate'])
            np.savez(os.path.join(out_dir, index + '_field.npz'), U=res['U'][0], geometry=np.array(res['geometry'], np.float64),
                     summaries=json.dumps(_json_safe(summaries)))
            for tag, fld in zip(('before', 'after'), res['fields']):
                canvas = drawing.gray_to_rgb(t)[0].contiguous()
                drawing.draw_residual_field(canvas, fld, 0, cfg['needle_scale'], c['min_rho'], c['min_margin'], c['tol_px'])
                drawing.save_png(os.path.join(out_dir, '%s_%s.png' % (index, tag)), canvas)
            entry['alternative'] = n
        report[index] = entry
    with open(os.path.join(out_dir, 'report.json'), 'wt') as fh:
        json.dump(_json_safe({'config': cfg, 'pairs': report}), fh, indent=1, sort_keys=True)
    applied = sum(e['applied'] for e in report.values())
    print('Corrected {} of {} pairs; report in {}'.format(applied, len(report), os.path.join(out_dir, 'report.json')))
    return 0


if __name__ == '__main__':
    sys.exit(main())
