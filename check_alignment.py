#!/usr/bin/env python3
"""Review the pairs align_images.py wrote and move the good ones to aligned/accepted: the reference's
create_dataset/check_alignment.py without its windows.  There a person watches optical and thermal image flicker on screen and
presses a key; here the pictures are written to files first and the decisions come back in a text file.

Phase 1   check_alignment.py -i DIR [-dt MS] [--review-dir DIR/review]
    for every <index>_optical.png of DIR/aligned/best that DIR/checked.log does not list:
      review/<index>.gif        optical and thermal image alternating every -dt ms, for ever
      review/<index>.png        a contact sheet: optical | thermal | checkerboard of both | anaglyph (optical red, thermal cyan)
      review/<index>_<i>.gif    the same flicker for every alternative DIR/aligned/all/<index>_optical_<i>.png
                                (align_images.py --save-candidates)
    and review/decisions_template.txt with one line `<index> ?` per pair.  The pictures are made on the GPU
    (multipoint_amd.utils.drawing).
    With --auto [--auto-config YAML] every pair's local residual field is measured as well:
      review/<index>_residual.png   the needle map of the best alignment on the thermal image
      review/residuals.json         the summary of the best alignment and of every alternative
      review/decisions_auto.txt     one line `<index> a|r|<digit>|?`: a PROPOSAL to copy or edit and hand to phase 2.  A digit
                                    names the alternative with the smallest median residual that passes the accept rule when
                                    the best alignment does not.  A sorting aid, not a verdict: every threshold is a guess.
    decisions_template.txt stays all `?`.

Phase 2  check_alignment.py -i DIR --decisions FILE
    FILE holds one line `<index> <decision>` per pair: a accept the best alignment, r or n reject the pair, a digit accept that
    alternative, ? leave the pair unchecked.  Accepted pairs are copied to DIR/aligned/accepted as <index>_optical.png,
    <index>_thermal.png and, when there is one, <index>_thermal_raw.png; every decided pair's optical file name is appended to
    DIR/checked.log, so that the next phase 1 leaves it out.  Needs no GPU."""
import argparse
import os
import shutil
import sys


def build_parser():
    parser = argparse.ArgumentParser(description='Write the aligned images as GIFs for review and accept / reject pairs from a decisions file')
    parser.add_argument('-i', '--input-dir', default='/tmp/data', help='Input directory')
    parser.add_argument('-dt', '--dt', type=int, default=500, help='Time to show images in ms')
    parser.add_argument('--review-dir', default=None, help='(extension, in place of the windows) directory the review pictures are '
                        'written to (default: <input-dir>/review)')
    parser.add_argument('--decisions', default=None, help='(extension, in place of the keys) file with one `<index> a|r|n|<digit>|?` '
                        'line per pair: apply the decisions instead of writing review pictures')
    parser.add_argument('--auto', action='store_true', help='(extension) phase 1 only: measure the local residual field of every pair '
                        '(multipoint_amd.utils.residual) and also write review/<index>_residual.png, review/residuals.json and '
                        'review/decisions_auto.txt, a PROPOSED decisions file -- a sorting aid, not a verdict')
    parser.add_argument('--auto-config', default=None, help='(extension) yaml with the field parameters and thresholds of --auto '
                        '(configs/config_check_alignment.yaml; every threshold in it is a guess)')
    return parser


def auto_config(path=None):
    """the settings of --auto: the defaults of multipoint_amd.utils.residual, overridden by the yaml's residual / confidence /
    decision sections"""
    from multipoint_amd.utils import residual
    t = residual.RESIDUAL_THRESHOLDS
    cfg = {'residual': {'window': 32, 'stride': 16, 'radius': 8, 'feature': 'gradient', 'ksize': 5, 'min_valid': 0.5,
                        'var_floor': residual.VAR_FLOOR, 'optical_shape': None},
           'confidence': {k: t[k] for k in ('min_rho', 'min_margin', 'tol_px')},
           'decision': {k: t[k] for k in ('min_coverage', 'accept_median_px', 'accept_p90_px', 'reject_median_px')},
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


def inside_mask(transform, thermal_hw, optical_hw):
    """uint8 (H, W): 1 where the thermal pixel's pre-image under `transform` (thermal pixel -> optical pixel) lies inside the
    optical frame: the pixels of the aligned optical image that hold image content"""
    import numpy as np
    T = np.asarray(transform, np.float64).reshape(3, 3)
    y, x = np.mgrid[0:thermal_hw[0], 0:thermal_hw[1]].astype(np.float64)
    with np.errstate(all='ignore'):
        den = T[2, 0] * x + T[2, 1] * y + T[2, 2]
        xs, ys = (T[0, 0] * x + T[0, 1] * y + T[0, 2]) / den, (T[1, 0] * x + T[1, 1] * y + T[1, 2]) / den
        return ((xs >= 0) & (xs <= optical_hw[1] - 1) & (ys >= 0) & (ys <= optical_hw[0] - 1)).astype(np.uint8)


def _json_safe(v):
    """NaN and the infinities as null (JSON has neither)"""
    if isinstance(v, dict):
        return {str(k): _json_safe(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_json_safe(x) for x in v]
    if isinstance(v, float) and not (v == v and abs(v) != float('inf')):
        return None
    return v


def auto_review(index, optical, alternative_paths, t, transforms, cfg, review_dir):
    """The residual field of the best alignment `optical` (1, H, W) and of every alternative against the thermal frame t
    (1, H, W): writes review/<index>_residual.png, returns (proposal, record for residuals.json)."""
    import numpy as np
    import torch
    from multipoint_amd.utils import alignment, drawing, residual
    frames = [optical]
    for path in alternative_paths.values():
        rgb = read_rgb(path)
        frames.append(alignment.frames_to_float(np.ascontiguousarray(rgb[:, :, ::-1]), single_bgr=True)[None])
    H, W = t.shape[1:]
    if any(tuple(f.shape) != (1, H, W) for f in frames):
        raise ValueError('%s: an alternative has another size than the thermal image' % index)
    r = cfg['residual']
    mask = None
    entry = transforms.get(index)
    if entry is not None and 'transform' in entry:
        shape = entry.get('optical_shape') or r['optical_shape'] or (H, W)
        mask = np.ones((len(frames), H, W), np.uint8)                 # (the alternatives' transforms are not recorded: no mask)
        mask[0] = inside_mask(entry['transform'], (H, W), shape)
    field = residual.residual_field(torch.cat(frames), t.expand(len(frames), -1, -1), r['window'], r['stride'], r['radius'],
                                    r['feature'], r['ksize'], mask, r['min_valid'], r['var_floor'])
    c = cfg['confidence']
    summaries = residual.summarize_residual_field(field, c['min_rho'], c['min_margin'], c['tol_px'])
    proposals = [residual.propose_decision(s, cfg['decision']) for s in summaries]
    proposal = proposals[0]
    if proposal != 'a':                                              # an alternative that passes the accept rule: the smallest median
        passing = [(summaries[k + 1]['median_mag'], i) for k, i in enumerate(alternative_paths) if proposals[k + 1] == 'a']
        if passing:
            proposal = str(min(passing)[1])
    canvas = drawing.gray_to_rgb(t)[0].contiguous()
    drawing.draw_residual_field(canvas, field, 0, cfg['needle_scale'], c['min_rho'], c['min_margin'], c['tol_px'])
    drawing.save_png(os.path.join(review_dir, index + '_residual.png'), canvas)
    record = {'proposal': proposal, 'masked': mask is not None, 'best': dict(summaries[0], proposal=proposals[0]),
              'alternatives': {str(i): dict(summaries[k + 1], proposal=proposals[k + 1]) for k, i in enumerate(alternative_paths)}}
    return proposal, record


def pending_pairs(input_dir):
    """the optical file names of aligned/best that checked.log does not list, sorted"""
    best = os.path.join(input_dir, 'aligned', 'best')
    names = sorted(f for f in os.listdir(best) if os.path.isfile(os.path.join(best, f)) and f.endswith('_optical.png'))
    log = os.path.join(input_dir, 'checked.log')
    checked = set()
    if os.path.exists(log):
        with open(log, 'rt') as fh:
            checked = {line.rstrip() for line in fh if line.strip()}
    return [n for n in names if n not in checked]


def alternatives(input_dir, index):
    """{i: path} of aligned/all/<index>_optical_<i>.png"""
    all_dir = os.path.join(input_dir, 'aligned', 'all')
    out = {}
    if os.path.isdir(all_dir):
        prefix = index + '_optical_'
        for f in os.listdir(all_dir):
            if f.startswith(prefix) and f.endswith('.png') and f[len(prefix):-4].isdigit():
                out[int(f[len(prefix):-4])] = os.path.join(all_dir, f)
    return dict(sorted(out.items()))


def read_rgb(path):
    """the file's own pixels as uint8 (H, W, 3)"""
    import numpy as np
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im.convert('RGB'), np.uint8)


def write_review(input_dir, review_dir, dt, auto=None):
    """auto: None, or the settings of --auto (auto_config)"""
    import torch
    from align_images import read_pair
    from multipoint_amd.utils import alignment, drawing
    best = os.path.join(input_dir, 'aligned', 'best')
    os.makedirs(review_dir, exist_ok=True)
    names = pending_pairs(input_dir)
    transforms, proposals, records = {}, [], {}
    if auto is not None and os.path.exists(os.path.join(input_dir, 'transforms.json')):
        import json
        with open(os.path.join(input_dir, 'transforms.json'), 'rt') as fh:
            transforms = json.load(fh)
    for name in names:
        index, optical, thermal, _ = read_pair(best, name)
        o = alignment.frames_to_float(optical, single_bgr=optical.ndim == 3)[None]
        t = alignment.frames_to_float(thermal[None])
        if o.shape != t.shape:
            raise ValueError('%s: the aligned optical image is %s, the thermal image %s' % (name, tuple(o.shape[1:]), tuple(t.shape[1:])))
        H, W = t.shape[1:]
        thermal_rgb = drawing.gray_to_rgb(t)[0].cpu().numpy()
        drawing.save_gif(os.path.join(review_dir, index + '.gif'), [read_rgb(os.path.join(best, name)), thermal_rgb], dt)
        sheet = torch.empty((1, H, 4 * W, 3), dtype=torch.uint8, device=o.device)
        drawing.gray_to_rgb(o, out=sheet)
        drawing.gray_to_rgb(t, out=sheet, offset=(0, W))
        drawing.compose(o, t, 'checker', out=sheet, offset=(0, 2 * W))
        drawing.compose(o, t, 'anaglyph', out=sheet, offset=(0, 3 * W))
        drawing.save_png(os.path.join(review_dir, index + '.png'), sheet)
        for i, path in alternatives(input_dir, index).items():
            drawing.save_gif(os.path.join(review_dir, '%s_%d.gif' % (index, i)), [read_rgb(path), thermal_rgb], dt)
        if auto is not None:
            proposal, records[index] = auto_review(index, o, alternatives(input_dir, index), t, transforms, auto, review_dir)
            proposals.append((index, proposal))
    with open(os.path.join(review_dir, 'decisions_template.txt'), 'wt') as fh:
        fh.write(''.join(n.split('_')[0] + ' ?\n' for n in names))
    if auto is not None:
        import json
        with open(os.path.join(review_dir, 'residuals.json'), 'wt') as fh:
            json.dump(_json_safe({'config': auto, 'pairs': records}), fh, indent=1, sort_keys=True)
        with open(os.path.join(review_dir, 'decisions_auto.txt'), 'wt') as fh:
            fh.write(''.join('%s %s\n' % p for p in proposals))
        print('Proposed {} of {} pairs ({} left to the reviewer) in {}'.format(
            sum(p != '?' for _, p in proposals), len(proposals), sum(p == '?' for _, p in proposals),
            os.path.join(review_dir, 'decisions_auto.txt')))
    print('Wrote the review pictures of {} pairs to {}'.format(len(names), review_dir))


def read_decisions(path):
    """[(index, decision)] with decision 'a', 'r', '?' or an int"""
    out = []
    with open(path, 'rt') as fh:
        for number, line in enumerate(fh, 1):
            parts = line.split()
            if not parts or parts[0].startswith('#'):
                continue
            if len(parts) != 2 or not (parts[1] in ('a', 'r', 'n', '?') or parts[1].isdigit()):
                raise ValueError('%s:%d: expected `<index> a|r|n|<digit>|?`, got %r' % (path, number, line.rstrip()))
            d = parts[1]
            out.append((parts[0], int(d) if d.isdigit() else 'r' if d == 'n' else d))
    return out


def apply_decisions(input_dir, decisions_file):
    best = os.path.join(input_dir, 'aligned', 'best')
    accepted_dir = os.path.join(input_dir, 'aligned', 'accepted')
    os.makedirs(accepted_dir, exist_ok=True)
    names = pending_pairs(input_dir)
    by_index = {n.split('_')[0]: n for n in names}
    accepted = 0
    for index, decision in read_decisions(decisions_file):
        if index not in by_index:
            raise ValueError('%s: no unchecked pair %s in %s' % (decisions_file, index, best))
        if decision == '?':
            continue
        name = by_index.pop(index)
        if decision != 'r':
            source = os.path.join(best, name)
            if decision != 'a':
                source = alternatives(input_dir, index).get(decision)
                if source is None:
                    raise ValueError('%s: pair %s has no alternative %d in aligned/all' % (decisions_file, index, decision))
            shutil.copyfile(source, os.path.join(accepted_dir, name))
            shutil.copyfile(os.path.join(best, index + '_thermal.png'), os.path.join(accepted_dir, index + '_thermal.png'))
            raw = os.path.join(best, index + '_thermal_raw.png')
            if os.path.exists(raw):
                shutil.copyfile(raw, os.path.join(accepted_dir, index + '_thermal_raw.png'))
            accepted += 1
        with open(os.path.join(input_dir, 'checked.log'), 'at') as fh:      # this sample is checked
            fh.write(name + '\n')
    print('Accepted {} images out of {}'.format(accepted, len(names)))
    return accepted, len(names)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.decisions and (args.auto or args.auto_config):
        print('check_alignment.py: --auto belongs to phase 1 and cannot be combined with --decisions', file=sys.stderr)
        return 2
    if args.decisions:
        apply_decisions(args.input_dir, args.decisions)
    else:
        auto = auto_config(args.auto_config) if args.auto else None
        write_review(args.input_dir, args.review_dir or os.path.join(args.input_dir, 'review'), args.dt, auto)
    return 0


if __name__ == '__main__':
    sys.exit(main())
