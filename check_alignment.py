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

Phase 2   check_alignment.py -i DIR --decisions FILE
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
    return parser


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


def write_review(input_dir, review_dir, dt):
    import torch
    from align_images import read_pair
    from multipoint_amd.utils import alignment, drawing
    best = os.path.join(input_dir, 'aligned', 'best')
    os.makedirs(review_dir, exist_ok=True)
    names = pending_pairs(input_dir)
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
    with open(os.path.join(review_dir, 'decisions_template.txt'), 'wt') as fh:
        fh.write(''.join(n.split('_')[0] + ' ?\n' for n in names))
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
    if args.decisions:
        apply_decisions(args.input_dir, args.decisions)
    else:
        write_review(args.input_dir, args.review_dir or os.path.join(args.input_dir, 'review'), args.dt)
    return 0


if __name__ == '__main__':
    sys.exit(main())
