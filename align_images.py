#!/usr/bin/env python3
"""Drop-in for the reference's create_dataset/align_images.py: refine the alignment of optical / thermal image pairs from a
hand-measured initial transform by maximising their mutual information -- image pyramid, optional stage on blurred frames,
full-resolution stage -- on an MI355X (multipoint_amd.utils.alignment.align_images_mutual_information).

Same surface: -y / -i / -o, <index>_optical.png and <index>_thermal.png (16 bit) in the input directory, next to an
initial_transform.yaml with the key `perspective` (3x3, thermal pixel -> optical pixel).  Pairs are aligned in batches
(--batch); all frames of a run have the same size.  Written to the output directory:

  failed.log                          the optical file name of every pair without a valid alignment
  transforms.json                     {index: {"transform": 3x3, "type": winning candidate}} of the aligned pairs; with a
                                      motion model other than the homography (--transform, alignment/model) also "model"
  aligned/best/<index>_optical.png    (save_aligned_images) the optical image warped onto the thermal frame, channel by channel
                                      with the fp32 warp of utils.alignment.warp_image, rounded to 8 bit; pixels that take part of
                                      the border are 0
  aligned/best/<index>_thermal.png    (save_aligned_images) the thermal file, copied
  aligned/all/<index>_optical_<i>.png (--save-candidates) the optical image under every valid candidate of the last stage, in
                                      candidate order: the alternatives check_alignment.py offers when the best one is rejected

and the method counters are printed in the reference's format (every stage that finds an alignment counts, as there).

Extension: `alignment_method: ecc` (or --method ecc) runs the same stages with the Nelder-Mead search switched
off and the gradient-based ECC candidate of multipoint_amd.utils.ecc in its place (type ecc_<feature>_<model>, the
alignment/ecc/ keys of the yaml); --ecc keeps the search and adds that candidate next to its results.

Differences: PNGs are read and written with PIL; a pair with a frame of one single value (no contrast: the mutual
information is the same for every transform) is not handed to the optimiser but logged as failed; the affine path
(`perspective: false`) is refused; the averaged rotation and translation the reference prints at the end are left out, they
need cv2.decomposeHomographyMat, which has no restatement in this project."""
import argparse
import json
import os
import shutil

import numpy as np
import yaml


def build_parser():
    parser = argparse.ArgumentParser(
        description='Align the image pairs of a directory by mutual information from an initial transform',
        epilog='The averaged rotation and translation of the reference (cv2.decomposeHomographyMat) are not computed. '
               'A pair with a frame of one single value is logged as failed without running the optimiser.')
    parser.add_argument('-y', '--yaml-config', default='configs/config_align_images.yaml', help='Yaml file containing the configs')
    parser.add_argument('-i', '--input-dir', default='/tmp/data', help='Input directory')
    parser.add_argument('-o', '--output-dir', default='/tmp/data/processed', help='Output directory')
    parser.add_argument('--batch', default=8, type=int, help='(extension) pairs aligned together in one batch')
    parser.add_argument('--save-candidates', action='store_true', help='(extension) also write aligned/all/<index>_optical_<i>.png, '
                        'the optical image under every valid candidate, for check_alignment.py')
    parser.add_argument('--transform', default=None, choices=['homography', 'similarity', 'affine'],
                        help='(extension) motion model the optimiser searches in; overrides the yaml key alignment/model (default '
                        'homography: all nine matrix entries).  similarity: rotation, scale and two translations; affine: the six '
                        'entries of the top two rows.  Both stay 3x3 matrices with last row (0, 0, 1) under the same warp')
    parser.add_argument('--method', default=None, choices=['mi', 'ecc'],
                        help='(extension) overrides the yaml key alignment_method.  ecc: the staged procedure with the Nelder-Mead '
                        'search switched off and the ECC candidate (gradient-based, multipoint_amd.utils.ecc) in its place')
    parser.add_argument('--ecc', action='store_true', help='(extension) with the method mi: add the ECC candidate next to the '
                        'mutual-information ones (yaml: alignment/ecc/enable and the other alignment/ecc/ keys)')
    return parser


def read_pair(input_dir, optical_name):
    """(index, optical uint8 (H, W) or BGR (H, W, 3), thermal uint16 (H, W), thermal path)"""
    from PIL import Image
    index = optical_name.split('_')[0]
    thermal_path = os.path.join(input_dir, index + '_thermal.png')
    with Image.open(os.path.join(input_dir, optical_name)) as im:
        if im.mode in ('L', 'P', '1'):
            optical = np.array(im.convert('L'), np.uint8)
        else:
            optical = np.ascontiguousarray(np.array(im.convert('RGB'), np.uint8)[:, :, ::-1])       # BGR, as cv2.imread
    with Image.open(thermal_path) as im:
        thermal = np.array(im)
    if thermal.ndim != 2:
        raise ValueError('%s: the thermal image must have one channel' % thermal_path)
    if thermal.dtype == np.uint8:
        thermal = thermal.astype(np.uint16) * 257           # 8-bit files on the 16-bit scale: v / 255 == 257 v / 65535
    elif thermal.dtype != np.uint16:
        thermal = np.clip(thermal, 0, 65535).astype(np.uint16)
    return index, optical, thermal, thermal_path


def count(counter, kind):
    """align.py:600-605"""
    counter[kind] = counter.get(kind, 0) + 1
    counter['total'] += 1


def print_counters(counter):
    """align_images.py:287-302"""
    print('---------')
    print('Alignment method counters:')
    print('  Number of pairs:             ' + str(counter['total']))
    for key in counter.keys():
        if not key == 'total':
            name = key
            if name == '0':
                name = 'init'
            print('   ' + name + ': ' + str(counter[key]))


def save_aligned(alignment, path, optical, transform, height, width):
    """the optical image (uint8, grey or BGR) under `transform` on the thermal frame, as an 8-bit PNG"""
    import torch
    from PIL import Image
    channels = optical[None] if optical.ndim == 2 else np.ascontiguousarray(optical.transpose(2, 0, 1))
    x = torch.from_numpy(channels.astype(np.float32)).cuda()[:, None]
    w = alignment.warp_image(x, transform, height, width)[:, 0].cpu().numpy()
    # a tap outside the optical frame reads -1: such a pixel is below its channel's smallest value and is written as 0
    out = np.where(w < 0, 0, np.clip(np.rint(w), 0, 255)).astype(np.uint8)
    Image.fromarray(out[0] if optical.ndim == 2 else np.ascontiguousarray(out.transpose(1, 2, 0)[:, :, ::-1])).save(path)


def main(argv=None):
    args = build_parser().parse_args(argv)
    with open(args.yaml_config, 'rt') as fh:
        params = yaml.safe_load(fh)
    if args.method is not None:
        params['alignment_method'] = args.method
    method = params.get('alignment_method', 'mi')
    if method not in ('mi', 'ecc'):
        raise ValueError('Unkown alignment method: ' + str(params['alignment_method']))
    if method == 'ecc':                                     # the same stages, the ECC candidate in place of the Nelder-Mead ones
        params['alignment/run_optimization'] = False
        params['alignment/ecc/enable'] = True
    elif args.ecc:
        params['alignment/ecc/enable'] = True
    import torch
    from multipoint_amd.utils import alignment
    if not params.get('perspective', True):
        raise NotImplementedError('perspective: false -- ' + alignment._AFFINE)
    if args.transform is not None:
        params['alignment/model'] = args.transform
    model = params.get('alignment/model', 'homography')
    os.makedirs(args.output_dir, exist_ok=True)
    names = sorted(f for f in os.listdir(args.input_dir)
                   if os.path.isfile(os.path.join(args.input_dir, f)) and 'optical' in f)
    print('Number of pairs: ' + str(len(names)))
    with open(os.path.join(args.input_dir, 'initial_transform.yaml'), 'rt') as fh:
        t_init = np.array(yaml.safe_load(fh)['perspective'], np.float64).reshape(3, 3)
    best_dir = os.path.join(args.output_dir, 'aligned', 'best')
    all_dir = os.path.join(args.output_dir, 'aligned', 'all')
    if params.get('save_aligned_images', False):
        os.makedirs(best_dir, exist_ok=True)
    if args.save_candidates:
        os.makedirs(all_dir, exist_ok=True)
    counter, transforms, failed = {'total': 0}, {}, []
    for at in range(0, len(names), max(args.batch, 1)):
        pairs = [read_pair(args.input_dir, n) + (n,) for n in names[at:at + max(args.batch, 1)]]
        live = []
        for p in pairs:
            if p[1].min() == p[1].max() or p[2].min() == p[2].max():
                failed.append(p[4])
            else:
                live.append(p)
        if not live:
            continue
        # (grey and colour optical files may share a run: each is converted on its own)
        optical = torch.stack([alignment.frames_to_float(p[1], single_bgr=p[1].ndim == 3) for p in live])
        thermal = alignment.frames_to_float(np.stack([p[2] for p in live]))
        results = alignment.align_images_mutual_information(optical, thermal, t_init, params)
        for (index, opt, th, thermal_path, name), (ok, T, kind, candidates, stages) in zip(live, results):
            for s in stages:
                if s['success']:
                    count(counter, s['type'])
            if params.get('verbose', False):
                print(index + ': ' + ', '.join('%s %dx%d %s' % (s['name'], s['shape'][0], s['shape'][1], s['type'] or 'failed')
                                               for s in stages))
            if not ok:
                failed.append(name)
                continue
            transforms[index] = {'transform': T.tolist(), 'type': kind}
            if model != 'homography':
                transforms[index]['model'] = model
            if params.get('save_aligned_images', False):
                save_aligned(alignment, os.path.join(best_dir, index + '_optical.png'), opt, T, th.shape[0], th.shape[1])
                shutil.copyfile(thermal_path, os.path.join(best_dir, index + '_thermal.png'))
            if args.save_candidates:                        # align_images.py:137-139
                for i, c in enumerate(candidates):
                    save_aligned(alignment, os.path.join(all_dir, '%s_optical_%d.png' % (index, i)), opt, c['transform'],
                                 th.shape[0], th.shape[1])
    with open(os.path.join(args.output_dir, 'failed.log'), 'wt') as fh:
        fh.write(''.join(n + '\n' for n in failed))
    with open(os.path.join(args.output_dir, 'transforms.json'), 'wt') as fh:
        json.dump(transforms, fh, indent=1, sort_keys=True)
    print_counters(counter)


if __name__ == '__main__':
    main()
