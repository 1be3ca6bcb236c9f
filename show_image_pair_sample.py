#!/usr/bin/env python3
"""Look at one sample of a pair dataset as the training sees it (the reference's show_image_pair_sample.py without its
windows): first as a single image (one spectrum drawn at random, label keypoints as blue rings of thickness 3), then as a pair
(thickness 5), each also multiplied by its valid mask.  Written to -o as <n>_single[_masked].png, <n>_optical[_masked].png and
<n>_thermal[_masked].png.  The keypoint file is optional; the pictures are drawn on the GPU (multipoint_amd.utils.drawing)."""
import argparse
import os
import sys

import torch

import multipoint_amd.datasets as datasets
from show_keypoints import write_views

BLUE = (0, 0, 255)


def build_parser():
    parser = argparse.ArgumentParser(description='Show a sample of the dataset')
    parser.add_argument('-i', '--input-file', default='/tmp/test.hdf5', help='Input dataset file')
    parser.add_argument('-k', '--keypoint-file', help='Keypoint dataset file')
    parser.add_argument('-n', dest='sample_number', type=int, default=0, help='Sample to show')
    parser.add_argument('-r', '--radius', default=4, type=int, help='Radius of the keypoint circle')
    parser.add_argument('-o', '--output-dir', default='sample_images', help='(extension, in place of the windows) directory the '
                        'PNGs are written to')
    return parser


def label_list(entry):
    return torch.nonzero(entry['keypoints'].squeeze()) if 'keypoints' in entry else None


def main(argv=None):
    args = build_parser().parse_args(argv)
    config = {'filename': args.input_file, 'keypoints_filename': args.keypoint_file, 'height': -1, 'width': -1,
              'raw_thermal': False, 'single_image': True}
    os.makedirs(args.output_dir, exist_ok=True)
    n = args.sample_number
    sample = datasets.ImagePairDataset(config)[n]
    write_views(args.output_dir, '%d_single' % n, sample['image'][0], sample['valid_mask'][0], label_list(sample), args.radius,
                BLUE, 3)
    sample = datasets.ImagePairDataset(dict(config, single_image=False))[n]
    for side in ('optical', 'thermal'):
        write_views(args.output_dir, '%d_%s' % (n, side), sample[side]['image'][0], sample[side]['valid_mask'][0],
                    label_list(sample[side]), args.radius, BLUE, 5)
    return 0


if __name__ == '__main__':
    sys.exit(main())
