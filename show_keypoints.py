#!/usr/bin/env python3
"""Look at the exported keypoint labels of one sample of a pair dataset (the reference's show_keypoints.py without its windows):
the labels of the keypoint file as green rings of radius -r on the optical and on the thermal image, written to -o as
<n>_optical.png, <n>_thermal.png and, multiplied by the sample's valid mask, <n>_optical_masked.png, <n>_thermal_masked.png.
Dataset and keypoint file are HDF5 files or .npz archives in the same layout; the pictures are drawn on the GPU
(multipoint_amd.utils.drawing)."""
import argparse
import os
import sys

import numpy as np
import torch

import multipoint_amd.datasets as datasets


def build_parser():
    parser = argparse.ArgumentParser(description='Show a sample of the dataset')
    parser.add_argument('-d', '--dataset-file', required=True, help='Input dataset file')
    parser.add_argument('-k', '--keypoint-file', required=True, help='Keypoint dataset file')
    parser.add_argument('-n', dest='sample_number', type=int, default=0, help='Sample to show')
    parser.add_argument('-r', '--radius', default=4, type=int, help='Radius of the keypoint circle')
    parser.add_argument('-o', '--output-dir', default='keypoint_images', help='(extension, in place of the windows) directory the '
                        'PNGs are written to')
    return parser


def write_views(output_dir, stem, image, valid_mask, keypoints, radius, color, thickness):
    """<stem>.png: the image with a ring on every keypoint; <stem>_masked.png: that picture times the valid mask"""
    from multipoint_amd.utils import drawing
    picture = drawing.gray_to_rgb(image.cuda() if torch.cuda.is_available() else image)      # (without a GPU this raises)
    if keypoints is not None:
        drawing.draw_keypoints(picture, keypoints, radius=radius, color=color, thickness=thickness)
    masked = picture * valid_mask.to(picture.device).reshape(1, *picture.shape[1:3], 1).to(torch.uint8)
    drawing.save_png(os.path.join(output_dir, stem + '.png'), picture)
    drawing.save_png(os.path.join(output_dir, stem + '_masked.png'), masked)


def main(argv=None):
    args = build_parser().parse_args(argv)
    from multipoint_amd.datasets.image_pair_dataset import _open_store
    dataset = datasets.ImagePairDataset({'filename': args.dataset_file, 'height': -1, 'width': -1, 'raw_thermal': False,
                                         'single_image': False})
    sample = dataset[args.sample_number]
    name = dataset.get_name(args.sample_number)
    with _open_store(args.keypoint_file) as f:
        labels = np.array(f[name]['keypoints'][...])
    print('Number of keypoints: {}'.format(labels.shape[0]))
    os.makedirs(args.output_dir, exist_ok=True)
    for side in ('optical', 'thermal'):
        write_views(args.output_dir, '%d_%s' % (args.sample_number, side), sample[side]['image'][0], sample[side]['valid_mask'][0],
                    labels.reshape(-1, 2).astype(np.int64), args.radius, (0, 255, 0), 1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
