#!/usr/bin/env python3
"""Look at SyntheticShapes samples (the reference's show_synthetic_images.py without a GUI): writes <i>_raw.png, the image
with its keypoints marked, and <i>_masked.png, the same with the pixels outside the valid mask darkened, into a directory."""
import argparse
import os
import random
import sys

import numpy as np
import yaml

import multipoint_amd.datasets as datasets


def build_parser():
    parser = argparse.ArgumentParser(description='Write SyntheticShapes samples as PNGs')
    parser.add_argument('-y', '--yaml-config', default='configs/config_synthetic_shapes.yaml', help='YAML config file')
    parser.add_argument('-n', '--number', default=4, type=int, help='Number of samples')
    parser.add_argument('-r', '--radius', default=2, type=int, help='Half size of the keypoint marks in pixels')
    parser.add_argument('-m', '--mask-weight', default=0.5, type=float, help='Brightness of the pixels outside the valid mask')
    parser.add_argument('-s', '--seed', default=None, type=int, help='Seed of the random generators')
    parser.add_argument('-o', '--output-dir', default='synthetic_images', help='Directory the PNGs are written to')
    return parser


def mark_keypoints(gray, keypoints, radius):
    """An RGB uint8 image with a green cross on every (y, x) keypoint."""
    rgb = np.repeat((np.clip(gray, 0.0, 1.0) * 255.0).round().astype(np.uint8)[:, :, None], 3, axis=2)
    H, W = gray.shape
    for y, x in keypoints:
        y, x = int(y), int(x)
        rgb[max(y - radius, 0):min(y + radius + 1, H), x] = (0, 255, 0)
        rgb[y, max(x - radius, 0):min(x + radius + 1, W)] = (0, 255, 0)
    return rgb


def main(argv=None):
    from PIL import Image
    args = build_parser().parse_args(argv)
    with open(args.yaml_config, 'r') as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    if args.seed is not None:
        random.seed(args.seed)
        np.random.seed(args.seed)
    dataset = datasets.SyntheticShapes(config['dataset'])
    os.makedirs(args.output_dir, exist_ok=True)
    for i in range(args.number):
        sample = dataset[i % len(dataset)]
        image = sample['image'][0].numpy()
        keypoints = sample['keypoints'].numpy()
        keypoints = np.argwhere(keypoints) if keypoints.dtype == bool else keypoints
        valid = sample['valid_mask'][0].numpy()
        Image.fromarray(mark_keypoints(image, keypoints, args.radius)).save(os.path.join(args.output_dir, '%d_raw.png' % i))
        masked = image * np.where(valid, 1.0, args.mask_weight)
        Image.fromarray(mark_keypoints(masked, keypoints, args.radius)).save(os.path.join(args.output_dir, '%d_masked.png' % i))
        print('%d: %s, %d keypoints' % (i, 'optical' if bool(sample['is_optical'][0]) else 'thermal', len(keypoints)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
