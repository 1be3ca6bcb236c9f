#!/usr/bin/env python3
"""The pixel work of the reference's create_dataset/extract_images.py (ImageExtractorRos.preprocess_images) on raw frames that
are already files: lens undistortion of both cameras, the 180-degree rotation of the thermal frame, the down-scale of the
optical frame to the thermal height, the 1 % / 99 % outlier rejection and min-max normalisation of the 16-bit thermal frame --
on an MI355X (multipoint_amd.utils.frames.prepare_frames).  Reading the bag, pairing frames by time stamp, the exposure-time
compensation and the pose filter need ROS and are not rebuilt.

Surface as align_images.py: -y / -i / -o.  The input directory holds <index>_optical_raw.png (8-bit colour) and
<index>_thermal_raw.png (16 bit) and, with undistort_images, the calibration file named by image/calibration_params.  Written
to OUTPUT_DIR/preprocessed, the reference's three files per pair:

  <index>_optical.png        the prepared optical frame (8-bit colour)
  <index>_thermal_raw.png    the thermal frame in sensor counts (16 bit) -- with outlier rejection the CLIPPED frame, as the
                             reference writes it
  <index>_thermal.png        the rescaled thermal frame times 65535 (16 bit)

so that `align_images.py -i OUTPUT_DIR/preprocessed` runs on them (next to an initial_transform.yaml).  Pairs are prepared in
batches (--batch); the frames of one batch have the same sizes.  PNGs are read and written with PIL."""
import argparse
import os

import numpy as np
import yaml

IGNORED_PREFIXES = ('rosbag/', 'rosgab/')
IGNORED_KEYS = ('check_pose', 'compensate_exposure_time', 'image/show_raw/dt')
SUFFIX = '_optical_raw.png'


def build_parser():
    parser = argparse.ArgumentParser(description='Prepare raw optical / thermal frames: undistort, rotate, down-scale, rescale')
    parser.add_argument('-y', '--yaml-config', default='configs/config_prepare_images.yaml', help='Yaml file containing the configs')
    parser.add_argument('-i', '--input-dir', default='/tmp/data', help='Input directory')
    parser.add_argument('-o', '--output-dir', default='/tmp/data/processed', help='Output directory')
    parser.add_argument('--batch', default=16, type=int, help='(extension) pairs prepared together in one batch')
    return parser


def read_raw_pair(input_dir, index):
    """(optical BGR uint8 (H, W, 3), thermal uint16 (h, w))"""
    from PIL import Image
    with Image.open(os.path.join(input_dir, index + SUFFIX)) as im:
        optical = np.ascontiguousarray(np.array(im.convert('RGB'), np.uint8)[:, :, ::-1])           # BGR, as cv_bridge's bgr8
    path = os.path.join(input_dir, index + '_thermal_raw.png')
    with Image.open(path) as im:
        thermal = np.array(im)
    if thermal.ndim != 2 or thermal.dtype != np.uint16:
        raise ValueError('%s: the raw thermal image must be 16-bit greyscale' % path)
    return optical, thermal


def write_pair(out_dir, index, optical, thermal_raw, thermal_rescaled_u16):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(optical[:, :, ::-1])).save(os.path.join(out_dir, index + '_optical.png'))
    Image.fromarray(thermal_raw).save(os.path.join(out_dir, index + '_thermal_raw.png'))
    Image.fromarray(thermal_rescaled_u16).save(os.path.join(out_dir, index + '_thermal.png'))


def index_key(i):
    return (0, int(i), i) if i.isdigit() else (1, 0, i)


def main(argv=None):
    args = build_parser().parse_args(argv)
    with open(args.yaml_config, 'rt') as fh:
        params = yaml.safe_load(fh)
    ignored = sorted(k for k in params if k in IGNORED_KEYS or k.startswith(IGNORED_PREFIXES))
    if ignored:
        print('Accepted and ignored (they need ROS or a display): ' + ', '.join(ignored))
    calibration = None
    if params['undistort_images']:
        with open(os.path.join(args.input_dir, params['image/calibration_params']), 'rt') as fh:
            calibration = yaml.safe_load(fh)
    import torch
    from multipoint_amd.utils import frames
    indices = sorted((f[:-len(SUFFIX)] for f in os.listdir(args.input_dir) if f.endswith(SUFFIX)), key=index_key)
    print('Number of pairs: ' + str(len(indices)))
    out_dir = os.path.join(args.output_dir, 'preprocessed')
    save = params.get('save_preprocessed_images', True)
    if save:
        os.makedirs(out_dir, exist_ok=True)
    step = max(args.batch, 1)
    for at in range(0, len(indices), step):
        batch = indices[at:at + step]
        pairs = [read_raw_pair(args.input_dir, i) for i in batch]
        optical, raw, _, saved = frames.prepare_frames(np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]),
                                                       params, calibration, return_saved=True)
        optical = optical.cpu().numpy()
        raw, saved = (t.view(torch.int16).cpu().numpy().view(np.uint16) for t in (raw, saved))
        for k, index in enumerate(batch):
            if save:
                write_pair(out_dir, index, optical[k], raw[k], saved[k])
            if params.get('verbose', False):
                print('%s: optical %dx%d, thermal %dx%d, counts %d .. %d' % (index, optical[k].shape[0], optical[k].shape[1],
                                                                            raw[k].shape[0], raw[k].shape[1], raw[k].min(), raw[k].max()))


if __name__ == '__main__':
    main()
