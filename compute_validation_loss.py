#!/usr/bin/env python3
"""Validation loss of one or more checkpoints: the validation loop of the reference's train.py (:44-50, :127-150) without
the training, to choose a checkpoint.  Forward (mp_forward, or mp_forward_batch_stats with --batch-statistics) and SuperPointLoss (multipoint_amd.utils.losses) run on the
GPU; the per-batch losses are accumulated on the device and read once per checkpoint."""
import argparse
import copy
import glob
import json
import os
import random
import sys

import numpy as np
import torch
import yaml

import multipoint_amd.datasets as datasets
import multipoint_amd.utils as utils
import multipoint_amd.utils.losses as losses
from predict_align_image_pair import load_network

DESCRIPTION = """Validation loss of the checkpoints of a training run (train.py's compute_validation_loss loop).

train.py validates with the network still in training mode, so its BatchNorm layers use the statistics of each
validation batch.  By default this tool runs the forward in eval mode (running statistics): the loss reported is the
loss of the eval-mode forward -- the outputs a deployment actually sees -- and differs from the validation loss train.py
logs for networks with BatchNorm.  With --batch-statistics the forward normalises with the statistics of each batch, as
train.py's does, and reports train.py's validation loss (fp32 models only; the running statistics are not updated).
A remaining difference: train.py under multi-GPU DataParallel computes the statistics per replica's chunk of the batch,
this tool over the whole batch."""


def build_parser():
    parser = argparse.ArgumentParser(description=DESCRIPTION, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('-y', '--yaml-config', default='configs/config_validation_loss.yaml',
                        help='YAML config with the training config keys dataset, model, loss, training.batchsize and '
                             'training.validation.{filename,keypoints}')
    parser.add_argument('-m', '--model-dir', default='model_weights/multipoint', help='Directory of the checkpoints')
    parser.add_argument('-v', '--versions', nargs='+', default=None,
                        help='Checkpoint versions (file names without .model); default: every *.model file, ordered by '
                             'epoch (e{N}), latest last')
    parser.add_argument('-s', '--seed', default=0, type=int,
                        help='Seed of the random generators, reset before every checkpoint so that each sees the same '
                             'augmentation and label noise')
    photometric = parser.add_mutually_exclusive_group()
    photometric.add_argument('--no-photometric', action='store_true',
                             help='Validate without the photometric augmentation the config asks for')
    photometric.add_argument('--photometric', choices=('host', 'device'), default=None,
                             help="Validate with the config's photometric augmentation (on the GPU), its per-pixel noise "
                                  "drawn as train.py draws it ('host': np.random fields, the reference's stream) or on "
                                  "the GPU from one np.random key per field ('device'); sets "
                                  'dataset.augmentation.photometric.noise')
    parser.add_argument('--batch-statistics', action='store_true',
                        help="Run the forward as train.py's validation loop does: BatchNorm with the statistics of each "
                             'batch (training mode, forward only) instead of the running statistics')
    parser.add_argument('--save-json', default=None, help='Write the averages of every checkpoint to this JSON file')
    return parser


def list_versions(model_dir):
    """Every *.model of the directory: e{N} by N, other names alphabetically, latest last."""
    names = [os.path.basename(p)[:-len('.model')] for p in glob.glob(os.path.join(model_dir, '*.model'))]

    def key(n):
        if n == 'latest':
            return (2, 0, n)
        if n[:1] == 'e' and n[1:].isdigit():
            return (0, int(n[1:]), n)
        return (1, 0, n)
    return sorted(names, key=key)


def validation_config(config):
    """train.py:44-50: the dataset config with the validation file and labels.  An on-the-fly SyntheticShapes block reads no
    file (its samples and labels are generated): it passes through as it is."""
    if config['dataset'].get('type') == 'SyntheticShapes' and config['dataset'].get('on-the-fly', True):
        return copy.deepcopy(config['dataset'])
    validation = config.get('training', {}).get('validation', {})
    if validation.get('filename') is None:
        raise SystemExit('error: the config names no validation set: set training.validation.filename (and '
                         'training.validation.keypoints for the detector loss)')
    val = copy.deepcopy(config['dataset'])
    val['filename'] = validation['filename']
    val['keypoints_filename'] = validation.get('keypoints')
    return val


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def evaluate_checkpoint(net, loader, loss_fn, device, returns_pair):
    """train.py:127-150: (average loss, {component: average}) over the loader, Σ batch value / len(loader)."""
    total, keys = None, None
    with torch.no_grad():
        for data in loader:
            data = utils.data_to_device(data, device)
            sample = data['optical'] if returns_pair else data
            if loss_fn.config['detector_loss'] and 'keypoints' not in sample:
                raise SystemExit('error: the validation samples carry no keypoints, but the detector loss is on: set '
                                 'training.validation.keypoints to a label file (export_keypoints.py) or disable '
                                 'loss.detector_loss')
            if returns_pair:
                values, keys = loss_fn.evaluate(net(data['optical']), data['optical'], net(data['thermal']), data['thermal'])
            else:
                values, keys = loss_fn.evaluate(net(data), data)
            total = values if total is None else total + values
    if total is None:
        raise SystemExit('error: the validation set is empty')
    avg = (total / len(loader)).cpu().tolist()
    return avg[0], {k: avg[i + 1] for i, k in enumerate(keys)}


def main(argv=None):
    args = build_parser().parse_args(argv)
    with open(args.yaml_config, 'r') as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    if 'model' not in config:
        with open(os.path.join(args.model_dir, 'params.yaml'), 'r') as f:
            config['model'] = yaml.load(f, Loader=yaml.FullLoader)['model']
    photometric = config['dataset'].get('augmentation', {}).get('photometric', {})
    if photometric.get('enable', False):
        if args.no_photometric:
            photometric['enable'] = False
        elif args.photometric is not None:
            photometric['noise'] = args.photometric
        elif photometric.get('noise') is None:
            raise SystemExit('error: the config enables photometric augmentation (dataset.augmentation.photometric) but '
                             "does not say where its per-pixel noise is drawn; rerun with --photometric host (train.py's "
                             'np.random stream) or --photometric device (drawn on the GPU), or with --no-photometric to '
                             'validate without it')
    if not torch.cuda.is_available():
        raise SystemExit('error: compute_validation_loss runs on an MI355X only (no CPU fallback)')
    device = torch.device('cuda:0')

    versions = args.versions or list_versions(args.model_dir)
    if not versions:
        raise SystemExit('error: no *.model checkpoint in %s' % args.model_dir)
    dataset_class = getattr(datasets, config['dataset']['type'])
    loss_fn = getattr(losses, config['loss']['type'])(config['loss'])
    batchsize = config['training']['batchsize']
    num_worker = config['training'].get('num_worker', 0)

    results = {}
    for version in versions:
        seed_all(args.seed)
        dataset = dataset_class(validation_config(config))
        loader = torch.utils.data.DataLoader(dataset, batch_size=batchsize, shuffle=False,
                                             num_workers=datasets.loader_num_workers(dataset, num_worker))
        net = load_network(config, args.model_dir, version, device, args.seed)
        if hasattr(net, 'set_force_return_logits'):
            net.set_force_return_logits(True)
        if args.batch_statistics:
            net.set_batch_statistics(True)
        loss, comp = evaluate_checkpoint(net, loader, loss_fn, device, dataset.returns_pair())
        results[version] = dict(loss=loss, **comp)
        print('%s: loss %.6g  %s' % (version, loss, '  '.join('%s %.6g' % (k, v) for k, v in comp.items())), flush=True)
        del net
    best = min(results, key=lambda v: results[v]['loss'])
    print('best: %s' % best)
    if args.save_json:
        with open(args.save_json, 'w') as f:
            json.dump({'versions': results, 'best': best, 'seed': args.seed,
                       'eval_mode': not args.batch_statistics}, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
