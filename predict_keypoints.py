#!/usr/bin/env python3
"""Drop-in for the hot path of the reference's predict_keypoints.py (flags -y -m -v -i -r -p -e -b -t
-mask -s): forward + box_nms (without the valid-mask multiply, reference predict_keypoints.py:136-156)
for a single sample or a batch (-b).  -e computes the keypoint repeatability of an image-pair dataset like the
reference (utils.compute_repeatability_multispectral) and, for a single-image dataset with 'keypoints' labels, the
detector precision / recall / mAP (utils.compute_detector_metrics) -- per-sample arithmetic on the GPU in both
cases.  The windows of -p are replaced by a text summary and, with --plot-dir, by PNG files drawn on the GPU
(multipoint_amd.utils.drawing)."""
import argparse
import os
import time

import numpy as np
import torch
import yaml

import multipoint_amd.datasets as datasets
import multipoint_amd.utils as utils
from predict_align_image_pair import add_topk_mode_arguments, apply_topk_mode_arguments, load_network, select_device


def build_parser():
    parser = argparse.ArgumentParser(description='Predict the keypoints of an image')
    parser.add_argument('-y', '--yaml-config', default='configs/config_image_pair_dataset_prediction.yaml', help='YAML config file')
    parser.add_argument('-m', '--model-dir', default='model_weights/multipoint', help='Directory of the model')
    parser.add_argument('-v', '--version', default='latest', help='Model version (name of the param file)')
    parser.add_argument('-i', '--index', default=0, type=int, help='Index of the sample to predict and show')
    parser.add_argument('-r', '--radius', default=4, type=int, help='Radius of the keypoint circle')
    parser.add_argument('-p', dest='plot', action='store_true', help='If set the prediction the results are displayed')
    parser.add_argument('-e', dest='evaluation', action='store_true', help='If set the evaluation metrics are computed')
    parser.add_argument('-b', dest='batch', action='store_true', help='If set a batch of images is predicted and displayed instead of a single image')
    parser.add_argument('-t', dest='threshold', default=3, type=int, help='Distance threshold for two keypoints to be considered a match')
    parser.add_argument('-mask', dest='mask', action='store_true', help='If set invalid image pixels will be set to 0')
    parser.add_argument('-s', '--seed', default=0, type=int, help='Seed of the random generators')
    parser.add_argument('--plot-dir', default=None, help='(extension) with -p: write the pictures the reference shows in windows '
                        'into this directory as <i>_image[_optical|_thermal].png, <i>_prob*.png and <i>_prob_masked*.png')
    add_topk_mode_arguments(parser)
    return parser


def write_plots(plot_dir, data, outs, detection_threshold, radius, use_mask):
    """The pictures of reference predict_keypoints.py:159-280, one set per sample i of the batch and per spectrum: the image
    (times the valid mask with -mask) with the predictions -- (prob > threshold) * valid_mask -- as green rings of `radius` and
    the label keypoints, where the dataset has them, as red rings of radius + 2; prob and prob * valid_mask at the reference's
    display gain 0.9 / threshold.  Returns the file names."""
    from multipoint_amd.utils import drawing
    os.makedirs(plot_dir, exist_ok=True)
    gain = 0.9 / detection_threshold
    written = []
    for side, out in outs.items():
        d = data if side == 'image' else data[side]
        suffix = '' if side == 'image' else '_' + side
        B, _, H, W = d['image'].shape
        mask = d['valid_mask'].reshape(B, H, W).to(torch.float32)
        prob = out['prob'].reshape(B, H, W).to(torch.float32)
        views = {'image': drawing.gray_to_rgb(d['image'], mask if use_mask else None),
                 'prob': drawing.gray_to_rgb(prob, gain=gain), 'prob_masked': drawing.gray_to_rgb(prob, mask, gain=gain)}
        labels = d.get('keypoints')
        for i in range(B):
            predicted = torch.nonzero((prob[i] > detection_threshold).float() * mask[i])
            drawing.draw_keypoints(views['image'][i], predicted, radius=radius, color=(0, 255, 0))
            if labels is not None:
                kp = labels[i].squeeze()
                if kp.shape == (H, W):
                    kp = torch.nonzero(kp)
                drawing.draw_keypoints(views['image'][i], kp, radius=radius + 2, color=(255, 0, 0))
            for name, view in views.items():
                written.append('%d_%s%s.png' % (i, name, suffix))
                drawing.save_png(os.path.join(plot_dir, written[-1]), view[i])
    return written


def main(argv=None):
    args = build_parser().parse_args(argv)
    with open(args.yaml_config, 'r') as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    with open(os.path.join(args.model_dir, 'params.yaml'), 'r') as f:
        config['model'] = yaml.load(f, Loader=yaml.FullLoader)['model']
    select = apply_topk_mode_arguments(args, config['prediction'])          # (refuses a bad mode before any work)
    device = select_device(config)
    print('Predicting on device: {}'.format(device))
    dataset = getattr(datasets, config['dataset']['type'])(config['dataset'])
    loader_dataset = torch.utils.data.DataLoader(dataset, batch_size=config['prediction']['batchsize'],
                                                 shuffle=False, num_workers=datasets.loader_num_workers(dataset, config['prediction']['num_worker']))
    net = load_network(config, args.model_dir, args.version, device, args.seed)
    pred = config['prediction']

    with torch.no_grad():
        if args.evaluation:
            # reference predict_keypoints.py:60-107
            import random
            random.seed(args.seed); np.random.seed(args.seed); torch.manual_seed(args.seed)
            if dataset.returns_pair():
                repeatability_mean, repeatability, n_kp_optical, n_kp_thermal = utils.compute_repeatability_multispectral(
                    net, loader_dataset, device, config, distance_thresh=args.threshold)
                print('Repeatability: {}'.format(repeatability_mean))
                print('Number of optical keypoints: {}'.format(np.mean(n_kp_optical)))
                print('Number of thermal keypoints: {}'.format(np.mean(n_kp_thermal)))
                results = {'repeatability_mean': repeatability_mean, 'repeatability': repeatability,
                           'n_kp_optical': n_kp_optical, 'n_kp_thermal': n_kp_thermal,
                           'distance_threshold': args.threshold, 'config': config}
            else:
                precision, recall, prob, dist = utils.compute_detector_metrics(net, loader_dataset, device, pred)
                results = {'precision': precision, 'recall': recall, 'prob': prob, 'dist': dist, 'config': config}
                print('Average distance error for true positives: {}'.format(dist.mean()))
                print('mAP: {}'.format(utils.compute_mAP(precision, recall)))
            target_dir = os.path.join(args.model_dir, 'detector_evaluation')
            os.makedirs(target_dir, exist_ok=True)
            np.save(os.path.join(target_dir, os.path.split(args.model_dir.strip('/'))[-1] + '_' +
                                 time.strftime('%Y-%m-%d_%H-%M-%S', time.gmtime())), results)
        t_start = time.time()
        if args.batch:
            for i in range(args.index + 1):
                data = next(iter(loader_dataset))
        else:
            data = dataset[args.index]
        data = utils.data_to_device(data, device)
        if not args.batch:
            data = utils.data_unsqueeze(data, 0)

        def nms(out, data):
            if pred['nms'] > 0:      # (with the top-k tie guard: utils.box_nms_tie_robust)
                return utils.box_nms_tie_robust(net, data, out, pred['nms'], pred['detection_threshold'], keep_top_k=pred['topk'],
                                                on_cpu=pred['cpu_nms'], **select)
            return out['prob']

        outs = {}
        if dataset.returns_pair():
            for side in ('optical', 'thermal'):
                out = net(data[side])
                out['prob'] = nms(out, data[side])
                outs[side] = out
        else:
            out = net(data)
            out['prob'] = nms(out, data)
            outs['image'] = out
        torch.cuda.synchronize()
        print('Prediction took: {} s'.format(time.time() - t_start))
        for side, out in outs.items():
            n = (out['prob'] > pred['detection_threshold']).flatten(1).sum(1).cpu().numpy()
            print('{} keypoints per image: {}'.format(side, n.tolist()))
        if args.plot and args.plot_dir:
            names = write_plots(args.plot_dir, data, outs, pred['detection_threshold'], args.radius, args.mask)
            print('Wrote {} pictures to {}'.format(len(names), args.plot_dir))


if __name__ == "__main__":
    main()
