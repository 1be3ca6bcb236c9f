#!/usr/bin/env python3
"""Drop-in for the hot path of the reference's predict_align_image_pair.py: same flags
(-y -m -v -i -r -p -e -tk -th -s), same yaml keys, same model_weights/<name>/{params.yaml,<version>.model}
format, same three timing prints (reference predict_align_image_pair.py:141-143) -- computed on an
MI355X through libmultipoint_hip.so.  -e computes NN-mAP, M-score and homography correctness like the
reference (utils.compute_descriptor_metrics; per-sample arithmetic and a batched RANSAC on the GPU -- the
RANSAC is the product's own, not OpenCV's RNG).  The matplotlib/cv2 visualisation of -p is replaced by a
text summary of keypoints/matches, the estimated and the ground-truth homography (and --save-npz), and with
--plot-dir by PNG files drawn on the GPU (multipoint_amd.utils.drawing)."""
import argparse
import os
import random
import time

import numpy as np
import torch
import yaml

import multipoint_amd.datasets as datasets
import multipoint_amd.models as models
import multipoint_amd.utils as utils
from multipoint_amd.pipeline import PairPipeline


def synchronize():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def build_parser():
    parser = argparse.ArgumentParser(description='Predict the keypoints of an image')
    parser.add_argument('-y', '--yaml-config', default='configs/config_image_pair_dataset_prediction.yaml', help='YAML config file')
    parser.add_argument('-m', '--model-dir', default='model_weights/multipoint', help='Directory of the model')
    parser.add_argument('-v', '--version', default='latest', help='Model version (name of the param file), none for no weights')
    parser.add_argument('-i', '--index', default=0, type=int, help='Index of the sample to predict and show')
    parser.add_argument('-r', '--radius', default=4, type=int, help='Radius of the keypoint circle')
    parser.add_argument('-p', dest='plot', action='store_true', help='If set the prediction the results are displayed')
    parser.add_argument('-e', dest='evaluation', action='store_true', help='If set the evaluation metrics are computed')
    parser.add_argument('-tk', dest='threshold_keypoints', default=4, type=int, help='Distance below which two keypoints are considered a match')
    parser.add_argument('-th', dest='threshold_homography', default=1, type=int, help='Homography correctness threshold')
    parser.add_argument('-s', '--seed', default=0, type=int, help='Seed of the random generators')
    parser.add_argument('--save-npz', default=None, help='(extension) write keypoints/descriptors/matches of the sample here')
    parser.add_argument('--refine', action='store_true', help='(extension) re-match under the first homography estimate and '
                        'polish it (utils.refine_alignment); the aligned image uses the refined estimate')
    parser.add_argument('--subpixel', action='store_true', help='(extension) refine the keypoints to sub-pixel positions on the '
                        'detector map (utils.refine_keypoints): descriptors are sampled and the homography is estimated at them; '
                        'with -e the same as prediction.subpixel.enable')
    parser.add_argument('--mi', action='store_true', help='(extension) print the negative normalised mutual information at 100 bins of '
                        'the pair under the identity, the estimated and (with --refine) the refined homography')
    parser.add_argument('--mi-refine', action='store_true', help='(extension) maximise the mutual information from the estimated '
                        'homography (utils.alignment.align_images; yaml block prediction.mi_alignment) and print the result')
    parser.add_argument('--ecc-refine', action='store_true', help='(extension) polish the estimated homography by ECC maximisation '
                        'on gradient images (utils.ecc.refine_alignment_ecc_batch; yaml block prediction.ecc_alignment) and print '
                        'the result')
    parser.add_argument('--ecc-transform', default=None, choices=['translation', 'similarity', 'affine', 'homography'],
                        help="(extension) with --ecc-refine: the motion model; overrides prediction.ecc_alignment['model'] "
                        '(default homography)')
    parser.add_argument('--mi-transform', default=None, choices=['homography', 'similarity', 'affine'],
                        help='(extension) with --mi-refine: motion model the mutual-information optimiser searches in; overrides '
                        "prediction.mi_alignment['alignment/model'] (default homography)")
    parser.add_argument('--transform', default=None, choices=['homography', 'similarity', 'affine'],
                        help='(extension) motion model of the estimate (default: prediction.transform_model, else homography): a '
                        'similarity (rotation, scale, two translations) or an affine transform are determined by fewer inliers '
                        'than the 8-parameter homography')
    parser.add_argument('--plot-dir', default=None, help='(extension) with -p: write matches.png, matches_inliers.png, '
                        'warped_optical.png, overlay_checker.png and overlay_anaglyph.png into this directory')
    add_topk_mode_arguments(parser)
    return parser


def add_topk_mode_arguments(parser):
    """--topk-mode / --anms-robust, shared by the command lines that cut their keypoint lists to prediction.topk."""
    parser.add_argument('--topk-mode', default=None, choices=list(utils.TOPK_MODES),
                        help="(extension) which prediction.topk keypoints are kept: 'score' the highest scores (default), 'anms' "
                        'the largest suppression radii -- adaptive non-maximal suppression, spread over the frame; overrides '
                        'prediction.topk_mode')
    parser.add_argument('--anms-robust', default=None, type=float,
                        help="(extension) with topk_mode 'anms': a keypoint is dominated by scores above its own divided by this "
                        'value in (0, 1]; overrides prediction.anms_robust (default 1.0)')


def apply_topk_mode_arguments(args, pred):
    """Write --topk-mode / --anms-robust into the prediction block (where PairPipeline and the evaluation drivers read them) and
    return the keyword arguments utils.box_nms / detect_keypoints take for it: none in the score mode.  An unknown mode, and
    'anms' with `topk: 0`, are a ValueError before any work."""
    if args.topk_mode is not None:
        pred['topk_mode'] = args.topk_mode
    if args.anms_robust is not None:
        pred['anms_robust'] = args.anms_robust
    return utils.topk_selection(pred)


def write_plots(plot_dir, optical, thermal, kp_optical, kp_thermal, matches, inlier_mask, H_final, radius):
    """The pictures of reference predict_align_image_pair.py:197-254 as files: the match picture with all matches and with
    RANSAC's inliers alone (its matchesMask picture), one colour per match in match order; the optical image warped onto the
    thermal frame by the final estimate and two overlays of it with the thermal image.  Returns the file names."""
    from multipoint_amd.datasets.augmentation import warp_perspective_cv
    from multipoint_amd.utils import drawing
    os.makedirs(plot_dir, exist_ok=True)
    query = np.array([m.queryIdx for m in matches], np.int64)
    train = np.array([m.trainIdx for m in matches], np.int64)
    kp_a, kp_b = kp_optical[query].reshape(-1, 2), kp_thermal[train].reshape(-1, 2)       # one keypoint pair per match
    inliers = np.zeros(len(matches), bool)
    inliers[:len(inlier_mask)] = np.asarray(inlier_mask).reshape(-1)[:len(matches)] != 0
    pictures = {'matches.png': drawing.draw_matches(optical, thermal, kp_a, kp_b, np.arange(len(matches)), radius=radius),
                'matches_inliers.png': drawing.draw_matches(optical, thermal, kp_a, kp_b, np.arange(len(matches)), mask=inliers,
                                                            radius=radius),
                'warped_optical.png': drawing.gray_to_rgb(warp_perspective_cv(optical, H_final[None], border_reflect=False))}
    views = drawing.alignment_views(optical, thermal, estimate_to_transform(H_final), modes=('checker', 'anaglyph'))
    pictures['overlay_checker.png'], pictures['overlay_anaglyph.png'] = views['checker'], views['anaglyph']
    for name, picture in pictures.items():
        drawing.save_png(os.path.join(plot_dir, name), picture)
    return list(pictures)


def load_network(config, model_dir, version, device, seed=0):
    net = getattr(models, config['model']['type'])(config['model'])
    if version != 'none':
        weights = torch.load(os.path.join(model_dir, version + '.model'), map_location=torch.device('cpu'))
        weights = utils.fix_model_weigth_keys(weights)
        net.load_state_dict(weights)
        del weights
    else:
        net.init_random_weights(seed)
    net.to(device)
    net.eval()
    return net


def select_device(config):
    if not config['prediction']['allow_gpu'] or not torch.cuda.is_available():
        raise RuntimeError('this implementation runs on an MI355X only: prediction.allow_gpu must be true and '
                           'a GPU must be visible (there is no CPU fallback; the reference runs on CPU)')
    return torch.device('cuda:0')


def refine_estimate(kp_optical, kp_thermal, desc_optical, desc_thermal, matches, mask, H, W, pred, H_est, sub_optical=None,
                    sub_thermal=None, model='homography'):
    """--refine: the sample's lists as a one-pair PairResults through utils.refine_alignment.  Prints inliers / matches
    before and after and returns the refined estimate (the first one where there is nothing to refine).  sub_*: the
    sub-pixel positions of --subpixel, which the estimates and the polish then read.  model: the motion model of --transform."""
    from multipoint_amd.pipeline import PairResults
    no, nt = kp_optical.shape[0], kp_thermal.shape[0]
    D = desc_optical.shape[1] if no else desc_thermal.shape[1] if nt else 0
    crosscheck = (pred['matching']['method'] == 'nnmatcher' or
                  (pred['matching']['method'] == 'bfmatcher' and not pred['matching']['knn_matches']
                   and pred['matching']['method_kwargs'].get('crossCheck', False)))
    if not crosscheck:
        raise ValueError('--refine starts from mutual matches: prediction.matching must be nnmatcher, or bfmatcher with crossCheck')
    before = 'Refinement: {} inliers of {} matches'.format(int(np.sum(mask)), len(matches))
    if no == 0 or nt == 0 or D not in (64, 128, 256, 384) or max(no, nt) > utils.MAX_RANSAC_MATCHES:
        print(before + ' -> unchanged (nothing to refine at these list sizes)')
        return H_est
    K = max(no, nt)
    dev = desc_optical.device
    kp = torch.zeros((2, K, 2), dtype=torch.int32, device=dev)
    kp[0, :no] = kp_optical.to(torch.int32); kp[1, :nt] = kp_thermal.to(torch.int32)
    desc = torch.zeros((2, K, D), dtype=torch.float32, device=dev)
    desc[0, :no] = desc_optical; desc[1, :nt] = desc_thermal
    midx = torch.full((1, K), -1, dtype=torch.int32)
    mdist = torch.zeros((1, K), dtype=torch.float32)
    for m in matches:
        midx[0, m.queryIdx] = m.trainIdx; mdist[0, m.queryIdx] = m.distance
    kp_sub = None
    if sub_optical is not None and sub_thermal is not None:
        kp_sub = torch.zeros((2, K, 2), dtype=torch.float32, device=dev)
        kp_sub[0, :no] = sub_optical; kp_sub[1, :nt] = sub_thermal
    res = PairResults(kp, None, torch.tensor([no, nt], dtype=torch.int32, device=dev), desc, midx.to(dev), mdist.to(dev),
                      torch.tensor([len(matches)], dtype=torch.int32, device=dev), H, W, kp_sub=kp_sub)
    res2, H_ref, _, n_in = utils.refine_alignment(res, pred['reprojection_threshold'],
                                                  threshold=pred['matching']['method_kwargs'].get('threshold', -1.0)
                                                  if pred['matching']['method'] == 'nnmatcher' else -1.0, model=model)
    if int(n_in[0]) < utils.transform_min_inliers(model):
        print(before + ' -> no refined estimate')
        return H_est
    print(before + ' -> {} inliers of {} matches'.format(int(n_in[0]), int(res2.match_count[0])))
    H_ref = H_ref[0].cpu().numpy()
    print('Refined Homography:' if model == 'homography' else 'Refined %s transform:' % model)
    print(H_ref)
    return H_ref


MI_ALIGNMENT_DEFAULTS = {'alignment/bin_sizes': [16, 32, 64, 100, 256], 'alignment/normalized_mi': True,
                         'alignment/smoothing_sigma': 0, 'alignment/check/both/max_diff_mi': 0.5, 'alignment/accept_init': True,
                         'alignment/ranking_method': 'order', 'use_image_pyramid': False, 'use_smoothing_stage': False,
                         'alignment/n_pyramid_levels': 2, 'alignment/filter_size': 5}
# (the values of the reference's config_align_images.yaml, except alignment/check/invalid_pixels, which is left off on purpose:
# an estimated homography usually brings border pixels into the frame, and that check would reject every refinement of it)


def estimate_to_transform(H_est):
    """The homography estimated here maps optical pixels to thermal ones (cv2.warpPerspective(optical, H_est) inverts it);
    the `transform` of utils.alignment maps thermal (destination) pixels to optical (source) ones, as the reference's align.py
    does: its inverse.  A singular estimate becomes the identity."""
    H_est = np.asarray(H_est, np.float64)
    if abs(np.linalg.det(H_est)) < 1e-12:
        return np.eye(3)
    return np.linalg.inv(H_est)


def mi_report(optical, thermal, named):
    """--mi: the negative normalised mutual information at 100 bins under each (name, optical -> thermal homography)."""
    from multipoint_amd.utils import alignment
    T = np.stack([estimate_to_transform(H) for _, H in named])
    v = alignment.negative_mutual_information_batch(optical, thermal, T[None], 100, normalized_mi=True)[0].cpu().numpy()
    print('Negative normalised MI (100 bins): ' + ', '.join('{} {:.6f}'.format(n, x) for (n, _), x in zip(named, v)))


def mi_refine(optical, thermal, H_est, pred, model=None):
    """--mi-refine: utils.alignment.align_images from the estimate -- with use_image_pyramid or use_smoothing_stage in the
    yaml block the staged align_images_mutual_information, which prints one line per stage.  Prints the winning candidate's
    type, its negative normalised mutual information at 100 bins and its matrix in the direction of the estimate (optical ->
    thermal).  model: --mi-transform, the optimiser's motion model in the place of the block's alignment/model."""
    from multipoint_amd.utils import alignment
    params = dict(MI_ALIGNMENT_DEFAULTS, **(pred.get('mi_alignment') or {}))
    if model is not None:
        params['alignment/model'] = model
    if params['use_image_pyramid'] or params['use_smoothing_stage']:
        _, T, kind, _, stages = alignment.align_images_mutual_information(optical[0, 0], thermal[0, 0],
                                                                          estimate_to_transform(H_est), params)
        for s in stages:
            print('MI stage {} {}x{}: {}'.format(s['name'], s['shape'][0], s['shape'][1], s['type'] or 'failed'))
    else:
        T, kind, _ = alignment.align_images(optical[0, 0], thermal[0, 0], estimate_to_transform(H_est), params)
    if T is None:
        print('MI alignment: none (no valid candidate)')
        return None
    v = alignment.calculate_negative_mutual_information(T, optical[0, 0], thermal[0, 0], T, 100, normalized_mi=True)
    print('MI alignment: {} negative normalised MI (100 bins) {:.6f}'.format(kind, v))
    H_mi = estimate_to_transform(T)
    print('MI-aligned Homography:')
    print(H_mi)
    return H_mi


ECC_ALIGNMENT_DEFAULTS = {'model': 'homography', 'feature': 'gradient', 'filter_size': 5, 'eps': 1e-6, 'max_iterations': 50,
                          'min_valid': 0.25}
ECC_STATUS = ('ok', 'too few valid pixels', 'G^T G not positive definite', "lambda's denominator <= 0", 'a non-finite value')


def ecc_refine(optical, thermal, H_est, pred, model=None):
    """--ecc-refine: utils.ecc.refine_alignment_ecc_batch from the estimate.  Prints the outcome, the correlation coefficient, the
    iterations and the matrix in the direction of the estimate (optical -> thermal); a failed refinement returns None.  model:
    --ecc-transform in the place of the block's model."""
    from multipoint_amd.utils import ecc
    params = dict(ECC_ALIGNMENT_DEFAULTS, **(pred.get('ecc_alignment') or {}))
    if model is not None:
        params['model'] = model
    r = ecc.refine_alignment_ecc_batch(optical[0, 0], thermal[0, 0], [0], estimate_to_transform(H_est)[None], params['model'],
                                       params['feature'], params['filter_size'], params['eps'], params['max_iterations'],
                                       params['min_valid'])
    if not r['success'][0]:
        print('ECC alignment: none ({} after {} iterations)'.format(ECC_STATUS[int(r['status'][0])], int(r['nit'][0])))
        return None
    print('ECC alignment: {} {} rho {:.6f} after {} iterations ({})'.format(
        params['feature'], params['model'], float(r['rho'][0]), int(r['nit'][0]),
        'converged' if r['converged'][0] else 'iteration limit'))
    H_ecc = estimate_to_transform(r['transform'][0])
    print('ECC-aligned Homography:')
    print(H_ecc)
    return H_ecc


def main(argv=None):
    args = build_parser().parse_args(argv)
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)

    with open(args.yaml_config, 'r') as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    with open(os.path.join(args.model_dir, 'params.yaml'), 'r') as f:
        config['model'] = yaml.load(f, Loader=yaml.FullLoader)['model']      # overwrite the model params
    select = apply_topk_mode_arguments(args, config['prediction'])          # (refuses a bad mode before any work)

    device = select_device(config)
    print('Predicting on device: {}'.format(device))

    dataset = getattr(datasets, config['dataset']['type'])(config['dataset'])
    loader_dataset = torch.utils.data.DataLoader(dataset, batch_size=config['prediction']['batchsize'],
                                                 shuffle=False, num_workers=datasets.loader_num_workers(dataset, config['prediction']['num_worker']))
    net = load_network(config, args.model_dir, args.version, device, args.seed)
    pred = config['prediction']
    if args.subpixel:
        pred['subpixel'] = dict(pred.get('subpixel') or {}, enable=True)
    if args.transform is not None:
        pred['transform_model'] = args.transform
    model = pred.get('transform_model', 'homography')
    utils.transform_model(model)                        # (refuses an unknown name before any work)
    subpixel = bool((pred.get('subpixel') or {}).get('enable', False))
    if subpixel and hasattr(net, 'describe'):
        raise ValueError('subpixel: ClassicDetectors models have no sub-pixel keypoints (LGHD descriptors are patch histograms '
                         'at integer centres)')

    with torch.no_grad():
        if args.evaluation:
            # reference predict_align_image_pair.py:69-88: utils.compute_descriptor_metrics over the whole loader; the
            # per-sample arithmetic (mp_pair_metrics) and the RANSAC homography estimate (mp_find_homography) run on the GPU
            synchronize(); t0 = time.time()
            results = utils.compute_descriptor_metrics(net, loader_dataset, device, pred, args.threshold_keypoints,
                                                       args.threshold_homography)
            synchronize(); dt = time.time() - t0
            print('NN-mAP: {}'.format(results['nn_map']))
            print('M-Score: {}'.format(results['m_score']))
            print('Homography Correctness: {}'.format(results['h_correctness']))
            print('Matches: {}  ({:.1f} pairs/s)'.format(len(results['tp_optical']), len(dataset) / dt))
            results['config'] = config
            results['threshold_keypoints'] = args.threshold_keypoints
            results['threshold_homography'] = args.threshold_homography
            target_dir = os.path.join(args.model_dir, 'descriptor_evaluation')
            os.makedirs(target_dir, exist_ok=True)
            np.save(os.path.join(target_dir, os.path.split(args.model_dir.strip('/'))[-1] + '_' +
                                 time.strftime('%Y-%m-%d_%H-%M-%S', time.gmtime())), results)

        # get the sample and move it to the right device
        synchronize()
        t_start = time.time()
        data = dataset[args.index]
        data = utils.data_to_device(data, device)
        data = utils.data_unsqueeze(data, 0)

        synchronize()
        t_1 = time.time()
        out_optical = net(data['optical'])
        out_thermal = net(data['thermal'])
        synchronize()
        t_2 = time.time()

        # the forward's maps: what the sub-pixel fit reads (the NMS output has zeros around every keypoint); an image the tie
        # guard redoes is redone in place, so these are the maps the keypoints come from
        prob_optical, prob_thermal = out_optical['prob'], out_thermal['prob']
        if pred['nms'] > 0:
            # (box_nms with the top-k tie guard: an image whose top-k cut falls inside a plateau of tied scores is re-evaluated
            # with the tie-exact convolution algorithm, so the kept indices follow the reference's exact score order)
            out_optical['prob'] = utils.box_nms_tie_robust(net, data['optical'], out_optical, pred['nms'], pred['detection_threshold'],
                                                           keep_top_k=pred['topk'], on_cpu=pred['cpu_nms'],
                                                           valid_mask=data['optical']['valid_mask'], **select)
            out_thermal['prob'] = utils.box_nms_tie_robust(net, data['thermal'], out_thermal, pred['nms'], pred['detection_threshold'],
                                                           keep_top_k=pred['topk'], on_cpu=pred['cpu_nms'],
                                                           valid_mask=data['thermal']['valid_mask'], **select)
        else:
            out_optical['prob'] = out_optical['prob'] * data['optical']['valid_mask']
            out_thermal['prob'] = out_thermal['prob'] * data['thermal']['valid_mask']
        synchronize()
        t_3 = time.time()
        print('Loading the data took: {} s'.format(t_1 - t_start))
        print('Two forward passes took: {} s'.format(t_2 - t_1))
        print('Box nms: {} s'.format(t_3 - t_2))

        if args.plot or args.save_npz or args.refine or args.mi or args.mi_refine or args.ecc_refine:
            H, W = data['optical']['image'].shape[2:]
            thr = pred['detection_threshold']
            pred_optical = torch.nonzero((out_optical['prob'][0].squeeze() > thr).float())
            pred_thermal = torch.nonzero((out_thermal['prob'][0].squeeze() > thr).float())
            sub_optical = sub_thermal = None
            if subpixel:
                def refine(prob, kp):
                    cnt = torch.tensor([kp.shape[0]], dtype=torch.int32, device=kp.device)
                    return utils.refine_keypoints(prob[:1], kp.to(torch.int32).reshape(1, -1, 2), cnt)[0]
                sub_optical, sub_thermal = refine(prob_optical, pred_optical), refine(prob_thermal, pred_thermal)
            desc_optical = utils.interpolate_descriptors(pred_optical if sub_optical is None else sub_optical,
                                                         out_optical['desc'][0], H, W)
            desc_thermal = utils.interpolate_descriptors(pred_thermal if sub_thermal is None else sub_thermal,
                                                         out_thermal['desc'][0], H, W)
            matches = utils.get_matches(desc_optical.cpu().numpy(), desc_thermal.cpu().numpy(),
                                        pred['matching']['method'], pred['matching']['knn_matches'],
                                        **pred['matching']['method_kwargs'])
            print('--------------------------------------------------------')
            print('Optical keypoints: {}'.format(pred_optical.shape[0]))
            print('Thermal keypoints: {}'.format(pred_thermal.shape[0]))
            print('Matches ({}): {}'.format(pred['matching']['method'], len(matches)))
            if matches:
                d = np.array([m.distance for m in matches])
                print('Match distance: min {:.4f} mean {:.4f} max {:.4f}'.format(d.min(), d.mean(), d.max()))
            print('--------------------------------------------------------')
            # align the images: homography from the matches (reference :209-216) next to the ground truth (:252-257)
            kpo = pred_optical.cpu().numpy(); kpt = pred_thermal.cpu().numpy()
            # (with --subpixel the estimate reads the refined positions: float points, as cv2.findHomography takes them)
            kpo_est = kpo if sub_optical is None else sub_optical.cpu().numpy()
            kpt_est = kpt if sub_thermal is None else sub_thermal.cpu().numpy()
            optical_pts = np.array([kpo_est[m.queryIdx][::-1] for m in matches]).reshape(-1, 2)
            thermal_pts = np.array([kpt_est[m.trainIdx][::-1] for m in matches]).reshape(-1, 2)
            H_est, mask = utils.find_transform_points(optical_pts, thermal_pts, model, pred['reprojection_threshold'], device=device)
            if H_est is None:
                H_est = np.eye(3, 3)
            eye = torch.eye(3)
            H_gt = np.matmul(data['thermal'].get('homography', eye[None])[0].cpu().numpy(),
                             np.linalg.inv(data['optical'].get('homography', eye[None])[0].cpu().numpy()))
            print('Estimated Homography:' if model == 'homography' else 'Estimated %s transform:' % model)
            print(H_est)
            if model == 'similarity':
                print('Similarity: angle {:.6f} rad  scale {:.6f}  dx {:.3f}  dy {:.3f}'.format(*utils.decompose_similarity(H_est)))
            print('RANSAC inliers: {} of {} matches'.format(int(np.sum(mask)), len(matches)))
            H_first = H_est
            if args.refine:
                H_est = refine_estimate(pred_optical, pred_thermal, desc_optical, desc_thermal, matches, mask, H, W, pred,
                                        H_est, sub_optical, sub_thermal, model)
            if args.mi:
                mi_report(data['optical']['image'][:1], data['thermal']['image'][:1],
                          [('identity', np.eye(3)), ('estimated', H_first)] + ([('refined', H_est)] if args.refine else []))
            H_mi = None
            if args.mi_refine:
                H_mi = mi_refine(data['optical']['image'][:1], data['thermal']['image'][:1], H_est, pred, args.mi_transform)
            if args.ecc_refine:
                H_ecc = ecc_refine(data['optical']['image'][:1], data['thermal']['image'][:1], H_est if H_mi is None else H_mi,
                                   pred, args.ecc_transform)
                H_mi = H_mi if H_ecc is None else H_ecc
            print('Ground Truth Homography:')
            print(H_gt)
            print('--------------------------------------------------------')
            # the aligned image: optical warped onto the thermal frame by the estimate (reference :218,
            # cv2.warpPerspective(im_optical, H_est, size, borderMode=cv2.BORDER_CONSTANT)), on the GPU
            from multipoint_amd.datasets.augmentation import warp_perspective_cv
            warped_image = warp_perspective_cv(data['optical']['image'][:1], H_est[None], border_reflect=False)
            inside = warp_perspective_cv(torch.ones_like(data['optical']['image'][:1]), H_est[None]) > 0.999
            if bool(inside.any()):
                resid = (warped_image - data['thermal']['image'][:1]).abs()[inside].mean().item()
                print('Aligned optical vs thermal: mean |diff| {:.4f} over {:.1f} % of the frame'.format(
                    resid, 100.0 * inside.float().mean().item()))
            if args.save_npz:
                np.savez_compressed(args.save_npz, kp_optical=pred_optical.cpu().numpy(), kp_thermal=pred_thermal.cpu().numpy(),
                                    desc_optical=desc_optical.cpu().numpy(), desc_thermal=desc_thermal.cpu().numpy(),
                                    match_query=np.array([m.queryIdx for m in matches]),
                                    match_train=np.array([m.trainIdx for m in matches]),
                                    match_distance=np.array([m.distance for m in matches], dtype=np.float32),
                                    homography_estimated=H_est, homography_ground_truth=H_gt,
                                    warped_optical=warped_image[0, 0].cpu().numpy(),
                                    **({'kp_optical_sub': kpo_est.astype(np.float32), 'kp_thermal_sub': kpt_est.astype(np.float32)}
                                       if subpixel else {}))
            if args.plot and args.plot_dir:
                # under the final estimate: the refined one with --refine, the MI- or ECC-aligned one with --mi-refine / --ecc-refine
                names = write_plots(args.plot_dir, data['optical']['image'][:1], data['thermal']['image'][:1], kpo, kpt, matches,
                                    mask, H_est if H_mi is None else H_mi, args.radius)
                print('Wrote {} to {}'.format(', '.join(names), args.plot_dir))


if __name__ == "__main__":
    main()
