#!/usr/bin/env python3
"""Estimate the initial transform align_images.py starts from, instead of measuring it by hand: ONE optical -> thermal
homography for a whole recording, from the pooled matches of many of its pairs (multipoint_amd.utils.estimate_shared_homography
on an MI355X).  A rig has one transform for all its frames; a single cross-spectral pair gives few matches and many wrong
ones, a few hundred pairs together give thousands.

    prepare_images.py  ->  estimate_initial_transform.py  ->  align_images.py  ->  check_alignment.py

The flags -y -m -v -s and the `prediction:` keys of the yaml (nms, detection_threshold, topk, matching,
reprojection_threshold, allow_gpu) are predict_align_image_pair.py's; -i is the directory of `<index>_optical.png` /
`<index>_thermal.png` pairs (prepare_images.py's `preprocessed/`: the optical frames of one size, the thermal frames of
another).  It works with a MultiPoint checkpoint and with the weight-free LGHD baseline (-m tests/golden/lghd -v none).

Written next to the pairs (or to -o and its directory):
  initial_transform.yaml          perspective: 3x3, thermal pixel -> optical pixel with h22 = 1 -- the inverse, taken in float64,
                                  of the estimated optical -> thermal homography; the key and direction align_images.py reads
  initial_transform_report.json   pairs read / used, matches pooled, inliers, cost before / after the polish, the inliers of every
                                  pair and the number of pairs with at least 4 of them

An existing yaml is not overwritten without --force: it may be a hand measurement.  When fewer than 4 inliers support the
model, nothing is written and the exit status is 1.

--transform similarity | affine estimates that model instead (multipoint_amd.utils.find_transform_pooled and
refine_transform_pooled; fewest inliers 3 | 4).  The yaml stays a 3x3 `perspective` that align_images.py reads as it is (its
last row is then (0, 0, 1)); the report gains `transform` and, for a similarity, `similarity`: the angle, scale, dx and dy of
the optical -> thermal estimate in the convention of multipoint_amd.utils.decompose_similarity.

--method fourier estimates a similarity without keypoints, descriptors or a network (-m and -v are ignored; --transform must
be similarity and is set to it when omitted): Fourier-Mellin phase correlation of the frames' gradient magnitudes, the
normalised cross-power spectra of all pairs added (multipoint_amd.utils.FourierEstimator).  The files are read
twice in --batch chunks, once for the angle and scale and once for the translation.  The report then holds the pairs read /
used, `similarity`, and per stage the peak of the pooled correlation surface, the second-highest value outside its 3 x 3 block
and their ratio, and `branch_180`, whether the theta + pi candidate won.  When either ratio is below --min-peak-ratio nothing is
written and the exit status is 1.  The default floor of 1.1 is a guess: no recording was available to set it on.

--ecc-refine refines the estimate of either method over ALL selected pairs at once: the pooled ECC refinement of
multipoint_amd.utils.estimate_shared_transform_ecc, one group, started from the float64 inverse of the estimate
(thermal -> optical), under --ecc-transform similarity | affine | homography (default homography: many pairs under one transform
determine the eight parameters a single pair does not) on gradient magnitudes blurred with --ecc-filter-size.  The pairs are read
once more in --batch chunks into resident feature planes.  --method ecc --init YAML does the same from an existing
initial_transform.yaml, a hand measurement for instance (-m and -v are ignored).  --auto-mask excludes the pixels of each camera
whose value never changes over the pairs read (the black margin undistortion leaves, a burnt-in overlay), --thermal-mask PNG /
--optical-mask PNG give such masks as 8-bit images (nonzero = use; with --auto-mask the two are intersected); the excluded sets
are grown by the features' support.  After the first run the pairs whose own correlation is below --ecc-reject-ratio times the
median are dropped and the rest runs once more (0: off; the default of 0.5 is a guess like --min-peak-ratio).  The yaml is
written from the refined transform when the refinement succeeded, else from the estimate as without the flag (--method ecc
then writes nothing and exits with 1); the exit status stays that of the estimate.  The report gains `ecc`: model, feature,
filter_size, rho_start, rho_end, iterations, status, rounds, success, per pair rho, valid_share and rejected, the share of
pixels each mask keeps after growth, and corner_shift, the largest displacement in optical pixels of a thermal corner
between the estimate and the refined transform.

Not known: how well this works on real thermal / optical recordings -- no such data and no trained weights are in this
repository; everything is verified on synthetic and planted data.  Look at the report (and at check_alignment.py's pictures)
before trusting the file."""
import argparse
import json
import os
import random
import sys

import numpy as np
import yaml

YAML_NAME = 'initial_transform.yaml'
REPORT_NAME = 'initial_transform_report.json'


class _ExplicitTransform(argparse.Action):
    """--transform, remembering that it was given: --method fourier sets an omitted one to similarity and refuses another."""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        namespace.transform_explicit = True


def build_parser():
    parser = argparse.ArgumentParser(description='Estimate initial_transform.yaml of a directory of image pairs from their pooled matches')
    parser.add_argument('-y', '--yaml-config', default='configs/config_image_pair_dataset_prediction.yaml', help='YAML config file')
    parser.add_argument('-m', '--model-dir', default='model_weights/multipoint', help='Directory of the model')
    parser.add_argument('-v', '--version', default='latest', help='Model version (name of the param file), none for no weights')
    parser.add_argument('-i', '--input-dir', required=True, help='Directory of the <index>_optical.png / <index>_thermal.png pairs')
    parser.add_argument('-o', '--output', default=None, help='The yaml file to write (default: <input-dir>/initial_transform.yaml)')
    parser.add_argument('-s', '--seed', default=0, type=int, help='Seed of the random generators and of the RANSAC sampling')
    parser.add_argument('--max-pairs', default=0, type=int, help='Use this many evenly spaced pairs (0: all)')
    parser.add_argument('--batch', default=8, type=int, help='Pairs per forward')
    parser.add_argument('--max-iters', default=2000, type=int, help='RANSAC hypotheses')
    parser.add_argument('--subpixel', action='store_true', help='Refine the keypoints to sub-pixel positions on the detector map '
                        '(prediction.subpixel.enable): the pooled matches then hold float positions')
    parser.add_argument('--topk-mode', default=None, choices=['score', 'anms'],
                        help="--method matches: which prediction.topk keypoints are kept -- 'score' the highest scores (default), "
                        "'anms' the largest suppression radii, spread over the frame; overrides prediction.topk_mode")
    parser.add_argument('--anms-robust', default=None, type=float,
                        help="with topk_mode 'anms': the robustness factor in (0, 1]; overrides prediction.anms_robust (default 1.0)")
    parser.add_argument('--transform', default='homography', choices=['homography', 'similarity', 'affine'], action=_ExplicitTransform,
                        help='Motion model of the estimate: the 8-parameter homography, a similarity (rotation, scale, two translations: '
                        'what a rigid rig is close to, and what few inliers still determine) or an affine transform')
    parser.add_argument('--force', action='store_true', help='Overwrite an existing yaml file (it may be hand-measured)')
    parser.add_argument('--method', default='matches', choices=['matches', 'fourier', 'ecc'],
                        help='matches: pooled keypoint matches of a network or baseline; fourier: keypoint-free Fourier-Mellin phase '
                        'correlation of the gradient magnitudes, a similarity only (no network: -m and -v are ignored); ecc: the '
                        'pooled ECC refinement of the transform in --init (no network either)')
    parser.add_argument('--min-peak-ratio', default=1.1, type=float,
                        help='--method fourier: write nothing when the highest value of a correlation surface is below this many times '
                        'the second-highest (a guess: not set on a real recording)')
    parser.add_argument('--ecc-refine', action='store_true', help='Refine the estimate over all selected pairs with the pooled ECC '
                        'refinement (implied by --method ecc)')
    parser.add_argument('--ecc-transform', default='homography', choices=['similarity', 'affine', 'homography'],
                        help='Motion model of the ECC refinement')
    parser.add_argument('--ecc-filter-size', default=5, type=int, help='Gaussian blur in front of the gradient magnitude (odd, 1: none)')
    parser.add_argument('--ecc-reject-ratio', default=0.5, type=float,
                        help='Drop the pairs whose correlation is below this many times the median after the first run and run once '
                        'more (0: off; a guess: not set on a real recording)')
    parser.add_argument('--init', default=None, help='--method ecc: the yaml file whose `perspective` the refinement starts from')
    parser.add_argument('--auto-mask', action='store_true', help='ECC: exclude the pixels of each camera that never change over the pairs read')
    parser.add_argument('--thermal-mask', default=None, help='ECC: 8-bit image of the thermal size, nonzero = use')
    parser.add_argument('--optical-mask', default=None, help='ECC: 8-bit image of the optical size, nonzero = use')
    parser.set_defaults(transform_explicit=False)
    return parser


def select_pairs(names, max_pairs):
    """`max_pairs` evenly spaced entries of `names`, the first and the last among them (all of them when max_pairs <= 0 or
    not below their number)."""
    names = list(names)
    if max_pairs <= 0 or max_pairs >= len(names):
        return names
    if max_pairs == 1:
        return names[:1]
    return [names[(i * (len(names) - 1)) // (max_pairs - 1)] for i in range(max_pairs)]


def perspective_from_estimate(H):
    """The matrix align_images.py reads (thermal pixel -> optical pixel, h22 = 1) from the estimated optical -> thermal
    homography: its inverse in float64, divided by its last entry."""
    H = np.asarray(H, np.float64).reshape(3, 3)
    if not np.isfinite(H).all() or abs(np.linalg.det(H)) < 1e-12:
        raise ValueError('the estimated homography is singular')
    T = np.linalg.inv(H)
    if abs(T[2, 2]) < 1e-12:
        raise ValueError('the inverse of the estimated homography has h22 = 0')
    return T / T[2, 2]


def build_report(names_read, names_used, pair_offsets, mask, n_inliers, cost, transform='homography', H=None):
    """The report's fields from the estimator's result: mask [N] per pooled match, pair_offsets [P+1] the rows of every used pair.
    With another `transform` than the homography the report names it, and for a similarity holds the decomposed estimate H."""
    mask = np.asarray(mask).reshape(-1) != 0
    po = np.asarray(pair_offsets).reshape(-1)
    if len(po) != len(names_used) + 1 or int(po[-1]) != len(mask):
        raise ValueError('build_report: %d pairs, %d offsets, %d matches' % (len(names_used), len(po), len(mask)))
    per_pair = {n: int(mask[int(po[p]):int(po[p + 1])].sum()) for p, n in enumerate(names_used)}
    report = {
        'pairs_read': len(names_read),
        'pairs_used': len(names_used),
        'matches_pooled': int(len(mask)),
        'inliers': int(n_inliers),
        'cost_before_polish': None if cost is None else float(cost[0]),
        'cost_after_polish': None if cost is None else float(cost[1]),
        'inliers_per_pair': per_pair,
        'pairs_with_4_inliers': int(sum(v >= 4 for v in per_pair.values())),
    }
    if transform != 'homography':
        report['transform'] = transform
        if transform == 'similarity' and H is not None and np.asarray(H).any():
            from multipoint_amd.utils import decompose_similarity
            report['similarity'] = dict(zip(('angle', 'scale', 'dx', 'dy'), decompose_similarity(H)))
    return report


def estimate_on_gpu(args, config, names):
    """Forward, keypoints, descriptors and matches of the pairs `names` in batches, pooled into one group; then the pooled
    RANSAC and its polish.  Returns (H 3x3 float64 optical -> thermal, mask [N] uint8, pair_offsets [P+1], n_inliers,
    (cost before, cost after))."""
    import torch

    import multipoint_amd.utils as utils
    from multipoint_amd.datasets.image_file_pairs import read_png_pair
    from multipoint_amd.pipeline import PairPipeline
    from multipoint_amd.utils import alignment
    from predict_align_image_pair import load_network, select_device
    device = select_device(config)
    print('Estimating on device: {}'.format(device))
    pred = config['prediction']
    if getattr(args, 'subpixel', False):
        pred = dict(pred, subpixel=dict(pred.get('subpixel') or {}, enable=True))
    if getattr(args, 'topk_mode', None) is not None:
        pred = dict(pred, topk_mode=args.topk_mode)
    if getattr(args, 'anms_robust', None) is not None:
        pred = dict(pred, anms_robust=args.anms_robust)
    utils.topk_selection(pred)              # (refuses an unknown mode, or 'anms' with topk 0, before the network is loaded)
    net = load_network(config, args.model_dir, args.version, device, args.seed)
    pipe = PairPipeline(net, pred)
    pts, counts = [], []
    with torch.no_grad():
        for at in range(0, len(names), max(args.batch, 1)):
            pairs = [read_png_pair(args.input_dir, n) for n in names[at:at + max(args.batch, 1)]]
            if len({p[0].shape[:2] for p in pairs}) != 1 or len({p[1].shape for p in pairs}) != 1:
                raise ValueError('all optical frames of a directory must have one size, and all thermal frames one size')
            optical = torch.stack([alignment.frames_to_float(p[0], device, single_bgr=p[0].ndim == 3) for p in pairs])[:, None]
            thermal = alignment.frames_to_float(np.stack([p[1] for p in pairs]), device).reshape(len(pairs), 1, *pairs[0][1].shape)
            pooled = utils.pool_matches(pipe.run_two_sized(optical.contiguous(), thermal.contiguous()))
            pts.append(pooled.pts)
            po = pooled.pair_offsets.cpu().numpy()
            counts.extend(int(c) for c in po[1:] - po[:-1])
    pair_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n = int(pair_offsets[-1])
    model = getattr(args, 'transform', 'homography')
    if n < utils.TRANSFORM_MIN_POINTS[model]:
        return np.zeros((3, 3)), np.zeros(n, np.uint8), pair_offsets, 0, None
    allp = utils.PooledMatches(torch.cat(pts).contiguous(), None, None, torch.tensor([0, n], dtype=torch.int32, device=device))
    thr = float(pred.get('reprojection_threshold', 3))
    H0, _, _ = utils.find_transform_pooled(allp, model, thr, max_iters=args.max_iters, seed=args.seed)
    H, mask, nin, cost = utils.refine_transform_pooled(allp, H0, model, thr)
    cost = cost[0].cpu().numpy()
    return H[0].cpu().numpy(), mask.cpu().numpy(), pair_offsets, int(nin[0]), (float(cost[0]), float(cost[1]))


def _ratio(peak, second):
    """peak / second of a correlation surface; 0 for a surface without a positive peak."""
    peak, second = float(peak), float(second)
    if not peak > 0.0:
        return 0.0
    return peak / max(second, 1e-30)


def build_fourier_report(names_read, names_used, H, info):
    """The report of --method fourier: H the optical -> thermal similarity, info the estimator's peak1, second1 (angle and scale),
    peak2, second2 (translation) and branch (1: the theta + pi candidate won)."""
    from multipoint_amd.utils import decompose_similarity
    report = {
        'method': 'fourier',
        'transform': 'similarity',
        'pairs_read': len(names_read),
        'pairs_used': len(names_used),
        'stage1': {'peak': float(info['peak1']), 'second': float(info['second1']), 'ratio': _ratio(info['peak1'], info['second1'])},
        'stage2': {'peak': float(info['peak2']), 'second': float(info['second2']), 'ratio': _ratio(info['peak2'], info['second2'])},
        'branch_180': bool(info['branch']),
    }
    H = np.asarray(H, np.float64).reshape(3, 3)
    if np.isfinite(H).all() and H.any():
        report['similarity'] = dict(zip(('angle', 'scale', 'dx', 'dy'), decompose_similarity(H)))
    return report


def estimate_fourier_on_gpu(args, names):
    """The pooled Fourier-Mellin estimate of the pairs `names`, read in --batch chunks: one pass over the files accumulates the
    cross-power sums of the angle-and-scale stage, a second pass those of the translation stage under the estimated similarity and
    its theta + pi twin.  Returns (H 3x3 float64 optical -> thermal, dict(peak1, second1, peak2, second2, branch))."""
    import torch

    from multipoint_amd import _lib
    from multipoint_amd.datasets.image_file_pairs import read_png_pair
    from multipoint_amd.utils import FourierEstimator, alignment
    device = _lib.require_cuda()
    print('Estimating on device: {}'.format(device))
    batch = max(args.batch, 1)

    def chunks():
        for at in range(0, len(names), batch):
            pairs = [read_png_pair(args.input_dir, n) for n in names[at:at + batch]]
            optical = torch.stack([alignment.frames_to_float(p[0], device, single_bgr=p[0].ndim == 3) for p in pairs])
            thermal = alignment.frames_to_float(np.stack([p[1] for p in pairs]), device).reshape(len(pairs), *pairs[0][1].shape)
            yield optical.contiguous(), thermal.contiguous()

    est = None
    for optical, thermal in chunks():
        if est is None:
            est = FourierEstimator(optical.shape[1:], thermal.shape[1:])
        est.add_stage1(optical, thermal)
    est.finish_stage1()
    for optical, thermal in chunks():
        est.add_stage2(optical, thermal)
    T, rep = est.finish()
    return T[0], dict(peak1=rep.peak1[0], second1=rep.second1[0], peak2=rep.peak2[0], second2=rep.second2[0], branch=int(rep.branch[0]))


def read_mask(path):
    """An 8-bit mask image as a uint8 array (H, W), nonzero = use."""
    from PIL import Image
    with Image.open(path) as im:
        return (np.array(im.convert('L'), np.uint8) != 0).astype(np.uint8)


def refine_ecc_on_gpu(args, names, T_est):
    """The pooled ECC refinement of T_est (3x3 float64, thermal -> optical) over the pairs `names`, read once in --batch chunks
    into resident feature planes, one group.  Returns (T refined 3x3 float64 with h22 = 1, the report's `ecc` object)."""
    import torch

    from multipoint_amd import _lib
    from multipoint_amd.datasets.image_file_pairs import read_png_pair
    from multipoint_amd.utils import SharedEccProblem, alignment
    device = _lib.require_cuda()
    print('Refining on device: {}'.format(device))
    batch = max(args.batch, 1)
    prob = SharedEccProblem('gradient', args.ecc_filter_size, auto_mask=args.auto_mask)
    for at in range(0, len(names), batch):
        pairs = [read_png_pair(args.input_dir, n) for n in names[at:at + batch]]
        if len({p[0].shape[:2] for p in pairs}) != 1 or len({p[1].shape for p in pairs}) != 1:
            raise ValueError('all optical frames of a directory must have one size, and all thermal frames one size')
        optical = torch.stack([alignment.frames_to_float(p[0], device, single_bgr=p[0].ndim == 3) for p in pairs])
        thermal = alignment.frames_to_float(np.stack([p[1] for p in pairs]), device).reshape(len(pairs), *pairs[0][1].shape)
        prob.add(optical.contiguous(), thermal.contiguous())
    prob.finish(None if args.thermal_mask is None else read_mask(args.thermal_mask),
                None if args.optical_mask is None else read_mask(args.optical_mask))
    rho_start = prob.correlation(T_est)[0][0]
    r = prob.refine(T_est, args.ecc_transform, reject_ratio=args.ecc_reject_ratio)
    T = r.transform[0] / r.transform[0][2, 2]
    H, W = prob.thw
    corners = np.array([[0, 0, 1], [W - 1, 0, 1], [0, H - 1, 1], [W - 1, H - 1, 1]], np.float64).T
    a, b = np.asarray(T_est, np.float64) @ corners, T @ corners
    kept = float(H * W) * prob.thermal_kept[0]

    def number(v):
        return float(v) if np.isfinite(v) else None

    report = {
        'model': args.ecc_transform, 'feature': 'gradient', 'filter_size': int(args.ecc_filter_size),
        'rho_start': number(rho_start), 'rho_end': number(r.rho[0]), 'iterations': int(r.nit[0]), 'status': int(r.status[0]),
        'success': bool(r.success[0]), 'converged': bool(r.converged[0]), 'rounds': int(r.rounds),
        'reject_ratio': float(args.ecc_reject_ratio),
        'pairs': {n: {'rho': number(r.rho_pair[i]), 'valid_share': float(r.valid_pair[i]) / max(kept, 1.0),
                      'rejected': bool(r.rejected[i])} for i, n in enumerate(names)},
        'thermal_mask_kept': float(prob.thermal_kept[0]), 'optical_mask_kept': float(prob.optical_kept[0]),
        'corner_shift': float(np.max(np.hypot(*(a[:2] / a[2] - b[:2] / b[2])))) if r.success[0] else None,
    }
    return T, report


def apply_ecc(args, names, T_est, refiner):
    """(the transform to write, the report's `ecc` object): the refined transform when the refinement succeeded, else T_est."""
    T, ecc = refiner(args, names, T_est)
    print('ECC {model}: rho {rho_start} -> {rho_end}  iterations {iterations}  status {status}  rounds {rounds}'.format(**ecc))
    rejected = [n for n, v in ecc['pairs'].items() if v['rejected']]
    if rejected:
        print('ECC rejected pairs: {}'.format(' '.join(rejected)))
    if not ecc['success']:
        print('the ECC refinement failed (status %d): the estimate is kept' % ecc['status'], file=sys.stderr)
        return T_est, ecc
    print('ECC moved the thermal corners by at most {:.3f} optical px'.format(ecc['corner_shift']))
    return np.asarray(T, np.float64), ecc


def main_ecc(args, out_yaml, out_report, refiner):
    """--method ecc: the refinement alone, from the `perspective` of --init."""
    from multipoint_amd.datasets.image_file_pairs import ImageFilePairs
    with open(args.init, 'r') as fh:
        T_est = np.array(yaml.safe_load(fh)['perspective'], np.float64)
    if T_est.shape != (3, 3) or not np.isfinite(T_est).all() or T_est[2, 2] == 0:
        print('%s holds no 3x3 `perspective`' % args.init, file=sys.stderr)
        return 2
    names_read = ImageFilePairs({'directory': args.input_dir}).memberslist
    names = select_pairs(names_read, args.max_pairs)
    if not names:
        print('no <index>_optical.png / <index>_thermal.png pairs in %s' % args.input_dir, file=sys.stderr)
        return 1
    print('Using {} of {} pairs'.format(len(names), len(names_read)))
    T, ecc = apply_ecc(args, names, T_est / T_est[2, 2], refiner)
    report = {'method': 'ecc', 'transform': args.ecc_transform, 'pairs_read': len(names_read), 'pairs_used': len(names), 'ecc': ecc}
    if not ecc['success']:
        print('nothing written', file=sys.stderr)
        return 1
    print('perspective (thermal -> optical):')
    print(T)
    with open(out_yaml, 'wt') as fh:
        yaml.safe_dump({'perspective': [[float(v) for v in row] for row in T]}, fh)
    with open(out_report, 'wt') as fh:
        json.dump(report, fh, indent=1, sort_keys=True)
    print('Wrote {} and {}'.format(out_yaml, out_report))
    return 0


def main_fourier(args, out_yaml, out_report, estimator, refiner=refine_ecc_on_gpu):
    from multipoint_amd.datasets.image_file_pairs import ImageFilePairs
    names_read = ImageFilePairs({'directory': args.input_dir}).memberslist
    names = select_pairs(names_read, args.max_pairs)
    if not names:
        print('no <index>_optical.png / <index>_thermal.png pairs in %s' % args.input_dir, file=sys.stderr)
        return 1
    print('Using {} of {} pairs'.format(len(names), len(names_read)))
    H, info = estimator(args, names)
    report = build_fourier_report(names_read, names, H, info)
    for stage in ('stage1', 'stage2'):
        print('{}: peak {peak:.4f}  second {second:.4f}  ratio {ratio:.3f}'.format(stage, **report[stage]))
    low = [stage for stage in ('stage1', 'stage2') if not report[stage]['ratio'] >= args.min_peak_ratio]
    if low or 'similarity' not in report:
        print('the correlation peak of %s is below %g times the second-highest value: nothing written'
              % (' and '.join(low) or 'no stage', args.min_peak_ratio), file=sys.stderr)
        return 1
    T = perspective_from_estimate(H)
    print('Similarity: angle {angle:.6f} rad  scale {scale:.6f}  dx {dx:.3f}  dy {dy:.3f}'.format(**report['similarity']))
    print('Estimated similarity transform (optical -> thermal):')
    print(np.asarray(H))
    if args.ecc_refine:
        T, report['ecc'] = apply_ecc(args, names, T, refiner)
    print('perspective (thermal -> optical):')
    print(T)
    with open(out_yaml, 'wt') as fh:
        yaml.safe_dump({'perspective': [[float(v) for v in row] for row in T]}, fh)
    with open(out_report, 'wt') as fh:
        json.dump(report, fh, indent=1, sort_keys=True)
    print('Wrote {} and {}'.format(out_yaml, out_report))
    return 0


def main(argv=None, estimator=estimate_on_gpu, fourier_estimator=estimate_fourier_on_gpu, ecc_refiner=refine_ecc_on_gpu):
    args = build_parser().parse_args(argv)
    if args.method == 'ecc':
        if not args.init:
            print('--method ecc refines an existing transform: --init YAML is required', file=sys.stderr)
            return 2
        args.ecc_refine = True
    elif args.init:
        print('--init belongs to --method ecc', file=sys.stderr)
        return 2
    if not args.ecc_refine and (args.auto_mask or args.thermal_mask or args.optical_mask):
        print('--auto-mask, --thermal-mask and --optical-mask belong to --ecc-refine and --method ecc', file=sys.stderr)
        return 2
    if args.ecc_refine and (args.ecc_filter_size % 2 == 0 or not 1 <= args.ecc_filter_size <= 31
                            or not 0.0 <= args.ecc_reject_ratio <= 1.0):
        print('--ecc-filter-size must be odd and in [1, 31], --ecc-reject-ratio in [0, 1]', file=sys.stderr)
        return 2
    if args.method == 'fourier':
        if args.transform_explicit and args.transform != 'similarity':
            print('--method fourier estimates a similarity: --transform %s is not available' % args.transform, file=sys.stderr)
            return 2
        args.transform = 'similarity'
    random.seed(args.seed)
    np.random.seed(args.seed)
    out_yaml = args.output or os.path.join(args.input_dir, YAML_NAME)
    out_report = os.path.join(os.path.dirname(out_yaml) or '.', REPORT_NAME)
    if os.path.exists(out_yaml) and not args.force:
        print('%s exists (it may be hand-measured): pass --force to overwrite it' % out_yaml, file=sys.stderr)
        return 2
    if args.method == 'fourier':
        return main_fourier(args, out_yaml, out_report, fourier_estimator, ecc_refiner)
    if args.method == 'ecc':
        return main_ecc(args, out_yaml, out_report, ecc_refiner)
    with open(args.yaml_config, 'r') as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    with open(os.path.join(args.model_dir, 'params.yaml'), 'r') as f:
        config['model'] = yaml.load(f, Loader=yaml.FullLoader)['model']      # overwrite the model params
    from multipoint_amd.datasets.image_file_pairs import ImageFilePairs
    names_read = ImageFilePairs({'directory': args.input_dir}).memberslist
    names = select_pairs(names_read, args.max_pairs)
    if not names:
        print('no <index>_optical.png / <index>_thermal.png pairs in %s' % args.input_dir, file=sys.stderr)
        return 1
    print('Using {} of {} pairs'.format(len(names), len(names_read)))
    H, mask, pair_offsets, n_inliers, cost = estimator(args, config, names)
    from multipoint_amd.utils import transform_min_inliers
    min_inliers = transform_min_inliers(args.transform)
    report = build_report(names_read, names, pair_offsets, mask, n_inliers, cost, args.transform, H)
    print('Matches pooled: {}  inliers: {}  pairs with at least 4 inliers: {} of {}'.format(
        report['matches_pooled'], report['inliers'], report['pairs_with_4_inliers'], report['pairs_used']))
    if n_inliers < min_inliers:
        print('fewer than %d inliers support a model: nothing written' % min_inliers, file=sys.stderr)
        return 1
    T = perspective_from_estimate(H)
    if 'similarity' in report:
        print('Similarity: angle {angle:.6f} rad  scale {scale:.6f}  dx {dx:.3f}  dy {dy:.3f}'.format(**report['similarity']))
    print('Estimated Homography (optical -> thermal):' if args.transform == 'homography' else
          'Estimated %s transform (optical -> thermal):' % args.transform)
    print(np.asarray(H))
    if args.ecc_refine:
        T, report['ecc'] = apply_ecc(args, names, T, ecc_refiner)
    print('perspective (thermal -> optical):')
    print(T)
    with open(out_yaml, 'wt') as fh:
        yaml.safe_dump({'perspective': [[float(v) for v in row] for row in T]}, fh)
    with open(out_report, 'wt') as fh:
        json.dump(report, fh, indent=1, sort_keys=True)
    print('Wrote {} and {}'.format(out_yaml, out_report))
    return 0


if __name__ == '__main__':
    sys.exit(main())
