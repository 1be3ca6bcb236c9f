"""GPU: the command lines that write result views on tiny frames with random weights (-v none): the files they
write, their sizes, and pictures recomputed from what the same run saved."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

import drawing_restatement as R
import pyramid_restatement as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 64, 96


def _run(script, *args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + [str(a) for a in args], capture_output=True, text=True,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def _png(path):
    with Image.open(str(path)) as im:
        return np.array(im)


@pytest.fixture()
def setup(tmp_path):
    d = tmp_path / 'multipoint'
    d.mkdir()
    with open(os.path.join(ROOT, 'model_weights', 'multipoint', 'params.yaml')) as f:
        (d / 'params.yaml').write_text(f.read())
    cfg = yaml.safe_load(open(os.path.join(ROOT, 'configs', 'config_image_pair_dataset_prediction.yaml')))
    cfg['dataset'].update({'num_samples': 2, 'height': H, 'width': W})
    cfg['dataset']['augmentation']['homographic']['enable'] = False
    # random weights give a flat heat map around 1 / 65: a low threshold and the 40 best keep the lists short and non-empty
    cfg['prediction'].update({'topk': 40, 'batchsize': 2, 'detection_threshold': 0.001, 'num_worker': 0})
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    return tmp_path, cfg


def test_predict_align_image_pair_plots(setup):
    from multipoint_amd.datasets import SyntheticPairs
    from multipoint_amd.utils import drawing
    tmp, cfg = setup
    plots, npz = tmp / 'plots', tmp / 'out.npz'
    out = _run('predict_align_image_pair.py', '-y', tmp / 'cfg.yaml', '-m', tmp / 'multipoint', '-v', 'none', '-i', 1, '-p',
               '-r', 3, '--plot-dir', plots, '--save-npz', npz)
    names = ['matches.png', 'matches_inliers.png', 'overlay_anaglyph.png', 'overlay_checker.png', 'warped_optical.png']
    assert sorted(os.listdir(str(plots))) == names and 'Wrote matches.png' in out
    g = np.load(str(npz))
    assert len(g['match_query']) > 0
    pictures = {n: _png(plots / n) for n in names}
    assert pictures['matches.png'].shape == pictures['matches_inliers.png'].shape == (H, 2 * W, 3)
    for n in names[2:]:
        assert pictures[n].shape == (H, W, 3) and pictures[n].dtype == np.uint8
    # matches.png from the lists of the same run: one keypoint pair per match, in match order
    o, t = SyntheticPairs.make_pair(0, 1, H, W)
    kp_a, kp_b = g['kp_optical'][g['match_query']][None], g['kp_thermal'][g['match_train']][None]
    M = kp_a.shape[1]
    want = R.match_picture(o, t, kp_a, kp_b, (M,), (M,), np.arange(M)[None], None, 3, 1, drawing.match_palette(64))
    assert np.array_equal(pictures['matches.png'], want[0])
    got = drawing.draw_matches(torch.from_numpy(o).cuda(), torch.from_numpy(t).cuda(), kp_a, kp_b, np.arange(M), radius=3)
    assert np.array_equal(got[0].cpu().numpy(), pictures['matches.png'])
    # the inlier picture marks a subset of those pixels, on the same two images
    plain = R.gray_to_rgb(np.zeros((1, H, 2 * W, 3), np.uint8), np.concatenate([o, t], 2))[0]
    marked, marked_inliers = (want[0] != plain).any(-1), (pictures['matches_inliers.png'] != plain).any(-1)
    assert marked.any() and not (marked_inliers & ~marked).any()
    # the warped image is the npz's, the anaglyph carries the thermal image in green and blue
    assert np.array_equal(pictures['warped_optical.png'][..., 0], R.gray_values(g['warped_optical']))
    assert np.array_equal(pictures['overlay_anaglyph.png'][..., 1], R.gray_values(t[0]))
    assert np.array_equal(pictures['overlay_anaglyph.png'][..., 2], R.gray_values(t[0]))
    # without the new flag nothing is written and the text is what it was
    plain = _run('predict_align_image_pair.py', '-y', tmp / 'cfg.yaml', '-m', tmp / 'multipoint', '-v', 'none', '-i', 1, '-p')
    assert 'Wrote' not in plain and 'Estimated Homography:' in plain


def test_predict_keypoints_plots(setup):
    import multipoint_amd.datasets as datasets
    import multipoint_amd.utils as utils
    from predict_align_image_pair import load_network
    tmp, cfg = setup
    plots = tmp / 'plots'
    out = _run('predict_keypoints.py', '-y', tmp / 'cfg.yaml', '-m', tmp / 'multipoint', '-v', 'none', '-b', '-p', '--plot-dir', plots,
               '-r', 3, '-mask')
    want = sorted('%d_%s_%s.png' % (i, v, s) for i in (0, 1) for v in ('image', 'prob', 'prob_masked') for s in ('optical', 'thermal'))
    assert sorted(os.listdir(str(plots))) == want and 'Wrote 12 pictures' in out
    for n in want:
        assert _png(plots / n).shape == (H, W, 3)
    # sample 1, optical, recomputed: the same network and post-processing in this process, the picture by the restatement
    cfg['model'] = yaml.safe_load(open(str(tmp / 'multipoint' / 'params.yaml')))['model']
    pred = cfg['prediction']
    dataset = datasets.SyntheticPairs(cfg['dataset'])
    loader = torch.utils.data.DataLoader(dataset, batch_size=2, shuffle=False, num_workers=0)
    data = utils.data_to_device(next(iter(loader)), torch.device('cuda:0'))      # the batch the command line predicted
    assert 'keypoints' not in data['optical']
    net = load_network(cfg, str(tmp / 'multipoint'), 'none', torch.device('cuda:0'), 0)
    with torch.no_grad():
        o = net(data['optical'])
        prob = utils.box_nms_tie_robust(net, data['optical'], o, pred['nms'], pred['detection_threshold'], keep_top_k=pred['topk'],
                                        on_cpu=pred['cpu_nms']).reshape(2, H, W)[1].cpu().numpy()
    image = data['optical']['image'].reshape(2, H, W)[1:].cpu().numpy()
    mask = data['optical']['valid_mask'].reshape(2, H, W)[1:].cpu().numpy().astype(np.float32)
    gain = 0.9 / pred['detection_threshold']
    assert np.array_equal(_png(plots / '1_prob_optical.png')[..., 0], R.gray_values(prob, None, gain))
    assert np.array_equal(_png(plots / '1_prob_masked_optical.png')[..., 1], R.gray_values(prob[None], mask, gain)[0])
    kp = np.argwhere((prob > pred['detection_threshold']) * mask[0])
    assert 0 < len(kp) <= 40
    canvas = R.gray_to_rgb(np.zeros((1, H, W, 3), np.uint8), image, mask)
    R.draw_marks(canvas, kp[None], (len(kp),), 3, 1, 'ring', [(0, 255, 0)])
    assert np.array_equal(_png(plots / '1_image_optical.png'), canvas[0])
    # without --plot-dir, -p stays a text summary
    assert 'Wrote' not in _run('predict_keypoints.py', '-y', tmp / 'cfg.yaml', '-m', tmp / 'multipoint', '-v', 'none', '-p')


def test_show_scripts(tmp_path):
    rng = np.random.default_rng(3)
    arrays, labels = {}, {}
    for i in range(2):
        arrays['s%d/optical' % i] = rng.random((40, 56), dtype=np.float32)
        arrays['s%d/thermal' % i] = rng.random((40, 56), dtype=np.float32)
        labels['s%d/keypoints' % i] = np.stack([rng.integers(0, 40, 9), rng.integers(0, 56, 9)], axis=1)
    np.savez(str(tmp_path / 'd.npz'), **arrays)
    np.savez(str(tmp_path / 'k.npz'), **labels)
    out = _run('show_keypoints.py', '-d', tmp_path / 'd.npz', '-k', tmp_path / 'k.npz', '-n', 1, '-r', 3, '-o', tmp_path / 'a')
    assert 'Number of keypoints: 9' in out
    assert sorted(os.listdir(str(tmp_path / 'a'))) == ['1_optical.png', '1_optical_masked.png', '1_thermal.png', '1_thermal_masked.png']
    for side in ('optical', 'thermal'):
        want = R.gray_to_rgb(np.zeros((1, 40, 56, 3), np.uint8), arrays['s1/' + side][None])
        R.draw_marks(want, labels['s1/keypoints'][None], (9,), 3, 1, 'ring', [(0, 255, 0)])
        assert np.array_equal(_png(tmp_path / 'a' / ('1_%s.png' % side)), want[0])
        assert np.array_equal(_png(tmp_path / 'a' / ('1_%s_masked.png' % side)), want[0])      # no augmentation: the mask is all ones
    _run('show_image_pair_sample.py', '-i', tmp_path / 'd.npz', '-k', tmp_path / 'k.npz', '-n', 0, '-r', 4, '-o', tmp_path / 'b')
    assert sorted(os.listdir(str(tmp_path / 'b'))) == ['0_optical.png', '0_optical_masked.png', '0_single.png', '0_single_masked.png',
                                                       '0_thermal.png', '0_thermal_masked.png']
    kp = np.argwhere(np.isin(np.arange(40 * 56).reshape(40, 56), labels['s0/keypoints'][:, 0] * 56 + labels['s0/keypoints'][:, 1]))
    for side in ('optical', 'thermal'):                      # blue rings of thickness 5 on the labels, in torch.nonzero's order
        want = R.gray_to_rgb(np.zeros((1, 40, 56, 3), np.uint8), arrays['s0/' + side][None])
        R.draw_marks(want, kp[None], (len(kp),), 4, 5, 'ring', [(0, 0, 255)])
        assert np.array_equal(_png(tmp_path / 'b' / ('0_%s.png' % side)), want[0])
    single = _png(tmp_path / 'b' / '0_single.png')
    wants = []
    for side in ('optical', 'thermal'):                      # the single image is one of the two, drawn at random; thickness 3
        want = R.gray_to_rgb(np.zeros((1, 40, 56, 3), np.uint8), arrays['s0/' + side][None])
        wants.append(R.draw_marks(want, kp[None], (len(kp),), 4, 3, 'ring', [(0, 0, 255)])[0])
    assert any(np.array_equal(single, w) for w in wants)
    # the keypoint file is optional
    _run('show_image_pair_sample.py', '-i', tmp_path / 'd.npz', '-n', 0, '-o', tmp_path / 'c')
    assert np.array_equal(_png(tmp_path / 'c' / '0_thermal.png')[..., 0], R.gray_values(arrays['s0/thermal']))


def test_align_candidates_and_review(tmp_path):
    src, dst = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    T_init = None
    for index, seed, colour in (('000', 11, False), ('001', 5, True)):
        opt, th, _, T_init = P.displaced_pair(seed)                # 96 x 128
        o8 = np.rint(opt * 255).astype(np.uint8)
        Image.fromarray(np.stack([o8] * 3, -1) if colour else o8).save(str(src / (index + '_optical.png')))
        Image.fromarray(np.rint(np.clip(th, 0, 1) * 65535).astype(np.uint16)).save(str(src / (index + '_thermal.png')))
    (src / 'initial_transform.yaml').write_text(yaml.safe_dump({'perspective': T_init.tolist()}))
    cfg = dict(P.PARAMS, alignment_method='mi', perspective=True, save_aligned_images=True, use_image_pyramid=False)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    _run('align_images.py', '-y', tmp_path / 'cfg.yaml', '-i', src, '-o', dst, '--save-candidates')
    best, every = dst / 'aligned' / 'best', dst / 'aligned' / 'all'
    assert sorted(os.listdir(str(best))) == ['000_optical.png', '000_thermal.png', '001_optical.png', '001_thermal.png']
    alternatives = sorted(os.listdir(str(every)))
    # accept_init makes the initial transform candidate 0 of every pair; candidate files are numbered without gaps
    for index in ('000', '001'):
        mine = [a for a in alternatives if a.startswith(index + '_optical_')]
        assert mine == ['%s_optical_%d.png' % (index, i) for i in range(len(mine))] and len(mine) >= 1
        assert _png(every / mine[0]).shape == _png(best / (index + '_optical.png')).shape
        assert any(np.array_equal(_png(every / a), _png(best / (index + '_optical.png'))) for a in mine)      # the best is one of them
    out = _run('check_alignment.py', '-i', dst, '-dt', 250)
    assert 'review pictures of 2 pairs' in out
    review = dst / 'review'
    expected = ['000.gif', '000.png', '001.gif', '001.png', 'decisions_template.txt'] + [a.replace('_optical_', '_').replace('.png', '.gif')
                                                                                         for a in alternatives]
    assert sorted(os.listdir(str(review))) == sorted(expected)
    assert (review / 'decisions_template.txt').read_text() == '000 ?\n001 ?\n'
    for name in (e for e in expected if e.endswith('.gif')):
        with Image.open(str(review / name)) as im:
            assert im.n_frames == 2 and im.size == (128, 96) and im.info['duration'] == 250 and im.info.get('loop') == 0
    for index in ('000', '001'):
        sheet = _png(review / (index + '.png'))
        assert sheet.shape == (96, 4 * 128, 3)
        thermal = (_png(best / (index + '_thermal.png')).astype(np.float32) / np.float32(65535.0))
        assert np.array_equal(sheet[:, 128:256, 0], R.gray_values(thermal))
        assert np.array_equal(sheet[:, 384:, 1], R.gray_values(thermal)) and np.array_equal(sheet[:, 384:, 0], sheet[:, :128, 0])
    # a pair that is decided is left out of the next review
    (dst / 'decisions.txt').write_text('000 a\n001 ?\n')
    assert 'Accepted 1 images out of 2' in _run('check_alignment.py', '-i', dst, '--decisions', dst / 'decisions.txt')
    assert sorted(os.listdir(str(dst / 'aligned' / 'accepted'))) == ['000_optical.png', '000_thermal.png']
    assert 'review pictures of 1 pairs' in _run('check_alignment.py', '-i', dst, '--review-dir', tmp_path / 'again')
    assert sorted(f for f in os.listdir(str(tmp_path / 'again')) if '_' not in f) == ['001.gif', '001.png']
