"""CPU: the oracle and the product's host code against what the reference's own code returned -- state-dict layouts,
forwards, host helpers, matchers and its evaluation / homographic-adaptation drivers -- stored in
tests/golden/reference_drivers.npz by tests/golden/make_golden_reference.py (which imports the reference, with the oracle
serving its absent third-party calls).  Inputs are rebuilt here from the same seeds."""
import collections
import json
import os

import numpy as np
import pytest
import torch


@pytest.fixture(scope='module')
def ref(golden_dir):
    """the reference's results: name -> array (json-encoded strings decoded by layout() / text())"""
    with np.load(os.path.join(golden_dir, 'reference_drivers.npz')) as g:
        return {k: g[k] for k in g.files}


def layout(ref, prefix):
    """the reference model's state_dict layout: [(key, shape tuple, dtype string)]"""
    shapes = json.loads(str(ref[prefix + '__shapes']))
    return [(str(k), tuple(s), str(d)) for k, s, d in zip(ref[prefix + '__keys'], shapes, ref[prefix + '__dtypes'])]


def text(ref, key):
    return json.loads(str(ref[key]))


def test_state_dict_layout_and_forward(oracle, ref):
    cfg = dict(oracle.SHIPPED_MODEL_CONFIG)
    spec = oracle.state_dict_spec(cfg)
    rsd = layout(ref, 'shipped')
    assert [k for k, _, _ in spec] == [k for k, _, _ in rsd]
    for (k, s, d), (_, rs, rd) in zip(spec, rsd):
        assert rs == tuple(s) and rd == str(d)
    sd = oracle.make_weights(21, cfg)
    img = oracle.make_images(22, 2, 48, 64)
    r = {k: torch.from_numpy(ref['shipped__' + k]) for k in ('prob', 'desc')}
    o = oracle.forward(sd, img, cfg)
    assert (r['prob'] - o['prob']).abs().max().item() <= 1e-7
    assert (r['desc'] - o['desc']).abs().max().item() <= 1e-7


def test_multispectral_default_config(oracle, ref):
    cfg = {'multispectral': True, 'descriptor_size': 128}
    spec = oracle.state_dict_spec(cfg)
    assert [k for k, _, _ in spec] == [k for k, _, _ in layout(ref, 'multispectral')]
    sd = oracle.make_weights(5, cfg)
    img = oracle.make_images(6, 4, 24, 32)
    flags = torch.tensor([[True], [False], [False], [True]])
    r = {k: torch.from_numpy(ref['multispectral__' + k]) for k in ('prob', 'desc')}
    o = oracle.forward(sd, img, cfg, is_optical=flags)
    assert (r['prob'] - o['prob']).abs().max().item() <= 1e-7
    assert (r['desc'] - o['desc']).abs().max().item() <= 1e-7


def test_interpolate_and_matcher(oracle, ref):
    from multipoint_amd.utils import NNMatcher
    rng = np.random.default_rng(1)
    desc = rng.standard_normal((16, 60, 80)).astype(np.float32)
    kp = np.stack([rng.integers(0, 480, 500), rng.integers(0, 640, 500)], 1).astype(np.int64)
    kp_in = kp.copy()
    r = ref['interp__desc']
    assert np.abs(oracle.interpolate_descriptors(kp_in, desc, 480, 640) - r).max() <= 1e-6
    assert np.array_equal(kp_in, kp)                             # the reference does not mutate its input, nor may the oracle
    d1 = r[:250]; d2 = r[200:]
    q, t, d = oracle.nn_match(d1, d2, 0.7)
    assert list(ref['interp__nn_query']) == list(q) and list(ref['interp__nn_train']) == list(t)
    assert np.allclose(ref['interp__nn_distance'], d, atol=1e-7)
    assert bool(ref['interp__nn_negative_raises'])              # the reference refuses a negative threshold, and so does the product
    with pytest.raises(ValueError):
        NNMatcher(-1.0)


def test_product_host_helpers_match_reference(ref):
    """dict_update / fix_model_weigth_keys / depth_to_space of the product package vs the reference."""
    import multipoint_amd.utils as U
    a = {'a': 1, 'b': {'c': 2, 'd': 3}}; b = {'b': {'c': 5}, 'e': 6}
    import copy
    assert U.dict_update(copy.deepcopy(a), b) == text(ref, 'helpers__dict_update')
    w = collections.OrderedDict([('module__encoder.1.weight', 1), ('x__y__detector.4.bias', 2), ('plain', 3)])
    assert [list(kv) for kv in U.fix_model_weigth_keys(w).items()] == text(ref, 'helpers__fix_keys')
    x = torch.from_numpy(ref['helpers__d2s_in'])
    assert torch.equal(U.depth_to_space(x, 8), torch.from_numpy(ref['helpers__d2s_out']))
    assert torch.equal(U.space_to_depth(U.depth_to_space(x, 8), 8), x)
    x = torch.randn(2, 64, 3, 4)
    assert torch.equal(U.space_to_depth(U.depth_to_space(x, 8), 8), x)
    import multipoint_amd.models as M
    assert json.loads(json.dumps(M.MultiPoint.default_config)) == text(ref, 'helpers__default_config')
    for i, cfg in enumerate(({'multispectral': False, 'descriptor_size': 64}, {'bn_first': True}, {'final_batchnorm': False})):
        ours = M.MultiPoint(dict(cfg)).state_dict_spec()
        theirs = layout(ref, 'helpers_cfg%d' % i)
        assert [k for k, _, _ in ours] == [k for k, _, _ in theirs]
        assert all(rs == tuple(s) for (_, s, _), (_, rs, _) in zip(ours, theirs))


def test_magicleap_vs_reference(oracle, ref):
    sd = oracle.make_weights_magicleap(8)
    assert [k for k, _, _ in layout(ref, 'magicleap')] == list(sd.keys())
    assert [s for _, s, _ in layout(ref, 'magicleap')] == [tuple(v.shape) for v in sd.values()]
    img = oracle.make_images(9, 2, 24, 32)
    r = {k: torch.from_numpy(ref['magicleap__' + k]) for k in ('logits', 'desc', 'prob')}
    o = oracle.forward_magicleap(sd, img)
    for k in ('logits', 'desc', 'prob'):
        assert (r[k] - o[k]).abs().max().item() <= 1e-6
    import multipoint_amd.models as M
    assert [k for k, _, _ in M.SuperPointMagicLeap().state_dict_spec()] == list(sd.keys())


def test_descriptor_metrics_against_reference_driver(oracle, ref):
    """The REFERENCE's own compute_descriptor_metrics (multipoint/utils/evaluation.py:209-439), run on CPU with the absent
    third-party calls (torchvision nms, cv2 BFMatcher / perspectiveTransform) served by the oracle's restatements, against
    the oracle per pair + the product's host bookkeeping -- so this pins the bookkeeping (ground-truth homography, correctness
    matrices, n_gt, true positives, M-score, precision/recall, NN-mAP), not the third-party arithmetic."""
    cfg = dict(oracle.SHIPPED_MODEL_CONFIG)
    sd = oracle.make_weights(31, cfg)
    H, W, B = 96, 128, 3
    rng = np.random.default_rng(5)
    opt = oracle.make_images(41, B, H, W)
    th = (opt + 0.02 * torch.from_numpy(rng.standard_normal(opt.shape).astype(np.float32))).clamp(0, 1)
    ho = torch.eye(3).repeat(B, 1, 1); ht = torch.eye(3).repeat(B, 1, 1)
    ht[:, 0, 2] = torch.tensor([0.0, 1.0, -2.0]); ht[1, 0, 0] = 1.01
    r = {k[len('descmetrics__'):]: v for k, v in ref.items() if k.startswith('descmetrics__')}

    from multipoint_amd.utils.evaluation import summarize_descriptor_metrics
    pairs = oracle.process_pairs(sd, cfg, opt, th, nms=4, detection_threshold=0.015, topk=150)
    tp_o, tp_t, dist, ms_o, ms_t, ngo, ngt = [], [], [], [], [], 0, 0
    for p, rec in enumerate(pairs):
        m = oracle.descriptor_metrics_pair(rec['kp_optical'], rec['kp_thermal'], rec['match_query'], rec['match_train'],
                                           ho[p], ht[p], 4.0, H, W)
        tp_o.append(m['tp_optical']); tp_t.append(m['tp_thermal']); dist.append(rec['match_dist'])
        ngo += m['n_gt_optical']; ngt += m['n_gt_thermal']
        ms_o.append(m['tp_optical'].sum() / m['N_optical'] if m['N_optical'] else 0.0)
        ms_t.append(m['tp_thermal'].sum() / m['N_thermal'] if m['N_thermal'] else 0.0)
    d = np.concatenate(dist)
    mine = summarize_descriptor_metrics(np.concatenate(tp_o), d, np.concatenate(tp_t), d, ngo, ngt, np.array(ms_o), np.array(ms_t))
    assert len(r['tp_optical']) == len(mine['tp_optical']) > 50
    assert r['tp_optical'].sum() == mine['tp_optical'].sum() and r['tp_thermal'].sum() == mine['tp_thermal'].sum()
    assert 0 < r['tp_optical'].sum() < len(r['tp_optical'])               # the case exercises true AND false positives
    # (the driver's BFMatcher stub returns ||a-b||, process_pairs the NNMatcher form sqrt(2-2ab): equal to ~1e-5 near 0)
    assert np.allclose(np.sort(r['distance_optical']), np.sort(mine['distance_optical']), atol=1e-4)
    assert np.allclose(r['m_score_optical'], mine['m_score_optical']) and np.allclose(r['m_score_thermal'], mine['m_score_thermal'])
    assert abs(r['m_score'] - mine['m_score']) < 1e-12
    assert abs(r['nn_map_optical'] - mine['nn_map_optical']) < 1e-6 and abs(r['nn_map_thermal'] - mine['nn_map_thermal']) < 1e-6
    assert np.allclose(r['recall_optical'][-2], mine['recall_optical'][-2])


def test_repeatability_against_reference_driver(oracle, ref):
    """The reference's compute_repeatability_multispectral (evaluation.py:105-200), run with oracle stubs for the absent
    torchvision / cv2 calls, against oracle.repeatability_pair on the oracle's own keypoints."""
    cfg = dict(oracle.SHIPPED_MODEL_CONFIG)
    sd = oracle.make_weights(33, cfg)
    H, W, B = 96, 128, 3
    rng = np.random.default_rng(6)
    opt = oracle.make_images(43, B, H, W)
    th = (opt + 0.02 * torch.from_numpy(rng.standard_normal(opt.shape).astype(np.float32))).clamp(0, 1)
    ho = torch.eye(3).repeat(B, 1, 1); ht = torch.eye(3).repeat(B, 1, 1)
    ht[:, 0, 2] = torch.tensor([0.0, 2.0, -3.0]); ho[2, 1, 2] = 1.5; ht[1, 0, 0] = 1.02
    mean, rep, n_o, n_t = (ref['repeat__' + k] for k in ('mean', 'rep', 'n_optical', 'n_thermal'))
    mine = []
    for p in range(B):
        kps = []
        for img in (opt, th):
            prob = oracle.forward(sd, img[p:p + 1], cfg)['prob']
            nmsp = oracle.box_nms(prob.numpy(), 4, 0.015, keep_top_k=120)
            kps.append(oracle.keypoints_from_map(nmsp[0, 0], 0.015))
        assert len(kps[0]) == n_o[p] and len(kps[1]) == n_t[p]
        c1, c2, nt, no = oracle.repeatability_pair(kps[0], kps[1], ho[p], ht[p], H, W, 3)
        mine.append((c1 + c2) / (nt + no))
    assert np.allclose(rep, mine, atol=1e-12) and 0.2 < mean < 1.0
    assert abs(float(mean) - float(np.mean(mine))) < 1e-12


@pytest.mark.parametrize('upd', [{'channel_version': 1}, {'channel_version': 2, 'descriptor_size': 128}])
def test_channel_versions_against_reference(oracle, ref, upd):
    name = 'cv%d' % upd['channel_version']
    cfg = dict(oracle.SHIPPED_MODEL_CONFIG); cfg.update(upd)
    spec = oracle.state_dict_spec(cfg)
    assert [k for k, _, _ in spec] == [k for k, _, _ in layout(ref, name)]
    sd = oracle.make_weights(51, cfg)
    img = oracle.make_images(52, 2, 32, 48)
    r = {k: torch.from_numpy(ref[name + '__' + k]) for k in ('prob', 'desc')}
    o = oracle.forward(sd, img, cfg)
    assert (r['prob'] - o['prob']).abs().max().item() <= 1e-7 and (r['desc'] - o['desc']).abs().max().item() <= 1e-7
    from multipoint_amd.models import MultiPoint
    assert [(k, tuple(s)) for k, s, _ in MultiPoint(dict(cfg)).state_dict_spec()] == [(k, tuple(s)) for k, s, _ in spec]


# ---- homographic adaptation (reference multipoint/utils/homographies.py) ---------------------------------------
def test_product_sample_homography_matches_reference(ref):
    """host logic of the product (no GPU): draw for draw the reference's sampler, on 12 seeds x 5 configurations x 2 shapes"""
    from multipoint_amd.utils.homographies import sample_homography, homography_adaptation_default_config
    cases = text(ref, 'sample_h__cases')
    assert cases[-1] == json.loads(json.dumps(dict(homography_adaptation_default_config['homographies'])))
    n = 0
    for seed in range(100, 112):
        for kw in cases:
            for shape in ((240, 320), (64, 64)):
                want, state = ref['sample_h__mats'][n], ref['sample_h__states'][n]
                np.random.seed(seed); got = sample_homography(np.array(shape), **kw)
                assert np.allclose(got, want, rtol=1e-9, atol=1e-11), (seed, kw)
                assert np.array_equal(np.random.get_state()[1][:4], state)       # same number of draws consumed
                n += 1
    assert n == len(ref['sample_h__mats'])


def test_oracle_homographic_adaptation_matches_reference_driver(oracle, ref):
    from oracle import ha_oracle as HA
    for c, (pair, agg, hc) in enumerate((
            (False, None, {'num': 3, 'erosion_radius': 2, 'mask_border': True, 'min_count': 2, 'filter_size': 0}),
            (False, None, {'num': 3, 'erosion_radius': 4, 'mask_border': False, 'min_count': 0, 'filter_size': 5}),
            (True, 'prod', {'num': 3, 'aggregation': 'prod', 'erosion_radius': 3, 'min_count': 3}),
            (True, 'sum', {'num': 2, 'aggregation': 'sum', 'erosion_radius': 0, 'filter_size': 3}))):
        cfg = {'multispectral': True, 'descriptor_size': 64} if pair else dict(oracle.SHIPPED_MODEL_CONFIG)
        sd = oracle.make_weights(17, cfg)
        img = oracle.make_images(41, 4 if pair else 2, 32, 40)
        want = torch.from_numpy(ref['ha%d__prob' % c])
        if pair:
            flags = [torch.ones(2, 1, dtype=torch.bool), torch.zeros(2, 1, dtype=torch.bool)]
            fwd = lambda i, x: oracle.forward(sd, x, cfg, is_optical=flags[i])['prob']
            streams = [img[:2], img[2:]]
        else:
            fwd = lambda i, x: oracle.forward(sd, x, cfg)['prob']
            streams = [img]
        homs = list(ref['ha%d__homs' % c])                       # the reference sampler's draws after np.random.seed(23)
        assert len(homs) == hc['num'] - 1
        got, _ = HA.homographic_adaptation(streams, fwd, hc, homs, aggregation=agg)
        assert (got - want).abs().max().item() <= 1e-6, hc


def test_detector_metrics_against_reference(oracle, ref):
    """The reference's compute_tp_fp_dist (evaluation.py:56-97, pure torch/numpy) and its compute_detector_metrics driver
    (:10-54, torchvision nms served by the oracle) against the oracle's restatement: pins the true-positive rule, n_gt, the
    distance list and the precision/recall bookkeeping."""
    from multipoint_amd.utils.evaluation import compute_mAP
    rng = np.random.default_rng(3)
    for case in range(6):
        H, W = 40, 56
        prob = np.zeros((H, W), np.float32)
        n = [60, 200, 5, 0, 400, 1][case]
        idx = rng.choice(H * W, n, replace=False)
        prob.flat[idx] = rng.permutation(n).astype(np.float32) / max(n, 1) * 0.9 + 0.01        # distinct scores
        km = np.zeros((H, W), bool)
        g = [40, 150, 0, 10, 300, 1][case]
        gi = np.concatenate([rng.choice(idx, min(g // 2, n), replace=False), rng.choice(H * W, g - min(g // 2, n), replace=False)]) if g else np.zeros(0, int)
        km.flat[gi.astype(int)] = True
        if case == 5:
            km[:] = False; km.flat[idx[0]] = True
        if n == 0:
            continue                                     # the reference's indexing fails on an empty prediction list
        r = [ref['tpfp%d__%s' % (case, k)] for k in ('tp', 'fp', 'prob', 'n_gt', 'dist')]
        o = oracle.compute_tp_fp_dist(prob, km)
        assert np.array_equal(r[0], o[0]) and np.array_equal(r[1], o[1]), case
        assert np.array_equal(r[2], o[2]) and r[3] == o[3]
        assert np.array_equal(np.asarray(r[4]), o[4]), case

    # the driver on two batches: its probability maps (the reference's forward, masked; values at or below the detection
    # threshold zeroed, which its box-NMS never reads) are stored with it -- the forward's parity is pinned above, and float32
    # forwards differ in the last bits between CPUs while this part compares exactly
    H, W = 64, 96
    mine = []
    for b in range(2):
        pr = ref['detmetrics__prob_map%d' % b]
        assert pr.shape == (2, 1, H, W) and not pr[:, :, :6].any()       # valid_mask: the top 6 rows masked
        pn = oracle.box_nms(pr, 4, 0.015)
        km = torch.zeros((2, H, W), dtype=torch.bool)
        for i in range(2):
            kept = np.argwhere(pn[i, 0] > 0.015)
            sel = kept[rng.choice(len(kept), len(kept) // 2, replace=False)]
            sel = np.clip(sel + rng.integers(-2, 3, sel.shape), 0, [H - 1, W - 1])       # jittered labels
            km[i, sel[:, 0], sel[:, 1]] = True
            mine.append(oracle.compute_tp_fp_dist(pn[i, 0], km[i].numpy()))
    precision, recall, prob, dist = (ref['detmetrics__' + k] for k in ('precision', 'recall', 'prob', 'dist'))
    tp = np.concatenate([m[0] for m in mine]); fp = np.concatenate([m[1] for m in mine])
    pp = np.concatenate([m[2] for m in mine]).astype(np.float64)
    p2, r2, prob2 = oracle.detector_precision_recall(tp, fp, pp, sum(m[3] for m in mine))
    assert 0 < tp.sum() < len(tp)
    assert np.array_equal(prob, prob2) and np.allclose(precision, p2, atol=0, rtol=0) and np.allclose(recall, r2, atol=0, rtol=0)
    assert np.array_equal(dist, np.concatenate([m[4] for m in mine]).astype(np.float64))
    assert abs(float(ref['detmetrics__map']) - compute_mAP(p2, r2)) == 0


def test_threshold_matcher_against_reference(oracle, ref):
    """ThresholdMatcher (matching.py:74-99) is in-repo numpy: the oracle restatement is pinned exactly."""
    from multipoint_amd.utils import ThresholdMatcher
    rng = np.random.default_rng(8)
    d1 = rng.standard_normal((120, 64)).astype(np.float32); d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    d2 = np.concatenate([d1[:60] + 0.05 * rng.standard_normal((60, 64)).astype(np.float32),
                         rng.standard_normal((50, 64)).astype(np.float32)]); d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
    for thr in (0.4, 0.7, 1.3):
        q, t, d = oracle.threshold_match(d1, d2, thr)
        assert list(ref['thr%g__query' % thr]) == list(q) and list(ref['thr%g__train' % thr]) == list(t) and len(q) > 0
        assert np.array_equal(ref['thr%g__distance' % thr], d)
    assert bool(ref['thr__negative_raises'])             # the reference refuses a negative threshold, and so does the product
    with pytest.raises(ValueError):
        ThresholdMatcher(-0.5)
