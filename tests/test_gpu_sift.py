"""GPU: the SIFT kernels (multipoint_amd/csrc/sift.hip) stage by stage against the float64 restatement (tests/sift_restatement.py,
DESIGN.md 3.19), at every frame of tests/sift_cases.py and B in {1, 3}.  Each later stage is checked on the GPU's OWN pyramids,
read back, so that a stage answers for its own arithmetic only."""
import functools

import numpy as np
import pytest
import torch

import sift_cases as C
import sift_restatement as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CASES = [(H, W, B) for (H, W) in C.FRAMES for B in (1, 3)]


def _u8(H, W, B):
    return np.stack([C.quantise(C.case_image(H, W, b)) for b in range(B)])


@functools.lru_cache(maxsize=None)
def gpu_run(H, W, B):
    """one detect + describe of the case's batch; every stage's result as numpy arrays"""
    from multipoint_amd.models import classic_detectors as S
    u8 = torch.from_numpy(_u8(H, W, B)).to(DEV)
    kp, count, flags, ws = S.sift_detect(u8, capacity=4096)
    desc = S.sift_describe(ws, kp, count)
    torch.cuda.synchronize()
    gauss, dog = ws.pyramids()
    cand, ncand = ws.candidates()
    rec, nori, info = ws.refined()
    lst, nlist = ws.oriented()
    cpu = lambda t: t.cpu().numpy().copy()
    return dict(u8=cpu(u8), gauss=[cpu(g) for g in gauss], dog=[cpu(d) for d in dog], cand=cpu(cand), ncand=cpu(ncand), rec=cpu(rec),
                nori=cpu(nori), info=cpu(info), list=cpu(lst), nlist=cpu(nlist), kp=cpu(kp), count=cpu(count), flags=cpu(flags),
                desc=cpu(desc), ws=ws)


@pytest.mark.parametrize('H, W, B', CASES)
def test_scale_space(H, W, B):
    """A blur pass computes acc = fma(w[k], x[k], acc) over n taps in fp32 (u = 2^-24): the computed sum differs from the exact one
    by at most gamma_n sum |w x| with gamma_n = n u / (1 - n u) <= (n + 1) u for n <= 27, and one more u covers the second-order
    terms and the weights' own representation being shared with the model (they are the same fp32 numbers): (n + 2) u sum |w x|
    per pass.  Weights and pixels are non-negative, so sum |w x| is the pass's own result.  The input's error eps passes through
    the filter as sum w eps (unit-sum, non-negative weights), so along the chain: bound_out = blur(bound_in) + the two passes'
    terms; the half-size copy picks its pixels' bounds; a difference layer adds its two layers' bounds and u |difference| for its
    own rounding.  The up-scale is exact (weights 1/4, 3/4 on 8-bit values).  R.scale_space(with_bound=True) evaluates this."""
    run = gpu_run(H, W, B)
    assert len(run['gauss']) == R.n_octaves(H, W)
    worst = 0.0
    for b in range(B):
        gauss, dog, gb, db = R.scale_space(run['u8'][b], np.float64, with_bound=True)
        for o in range(len(gauss)):
            for got, want, bound in ((run['gauss'][o][b], gauss[o], gb[o]), (run['dog'][o][b], dog[o], db[o])):
                assert got.shape == want.shape
                err = np.abs(got.astype(np.float64) - want)
                tiny = 1e-300
                worst = max(worst, float((err / (bound + tiny)).max()))
                assert np.all(err <= bound), 'octave %d: error %g over its bound' % (o, float((err - bound).max()))
    print('scale space %dx%d B=%d: largest error / bound = %.3f' % (H, W, B, worst))


@pytest.mark.parametrize('H, W, B', CASES)
def test_candidates(H, W, B):
    run = gpu_run(H, W, B)
    assert not run['flags'].any()
    for b in range(B):
        want = R.candidates([d[b] for d in run['dog']])
        n = int(run['ncand'][b])
        assert n == len(want)
        assert [tuple(int(v) for v in row) for row in run['cand'][b, :n]] == want          # equal, in order
    if (H, W) == (16, 16):
        # the smallest frame: the count equals the restatement's on its own pyramids (see sift_cases.FRAMES for why it is not 0)
        assert run['count'].tolist() == [len(R.select(R.detect_records([g[b] for g in run['gauss']], [d[b] for d in run['dog']])))
                                         for b in range(B)]


def _bins(info_row):
    mask = (int(info_row[2]) & 0x3ffff) | ((int(info_row[3]) & 0x3ffff) << 18)
    return [j for j in range(36) if mask >> j & 1]


@pytest.mark.parametrize('H, W, B', CASES)
def test_refinement_and_orientation(H, W, B):
    """Every candidate whose float64 decision margins lie above the exclusion thresholds agrees in fate, integer position, layer and
    emitted bins; x, y, size, angle and response agree within 4 x the restatement's float32-mode error (sift_cases.noise_floor)."""
    run = gpu_run(H, W, B)
    tol, eps = C.noise_floor()
    total = left_out = 0
    worst = dict.fromkeys(tol, 0.0)
    for b in range(B):
        gauss, dog = [g[b] for g in run['gauss']], [d[b] for d in run['dog']]
        for i in range(int(run['ncand'][b])):
            cand = tuple(int(v) for v in run['cand'][b, i])
            want = R.detect_candidate(gauss, dog, cand)
            total += 1
            n, rec, info = int(run['nori'][b, i]), run['rec'][b, i].astype(np.float64), run['info'][b, i]
            if C.excluded(want, eps):
                left_out += 1
                continue
            bins = want.get('bins', [])
            assert n == len(bins) and (_bins(info) == bins or not bins), 'candidate %s: %s' % (cand, want['fate'])
            if want['fate'] != 'kept' or not bins:
                continue
            assert (int(info[0]), int(info[1]), int(rec[4])) == (want['r'], want['c'], want['o'] * 8 + want['layer'])
            err = {'x': abs(rec[0] - want['x']), 'y': abs(rec[1] - want['y']), 'size': abs(rec[2] - want['size']) / want['size'],
                   'response': abs(rec[3] - want['response']) / want['response']}
            worst = {k: max(worst[k], err.get(k, 0.0)) for k in worst}
            for name, e in err.items():
                assert e <= tol[name], 'candidate %s: %s off by %g (tolerance %g)' % (cand, name, e, tol[name])
        # the angles, and the second compaction: the list holds every candidate's records in candidate order, then bin order
        pos = 0
        for i in range(int(run['ncand'][b])):
            n = int(run['nori'][b, i])
            want = R.detect_candidate(gauss, dog, tuple(int(v) for v in run['cand'][b, i]))
            for e in range(n):
                row = run['list'][b, pos]
                assert np.array_equal(row[[0, 1, 2, 4, 5]], run['rec'][b, i])
                if not C.excluded(want, eps) and want['fate'] == 'kept':
                    d = C._circ(row[3], want['records'][e][3])
                    worst['angle'] = max(worst['angle'], d)
                    assert d <= tol['angle'], 'candidate %d bin %d: angle off by %g (tolerance %g)' % (i, e, d, tol['angle'])
                pos += 1
        assert pos == int(run['nlist'][b])
    print('refinement %dx%d B=%d: %d of %d candidates excluded; observed / tolerance: %s' % (
        H, W, B, left_out, total, ', '.join('%s %.3g / %.3g' % (k, worst[k], tol[k]) for k in tol)))
    assert left_out <= 0.05 * total


def _variants(kps, target=300):
    """the detector's records plus rotated / rescaled copies, so that the share of differing entries is a statistic"""
    out = [kp.copy() for kp in kps]
    turns = [(37.0, 1.0), (111.0, 1.3), (222.0, 0.8), (301.0, 1.15), (15.0, 0.9), (180.0, 1.0), (77.0, 1.25)]
    for da, fs in turns[:max(0, target // max(len(kps), 1) - 1)]:
        for kp in kps:
            v = kp.copy()
            v[3] = np.float32((v[3] + da) % 360.0)
            v[2] = np.float32(v[2] * fs)
            out.append(v)
    return np.array(out, dtype=np.float32).reshape(-1, 6)


@pytest.mark.parametrize('H, W, B', CASES)
def test_descriptors(H, W, B):
    """from given keypoint records: entries agree within +-1 (the final rounding); the share that differs at all is bounded by 4 x the
    share the restatement's float32 mode shows against float64 on the same records"""
    from multipoint_amd.models import classic_detectors as S
    run = gpu_run(H, W, B)
    lists = [_variants(run['kp'][b, :int(run['count'][b])]) for b in range(B)]
    N = max(max(len(l) for l in lists), 1)
    kp = np.zeros((B, N, 6), np.float32)
    for b, l in enumerate(lists):
        kp[b, :len(l)] = l
    count = torch.tensor([len(l) for l in lists], dtype=torch.int32)
    got = S.sift_describe(run['ws'], torch.from_numpy(kp).to(DEV), count.to(DEV)).cpu().numpy()
    differ = differ32 = entries = 0
    for b, l in enumerate(lists):
        gauss = [g[b] for g in run['gauss']]
        assert not got[b, len(l):].any()                      # rows beyond the count are zero
        for k, rec in enumerate(l):
            want = R.describe(gauss, rec)
            d = np.abs(got[b, k] - want)
            assert d.max() <= 1, 'image %d keypoint %d: an entry differs by %g' % (b, k, d.max())
            differ += int((d > 0).sum())
            differ32 += int((R.describe(gauss, rec, np.float32) != want).sum())
            entries += 128
    print('descriptors %dx%d B=%d: %d entries, %d differ on the GPU (share %.2e), %d in float32 mode (share %.2e)' % (
        H, W, B, entries, differ, differ / max(entries, 1), differ32, differ32 / max(entries, 1)))
    assert differ <= 4 * differ32


def test_selection():
    """a crafted list: equal responses across the cut, planted duplicates, two images of different lengths"""
    from multipoint_amd.models import classic_detectors as S
    rng = np.random.default_rng(5)
    M = 3000
    rec = np.zeros((2, M, 6), np.float32)
    counts = [M, 1700]
    for b in range(2):
        rec[b, :, 0] = rng.uniform(10, 200, M).astype(np.float32)
        rec[b, :, 1] = rng.uniform(10, 200, M).astype(np.float32)
        rec[b, :, 2] = rng.uniform(2, 20, M).astype(np.float32)
        rec[b, :, 3] = rng.uniform(0, 360, M).astype(np.float32)
        rec[b, :, 4] = (rng.integers(14, 60, M) / 1000.0).astype(np.float32)          # 46 distinct responses: ties everywhere
        rec[b, :, 5] = rng.integers(0, 4, M) * 8 + rng.integers(1, 4, M)
        for src, dst in ((3, 40), (3, 2999 if b == 0 else 1650), (500, 501), (1200, 777)):          # duplicates, also of later by earlier
            lo, hi = min(src, dst), max(src, dst)
            rec[b, hi, :4] = rec[b, lo, :4]
            rec[b, hi, 4] = 0.9                                    # a duplicate goes whatever its response
    for nfeat in (1000, 64, 5000):
        kp, count = S.sift_select(torch.from_numpy(rec).to(DEV), torch.tensor(counts, dtype=torch.int32), nfeatures=nfeat)
        kp, count = kp.cpu().numpy(), count.cpu().numpy()
        for b in range(2):
            want = R.select(rec[b, :counts[b]], nfeat)
            assert int(count[b]) == len(want)
            assert np.array_equal(kp[b, :len(want)].astype(np.float64), want)          # the kept set, its order, the halved values
            assert not kp[b, len(want):].any()


def test_capacity_overflow():
    """more candidates than slots: the flag is set and the head of the list is kept"""
    from multipoint_amd.models import classic_detectors as S
    H, W = 96, 120
    u8 = torch.from_numpy(_u8(H, W, 1)).to(DEV)
    full = gpu_run(H, W, 1)
    cap = 16
    assert int(full['ncand'][0]) > cap
    kp, count, flags, ws = S.sift_detect(u8, capacity=cap, nfeatures=cap)
    cand, ncand = ws.candidates()
    rec, nlist = ws.oriented()
    assert int(flags[0]) & 1 and int(ncand[0]) == int(full['ncand'][0])
    assert np.array_equal(cand[0].cpu().numpy(), full['cand'][0, :cap])
    head = int(full['nori'][0, :cap].sum())                         # records of the first `cap` candidates
    assert int(nlist[0]) == head and bool(int(flags[0]) & 2) == (head > cap)
    assert np.array_equal(rec[0, :min(head, cap)].cpu().numpy(), full['list'][0, :min(head, cap)])
    want = R.select(full['list'][0, :min(head, cap)].astype(np.float64), cap)
    assert int(count[0]) == len(want) and np.array_equal(kp[0, :len(want)].cpu().numpy().astype(np.float64), want)


def test_owner_map():
    """three keypoints rounding to one pixel: the last in list order owns it; describe returns its row; the B == 1 dense map holds
    the raw row"""
    from multipoint_amd.models import ClassicDetectors, classic_detectors as S
    H, W = 24, 32
    kp = np.zeros((1, 8, 6), np.float32)
    kp[0, :5, :2] = [(10.4, 7.3), (20.0, 12.0), (9.6, 6.6), (10.5, 7.5), (3.2, 19.9)]          # (x, y); 10.5 and 7.5 round to even
    count = torch.tensor([5], dtype=torch.int32, device=DEV)
    prob, owner = S.sift_scatter(torch.from_numpy(kp).to(DEV), count, H, W)
    want_prob, want_owner = R.scatter(kp[0, :5], H, W)
    assert np.array_equal(prob[0, 0].cpu().numpy(), want_prob) and np.array_equal(owner[0].cpu().numpy(), want_owner)
    assert want_owner[7, 10] == 2 and want_owner[8, 10] == 3 and want_prob.sum() == 4          # 0 and 2 share (7, 10); 3 rounds to (8, 10)
    kp[0, 3, :2] = (10.2, 6.9)                                       # now 0, 2 and 3 share the pixel
    prob, owner = S.sift_scatter(torch.from_numpy(kp).to(DEV), count, H, W)
    assert int(owner[0, 7, 10]) == 3 and float(prob.sum()) == 3.0
    desc = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (1, 8, 128)).astype(np.float32)).to(DEV)
    out = {'sift_desc': desc, 'sift_owner': owner}
    net = ClassicDetectors({'method': 'SIFT', 'implementation': 'restated'})
    yx = torch.tensor([[[7, 10], [12, 20], [0, 0], [19, 3]]], dtype=torch.int32, device=DEV)
    rows = net.describe(out, yx, torch.tensor([3], dtype=torch.int32, device=DEV)).cpu().numpy()
    d = desc.cpu().numpy()[0].astype(np.float64)
    assert np.allclose(rows[0, 0], d[3] / np.linalg.norm(d[3]), rtol=1e-6, atol=0)
    assert np.allclose(rows[0, 1], d[1] / np.linalg.norm(d[1]), rtol=1e-6, atol=0)
    assert not rows[0, 2].any() and not rows[0, 3].any()            # a pixel without an owner; a row beyond the count
    dense = S.sift_dense_map(desc, owner).cpu().numpy()
    assert dense.shape == (1, 128, H, W)
    assert np.array_equal(dense[0, :, 7, 10], d[3]) and np.array_equal(dense[0, :, 20, 3], d[4]) and not dense[0, :, 0, 0].any()
    assert (dense != 0).any(axis=1).sum() <= 3
    empty = S.sift_dense_map(desc, torch.full_like(owner, -1))
    assert empty.shape == (1, 1, H, W) and not empty.any()


def test_forward_outputs_and_run_to_run():
    """two runs of the full forward are bit-identical (B = 3, 96 x 120); the outputs have the documented shapes"""
    from multipoint_amd.models import ClassicDetectors
    H, W, B = 96, 120, 3
    images = torch.from_numpy(np.stack([C.case_image(H, W, b) for b in range(B)])[:, None]).to(DEV)
    net = ClassicDetectors({'method': 'SIFT', 'implementation': 'restated'}).to(DEV).eval()
    a, b = net({'image': images}), net({'image': images})
    assert set(a) == {'prob', 'sift_keypoints', 'sift_count', 'sift_desc', 'sift_owner', 'sift_flags'}
    assert a['prob'].shape == (B, 1, H, W) and a['sift_keypoints'].shape == (B, 1000, 6) and a['sift_desc'].shape == (B, 1000, 128)
    assert a['sift_owner'].shape == (B, H, W) and a['sift_owner'].dtype == torch.int32 and a['sift_count'].shape == (B,)
    for key in a:
        assert torch.equal(a[key], b[key]), key
    run = gpu_run(H, W, B)
    assert np.array_equal(a['sift_keypoints'][:, :run['kp'].shape[1]].cpu().numpy(), run['kp'][:, :1000])
    assert int(a['sift_count'].min()) > 20 and not a['sift_flags'].any()
    one = net({'image': images[:1]})
    assert one['desc'].shape == (1, 128, H, W) and torch.equal(one['sift_keypoints'][0], a['sift_keypoints'][0])
    flat = net({'image': torch.full((1, 1, 16, 16), 0.3, device=DEV)})          # nothing to find: empty lists, the [1,1,H,W] zero map
    assert int(flat['sift_count'][0]) == 0 and flat['desc'].shape == (1, 1, 16, 16) and not flat['prob'].any()


def test_invalid_arguments():
    from multipoint_amd.models import classic_detectors as S
    for shape in ((1, 15, 64), (1, 64, 15), (1, 4097, 16)):
        with pytest.raises(ValueError):
            S.sift_detect(torch.zeros(shape, dtype=torch.uint8, device=DEV))
    ws = S.SiftWorkspace(1, 32, 32, 64, DEV)
    small = S.SiftWorkspace(1, 16, 16, 64, DEV)
    small.B, small.H, small.W = 1, 32, 32                                   # a workspace that is too small for the frame
    with pytest.raises(ValueError, match='workspace'):
        S.sift_scale_space(torch.zeros((1, 32, 32), dtype=torch.uint8, device=DEV), workspace=small)
    with pytest.raises(ValueError):
        S.sift_detect(torch.zeros((1, 32, 32), dtype=torch.uint8, device=DEV), workspace=ws, nfeatures=100, N=50)
