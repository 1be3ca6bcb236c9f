"""GPU (MI355X): the warp, adaptation and descriptor-sampling kernels (homog_adapt.hip: warp_kernel in its four variants,
accumulate_kernel in its three aggregations, begin_kernel, finalize_kernel, gaussian_filter_kernel, valid_mask_kernel;
sample_desc.hip: sample_desc_kernel) on every case of tests/sampling_cases.py against the float64 restatement of
tests/sampling_restatement.py under its own derived bounds; tests/test_sampling_host.py holds the premises.

  continuous outputs   |got - want| <= bound everywhere
  nearest samples      exact off the near-tie pixels, one of the candidates on them
  masks, counts, zero rows, begin and finalize (single IEEE operations)   equal

Every kernel runs twice -- once behind its public entry point, once over the C ABI into a buffer with a guard of 64 sentinel
elements behind it, pre-filled with the sentinel: the two results hold the same bytes, every element was written, and the guard
is untouched.  `pytest -s` prints the largest error relative to the bound per case."""
import numpy as np
import pytest
import torch

import sampling_cases as C
import sampling_restatement as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64
SENTINEL = {torch.float32: -777.25, torch.uint8: 0xA5}


def _api():
    from multipoint_amd import _lib
    dev = torch.device(DEV)
    return _lib, _lib.get_handle(dev), _lib.stream_ptr(dev)


class Guarded:
    """an output of `shape` with GUARD sentinel elements behind it; `init` (numpy) or the sentinel fills the output itself"""

    def __init__(self, shape, dtype=torch.float32, init=None):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + GUARD,), SENTINEL[dtype], dtype=dtype, device=DEV)
        self.out = self.buf[:self.n].view(*shape)
        if init is not None:
            self.out.copy_(torch.from_numpy(np.ascontiguousarray(init)))

    def result(self):
        torch.cuda.synchronize()
        guard = self.buf[self.n:].cpu()
        assert torch.equal(guard, torch.full_like(guard, SENTINEL[self.buf.dtype])), 'the guard behind the output was written'
        return self.out.cpu().numpy()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def _same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _ratio(err, bound):
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(np.max(r, initial=0.0))


# ---- warp_kernel<MODE, PAD> ----
WARP_CASES = C.warp_cases()
MODES, PADS = {'bilinear': 0, 'nearest': 1}, {'zeros': 0, 'reflection': 1}


@pytest.mark.parametrize('case', WARP_CASES, ids=lambda c: c['name'])
def test_warp(case):
    from multipoint_amd.utils import homographies as PH
    lib, h, stream = _api()
    n_src, H, W = case['src'].shape
    n_out, (Ho, Wo) = len(case['hom']), case['dsize']
    src = _dev(case['src'])[:, None]
    hom = PH._hom_tensor(case['hom'], torch.device(DEV))
    for mode, pad in C.WARP_VARIANTS:
        if pad not in case['paddings']:
            continue
        if case['route'] == 'tensor':
            got = PH.warp_perspective_tensor(src, torch.from_numpy(case['M']), (Ho, Wo), mode, pad)
        else:
            got = PH._warp(src, case['hom'], n_out, (Ho, Wo), mode, pad)
        assert got.shape == (n_out, 1, Ho, Wo) and got.dtype == torch.float32 and got.is_cuda
        got = got[:, 0].cpu().numpy()
        g = Guarded((n_out, Ho, Wo))
        h.check(h.lib.mp_warp_perspective(h.ptr, lib.ptr(src), n_src, H, W, lib.ptr(hom), n_out, Ho, Wo, MODES[mode], PADS[pad],
                                          lib.ptr(g.out), stream))
        assert _same_bytes(got, g.result()), (case['name'], mode, pad)
        r = R.warp(case['src'], case['hom'], (Ho, Wo), mode, pad)
        assert np.isfinite(got).all()
        err = np.abs(got - r['want'])
        if mode == 'bilinear':
            print('warp %-26s %-8s %-10s max err / bound %.3f  (max err %.3g)' % (case['name'], mode, pad, _ratio(err, r['bound']), err.max()))
            assert (err <= r['bound']).all(), (case['name'], mode, pad, _ratio(err, r['bound']))
        else:
            off = ~r['tie']
            print('warp %-26s %-8s %-10s differing off ties %d, near-tie pixels %d' % (case['name'], mode, pad, int((err[off] != 0).sum()),
                                                                                     int(r['tie'].sum())))
            assert np.array_equal(got[off], r['want'][off]), (case['name'], mode, pad, int((err[off] != 0).sum()))
            assert (got[None] == r['alts'])[:, r['tie']].any(axis=0).all(), (case['name'], mode, pad)


def test_warp_refusals():
    from multipoint_amd.utils import homographies as PH
    src = torch.zeros(3, 1, 5, 65, device=DEV)
    with pytest.raises(ValueError):
        PH._warp(src, np.stack([np.eye(3)] * 2), 7, (5, 65), 'bilinear', 'zeros')         # one matrix per output map
    with pytest.raises(ValueError):
        PH._warp(src, np.stack([np.eye(3)] * 3), 3, (5, 65), 'bilinear', 'border')


# ---- accumulate_kernel<AGG> ----
ACC_CASES = C.accumulate_cases()


@pytest.mark.parametrize('case', ACC_CASES, ids=lambda c: c['name'])
def test_accumulate(case):
    from multipoint_amd.utils import homographies as PH
    lib, h, stream = _api()
    G, B, H, W, agg = case['G'], case['B'], case['H'], case['W'], case['agg']
    pa, pb, mask = _dev(case['pa']), _dev(case['pb']), _dev(case['mask'])
    hom = PH._hom_tensor(case['hom'], torch.device(DEV))
    runs = []
    for _ in range(2):
        prob, count = Guarded((B, H, W), init=case['prob0']), Guarded((B, H, W), init=case['count0'])
        h.check(h.lib.mp_ha_accumulate(h.ptr, lib.ptr(pa), lib.ptr(pb) if agg else None, lib.ptr(mask), lib.ptr(hom), G, B, H, W, agg,
                                       lib.ptr(prob.out), lib.ptr(count.out), stream))
        runs.append((prob.result(), count.result()))
    assert _same_bytes(runs[0][0], runs[1][0]) and _same_bytes(runs[0][1], runs[1][1])
    prob, count = runs[0]
    r = R.accumulate(case['pa'], case['pb'], case['mask'], case['hom'], B, agg, case['prob0'], case['count0'])
    off = ~r['tie']
    err = np.abs(prob - r['prob'])
    print('accumulate %-22s max err / bound %.3f  (max err %.3g), near-tie pixels %d' % (case['name'], _ratio(err[off], r['bound'][off]),
                                                                                       err[off].max(initial=0), int(r['tie'].sum())))
    assert np.array_equal(count[off], r['count'][off]), case['name']
    assert ((r['count_lo'] <= count) & (count <= r['count_hi'])).all() and np.array_equal(count, np.rint(count))
    assert np.isfinite(prob).all() and (err[off] <= r['bound'][off]).all(), (case['name'], _ratio(err[off], r['bound'][off]))


# ---- begin_kernel, finalize_kernel ----
@pytest.mark.parametrize('shape', C.POINTWISE_SHAPES, ids=lambda s: 'n%d' % int(np.prod(s)))
def test_begin_and_finalize(shape):
    lib, h, stream = _api()
    B, H, W = shape
    for agg in C.AGGREGATIONS:
        c = C.pointwise_case(shape, agg)
        pa, pb = _dev(c['pa']), _dev(c['pb'])
        runs = []
        for _ in range(2):
            prob, count = Guarded(shape), Guarded(shape)
            h.check(h.lib.mp_ha_begin(h.ptr, lib.ptr(pa), lib.ptr(pb) if agg else None, B, H, W, agg, lib.ptr(prob.out),
                                      lib.ptr(count.out), stream))
            runs.append((prob.result(), count.result()))
        want_prob, want_count = R.begin(c['pa'], c['pb'], agg)
        assert _same_bytes(runs[0][0], runs[1][0]) and _same_bytes(runs[0][0], want_prob), (shape, agg)
        assert _same_bytes(runs[0][1], want_count) and _same_bytes(runs[1][1], want_count)
        p, n = _dev(c['prob']), _dev(c['count'])
        for mc in C.MIN_COUNTS:
            outs = []
            for _ in range(2):
                out = Guarded(shape)
                h.check(h.lib.mp_ha_finalize(h.ptr, lib.ptr(p), lib.ptr(n), B, H, W, agg, mc, lib.ptr(out.out), stream))
                outs.append(out.result())
            want = R.finalize(c['prob'], c['count'], agg, mc)
            assert np.array_equal(outs[0], outs[1], equal_nan=True)
            assert np.array_equal(outs[0], want, equal_nan=True), (shape, agg, mc, int((outs[0] != want).sum()))


def test_adaptation_refusals():
    lib, h, stream = _api()
    a = torch.zeros(2, 5, 65, device=DEV)
    out, out2 = torch.zeros_like(a), torch.zeros_like(a)
    mask = torch.ones(1, 5, 65, dtype=torch.uint8, device=DEV)
    hom = torch.eye(3, dtype=torch.float64, device=DEV).reshape(1, 9)
    p = lib.ptr
    for agg, pb in ((3, p(a)), (-1, p(a)), (1, None), (2, None)):
        with pytest.raises(ValueError):
            h.check(h.lib.mp_ha_begin(h.ptr, p(a), pb, 2, 5, 65, agg, p(out), p(out2), stream))
        with pytest.raises(ValueError):
            h.check(h.lib.mp_ha_accumulate(h.ptr, p(a), pb, p(mask), p(hom), 1, 2, 5, 65, agg, p(out), p(out2), stream))
    for agg in (3, -1):
        with pytest.raises(ValueError):
            h.check(h.lib.mp_ha_finalize(h.ptr, p(a), p(a), 2, 5, 65, agg, 1.0, p(out), stream))
    torch.cuda.synchronize()
    assert not out.any() and not out2.any()


# ---- gaussian_filter_kernel ----
@pytest.mark.parametrize('k', C.FILTER_SIZES)
def test_gaussian_filter(k):
    from multipoint_amd.utils import homographies as PH
    lib, h, stream = _api()
    for kind in C.FILTER_WEIGHTS:
        w = C.filter_weights(kind, k)
        wd = _dev(w)
        for H, W in C.filter_frames(k):
            x = C.filter_input(k, H, W)
            xd = _dev(x)[:, None]
            got = PH.gaussian_filter(xd, k, None if kind == 'gaussian' else wd)
            assert got.shape == xd.shape and got.is_cuda
            got = got[:, 0].cpu().numpy()
            g = Guarded(x.shape)
            h.check(h.lib.mp_gaussian_filter(h.ptr, lib.ptr(xd), x.shape[0], H, W, k, lib.ptr(wd), lib.ptr(g.out), stream))
            assert _same_bytes(got, g.result()), (k, kind, H, W)
            want, bound = R.gaussian_filter(x, w)
            err = np.abs(got - want)
            print('filter k=%-2d %-8s %2dx%-3d max err / bound %.3f  (max err %.3g)' % (k, kind, H, W, _ratio(err, bound), err.max()))
            assert (err <= bound).all(), (k, kind, H, W, _ratio(err, bound))
            if kind == 'one_hot':
                assert np.array_equal(got.astype(np.float64), want)         # a reflected shift: copies


def test_gaussian_filter_refusals():
    lib, h, stream = _api()
    x = torch.rand(1, 70, 70, device=DEV)             # as large as the largest shape claimed below
    out = torch.zeros_like(x)
    w = torch.zeros(33 * 33, device=DEV)
    p = lib.ptr
    for H, W, k in ((4, 70, 9), (4, 70, 11), (70, 4, 9), (40, 40, 33), (40, 40, 4), (40, 40, 0)):      # r >= H, r >= W, k = 33, even k
        with pytest.raises(ValueError):
            h.check(h.lib.mp_gaussian_filter(h.ptr, p(x), 1, H, W, k, p(w), p(out), stream))
    with pytest.raises(ValueError):
        h.check(h.lib.mp_gaussian_filter(h.ptr, p(x), 1, 4, 70, 3, p(w), p(x), stream))                  # in place
    torch.cuda.synchronize()
    assert not out.any()


# ---- valid_mask_kernel ----
@pytest.mark.parametrize('H,W', C.MASK_FRAMES)
def test_valid_mask(H, W):
    from multipoint_amd.utils import homographies as PH
    lib, h, stream = _api()
    dev = torch.device(DEV)
    homs = C.mask_homographies(H, W)
    hd = PH._hom_tensor(homs, dev)
    for r in C.MASK_RADII:
        for border in (False, True):
            want = R.valid_mask(homs, H, W, r, border)
            got = PH._valid_masks(homs, (H, W), r, border, dev)
            assert got.shape == (C.MASK_G, H, W) and got.dtype == torch.uint8
            got = got.cpu().numpy()
            g = Guarded((C.MASK_G, H, W), torch.uint8)
            h.check(h.lib.mp_ha_valid_mask(h.ptr, lib.ptr(hd), C.MASK_G, H, W, r, int(border), lib.ptr(g.out), stream))
            assert _same_bytes(got, g.result())
            assert np.array_equal(got, want), (r, border, int((got != want).sum()))
            for i in range(C.MASK_G):       # one launch of G homographies == G launches of one
                assert np.array_equal(PH._valid_masks(homs[i:i + 1], (H, W), r, border, dev)[0].cpu().numpy(), want[i]), (r, border, i)
            fwd = np.linalg.inv(homs[0])
            one = PH.compute_valid_mask((H, W), fwd, r, border)
            assert one.dtype == np.float64 and np.array_equal(one, R.valid_mask(np.linalg.inv(fwd), H, W, r, border)[0])


# ---- sample_desc_kernel ----
DESC_CASES = C.desc_cases()


@pytest.mark.parametrize('case', DESC_CASES, ids=lambda c: c['name'])
def test_sample_descriptors(case):
    from multipoint_amd.utils.utils import interpolate_descriptors_batched
    lib, h, stream = _api()
    B, Hc, Wc, D = case['desc'].shape
    K = case['kp'].shape[1]
    desc, kp, cnt = _dev(case['desc']), _dev(case['kp']), _dev(case['count'])
    got = interpolate_descriptors_batched(kp, cnt, desc.permute(0, 3, 1, 2), case['H'], case['W'])
    assert got.shape == (B, K, D) and got.dtype == torch.float32
    got = got.cpu().numpy()
    g = Guarded((B, K, D))
    h.check(h.lib.mp_sample_descriptors(h.ptr, lib.ptr(desc), B, Hc, Wc, D, case['H'], case['W'], lib.ptr(kp), lib.ptr(cnt), K,
                                        lib.ptr(g.out), stream))
    assert _same_bytes(got, g.result()), case['name']
    r = R.sample_descriptors(case['desc'], case['H'], case['W'], case['kp'], case['count'])
    low = np.zeros((B, K), bool)
    for b, k in case['low_norm_rows']:
        low[b, k] = True
    assert np.isfinite(got).all()
    assert not got[~r['valid']].any()                                     # rows beyond the count: written, and zero
    assert (np.linalg.norm(got.astype(np.float64), axis=-1) <= 1 + (R.C2 + D) * R.U).all()
    err = np.abs(got - r['want'])
    print('descriptors %-24s max err / bound %.3f  (max err %.3g), low-norm rows %d' % (case['name'], _ratio(err[~low], r['bound'][~low]),
                                                                                      err[~low].max(initial=0), int(low.sum())))
    assert (err[~low] <= r['bound'][~low]).all(), (case['name'], _ratio(err[~low], r['bound'][~low]))
    for b, k in case['zero_rows']:
        assert not got[b, k].any()


def test_sample_descriptors_refusals():
    lib, h, stream = _api()
    kp = torch.zeros(1, 4, 2, dtype=torch.int32, device=DEV)
    cnt = torch.full((1,), 4, dtype=torch.int32, device=DEV)
    out = torch.zeros(1, 4, 448, device=DEV)
    for D in (96, 448, 0):
        desc = torch.rand(1, 3, 4, max(D, 1), device=DEV)
        with pytest.raises(ValueError):
            h.check(h.lib.mp_sample_descriptors(h.ptr, lib.ptr(desc), 1, 3, 4, D, 24, 32, lib.ptr(kp), lib.ptr(cnt), 4, lib.ptr(out), stream))
    torch.cuda.synchronize()
    assert not out.any()
