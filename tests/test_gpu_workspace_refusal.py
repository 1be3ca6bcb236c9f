"""GPU: every entry of the C ABI that takes (workspace, workspace_bytes) refuses a workspace one byte short of what its sizer
reports -- before any launch: the outputs, prefilled with a sentinel, keep it -- and runs in one of exactly that size.  Each
entry is called at the smallest shape it admits."""
import ctypes

import numpy as np
import pytest
import torch

from multipoint_amd import _lib

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENTINEL = 0x5A
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
MP_PHOTO_SHADE = 4


def dev(array):
    return torch.from_numpy(np.ascontiguousarray(array)).to(DEV)


def out(count, dtype):
    """an output tensor filled with the sentinel byte"""
    return torch.full((count * torch.empty((), dtype=dtype).element_size(),), SENTINEL, dtype=torch.uint8, device=DEV).view(dtype)


def ints(*values):
    return (ctypes.c_int * len(values))(*values)


def sized(lib, name, *args):
    n = _lib.c_ll()
    assert getattr(lib, name)(*args, ctypes.byref(n)) == _lib.MP_OK
    return n.value


class Case:
    """need: the sizer's bytes; call(ws_ptr, ws_bytes) -> status; outs: the output tensors of the call"""

    def __init__(self, need, call, outs):
        self.need, self.call, self.outs = need, call, outs


def frames8(seed):
    rng = np.random.default_rng(seed)
    return dev(rng.random((1, 8, 8), dtype=np.float32))


def ecc_case(h, s, entry):
    lib, p = h.lib, _lib.ptr
    packed, thermal, T = dev(np.zeros((1, 8, 8, 4), np.float32)), frames8(1), dev(np.array([IDENTITY]))
    one, sums = ints(0), out(66, torch.float64)
    keep = (packed, thermal, T, one)
    if entry == 'mp_ecc_sums':
        return Case(sized(lib, 'mp_ecc_workspace_bytes', 1, 8, 8), lambda w, n: lib.mp_ecc_sums(
            h.ptr, p(packed), 8, 8, p(thermal), 8, 8, 1, one, p(T), 1, 0, p(sums), w, n, s), [sums, keep])
    if entry == 'mp_ecc_begin':
        return Case(sized(lib, 'mp_ecc_workspace_bytes', 1, 8, 8), lambda w, n: lib.mp_ecc_begin(
            h.ptr, p(packed), 8, 8, p(thermal), 8, 8, 1, one, p(T), 1, 0, 1e-6, 5, 0.1, w, n, s), [keep])
    need = sized(lib, 'mp_ecc_pooled_workspace_bytes', 1, 1, 8, 8)           # one pair, one group
    if entry == 'mp_ecc_pooled_sums':
        return Case(need, lambda w, n: lib.mp_ecc_pooled_sums(
            h.ptr, p(packed), 8, 8, p(thermal), 8, 8, 1, one, 1, p(T), None, 0, None, 0, p(sums), w, n, s), [sums, keep])
    return Case(need, lambda w, n: lib.mp_ecc_pooled_begin(
        h.ptr, p(packed), 8, 8, p(thermal), 8, 8, 1, one, None, 1, p(T), None, 0, None, 0, 1e-6, 5, 0.1, w, n, s), [keep])


def mi_case(h, s, entry):
    lib, p = h.lib, _lib.ptr
    optical, thermal, T = frames8(2), frames8(3), dev(np.array([IDENTITY]))
    pair, bins = ints(0), ints(1)                                            # B = E = 1, bins = 1
    keep = (optical, thermal, T, pair, bins)
    if entry == 'mp_mi_joint_histogram':
        counts, minmax = out(2, torch.int32), out(2, torch.float32)
        return Case(sized(lib, 'mp_mi_workspace_bytes', 1, 1, 1, 8, 8, 1, 0), lambda w, n: lib.mp_mi_joint_histogram(
            h.ptr, p(optical), 8, 8, p(thermal), 8, 8, 1, pair, bins, p(T), 1, 0, p(counts), p(minmax), None, w, n, s),
            [counts, minmax, keep])
    if entry == 'mp_mi_objective':
        values = out(1, torch.float64)
        return Case(sized(lib, 'mp_mi_workspace_bytes', 1, 1, 1, 8, 8, 1, 0), lambda w, n: lib.mp_mi_objective(
            h.ptr, p(optical), 8, 8, p(thermal), 8, 8, 1, pair, bins, p(T), 1, 0.0, 0, None, p(values), w, n, s), [values, keep])
    problem = (_lib.MiProblem * 1)(_lib.MiProblem(0, 1, 5, 10, 1e-3, 1e-3))
    return Case(sized(lib, 'mp_mi_workspace_bytes', _lib.MP_MI_SLOTS, 1, 1, 8, 8, 1, 0), lambda w, n: lib.mp_mi_refine_begin(
        h.ptr, p(optical), 8, 8, p(thermal), 8, 8, 1, problem, p(T), 1, 0.0, 0, 0, w, n, s), [keep, problem])


def sift_case(h, s, entry):
    lib, p = h.lib, _lib.ptr
    u8 = dev(np.random.default_rng(4).integers(0, 256, (1, 16, 16), dtype=np.uint8))
    need = sized(lib, 'mp_sift_workspace_bytes', 1, 16, 16, 1)               # 16 x 16, capacity 1
    if entry == 'mp_sift_scale_space':
        return Case(need, lambda w, n: lib.mp_sift_scale_space(h.ptr, p(u8), 1, 16, 16, 1, w, n, s), [u8])
    kp, count, flags = out(6, torch.float32), out(1, torch.int32), out(1, torch.int32)
    if entry == 'mp_sift_detect':
        return Case(need, lambda w, n: lib.mp_sift_detect(h.ptr, p(u8), 1, 16, 16, 1, 1, w, n, p(kp), p(count), p(flags), 1, s),
                    [kp, count, flags, u8])
    none, desc = dev(np.zeros(1, np.int32)), out(128, torch.float32)         # no keypoint to describe: the pyramids are not read
    return Case(need, lambda w, n: lib.mp_sift_describe(h.ptr, 1, 16, 16, 1, w, n, p(kp), p(none), 1, p(desc), s), [desc, kp, none])


def fft_case(h, s, entry):
    lib, p = h.lib, _lib.ptr
    rng = np.random.default_rng(5)
    u8, bank = dev(rng.integers(0, 256, (1, 8, 8), dtype=np.uint8)), dev(rng.random((24, 8, 8), dtype=np.float32))
    if entry == 'mp_lghd_orientation':
        orientation = out(4 * 64, torch.uint8)
        return Case(sized(lib, 'mp_lghd_workspace_bytes', 1, 8, 8), lambda w, n: lib.mp_lghd_orientation(
            h.ptr, p(u8), p(bank), 1, 8, 8, p(orientation), w, n, s), [orientation, u8, bank])
    M, m, mim, T = out(64, torch.float32), out(64, torch.float32), out(64, torch.uint8), out(6, torch.float32)
    return Case(sized(lib, 'mp_rift_workspace_bytes', 1, 8, 8), lambda w, n: lib.mp_phase_congruency(
        h.ptr, p(u8), p(bank), 1, 8, 8, 2.0, 10.0, 0.5, p(M), p(m), p(mim), p(T), None, w, n, s), [M, m, mim, T, u8, bank])


def small_case(h, s, entry):
    lib, p = h.lib, _lib.ptr
    if entry == 'mp_register_peak':                                          # G = 1, 3 x 3
        planes, oi, of = dev(np.arange(9, dtype=np.float32)), out(2, torch.int32), out(6, torch.float32)
        return Case(sized(lib, 'mp_register_peak_workspace_bytes', 1, 3, 3), lambda w, n: lib.mp_register_peak(
            h.ptr, p(planes), 1, 3, 3, 1, p(oi), p(of), w, n, s), [oi, of, planes])
    if entry == 'mp_thermal_rescale':                                        # n = 1
        raw = dev(np.arange(64, dtype=np.int16).reshape(1, 8, 8))
        rescaled = out(64, torch.float32)
        return Case(sized(lib, 'mp_thermal_rescale_workspace_bytes', 1), lambda w, n: lib.mp_thermal_rescale(
            h.ptr, p(raw), 1, 8, 8, 1, None, p(rescaled), None, w, n, s), [rescaled, raw])
    if entry == 'mp_field_fit':                                              # B = 1, a 1 x 1 lattice
        d, weight = dev(np.array([0.5, -0.25])), dev(np.array([1.0]))
        u, info, res = out(2, torch.float64), out(16, torch.int32), out(1, torch.float64)
        return Case(sized(lib, 'mp_field_fit_workspace', 1, 1, 1), lambda w, n: lib.mp_field_fit(
            h.ptr, p(d), p(weight), 1, 1, 1, 1.0, 0.0, 0, 1e-9, 10, w, n, p(u), p(info), p(res), None, s), [u, info, res, d, weight])
    raise KeyError(entry)


def pooled_case(h, s, entry):
    lib, p = h.lib, _lib.ptr
    if entry == 'mp_pool_matches':
        # the sizer reports the larger of the pooling's and the search's need: 8 pairs are the fewest at which the pooling's decides
        P = 8
        kp, count, match = dev(np.zeros((2 * P, 1, 2), np.int32)), dev(np.zeros(2 * P, np.int32)), dev(np.full((P, 1), -1, np.int32))
        po, go = out(P + 1, torch.int32), out(2, torch.int32)
        need = sized(lib, 'mp_pooled_workspace_bytes', P, 1, 1)
        assert need == 4 * P
        return Case(need, lambda w, n: lib.mp_pool_matches(
            h.ptr, p(kp), p(count), p(match), None, P, 1, 1, None, None, 0, p(po), p(go), w, n, s), [po, go, kp, count, match])
    pts = dev(np.array([[0, 0, 1, 2], [8, 0, 9, 2], [0, 8, 1, 10], [8, 8, 9, 10]], np.float32))
    offsets = dev(np.array([0, 4], np.int32))
    T, mask, inl = out(9, torch.float64), out(4, torch.uint8), out(1, torch.int32)
    need = sized(lib, 'mp_pooled_workspace_bytes', 1, 1, 1)                  # P = G = 1, one hypothesis
    if entry == 'mp_find_homography_pooled':
        return Case(need, lambda w, n: lib.mp_find_homography_pooled(
            h.ptr, p(pts), p(offsets), 4, 1, 3.0, 1, 0, p(T), p(mask), p(inl), w, n, s), [T, inl, pts, offsets, mask])
    return Case(need, lambda w, n: lib.mp_find_transform_pooled(
        h.ptr, p(pts), p(offsets), 4, 1, 1, 3.0, 1, 0, p(T), p(mask), p(inl), w, n, s), [T, inl, pts, offsets, mask])


def loss_case(h, s, entry):
    lib, p = h.lib, _lib.ptr
    rng = np.random.default_rng(6)
    need = sized(lib, 'mp_loss_workspace_bytes', 1, 8, 8)                    # B = 1, 8 x 8: one cell
    logits, kp = dev(rng.random((1, 65, 1, 1), dtype=np.float32)), dev((rng.random((1, 8, 8)) > 0.9).astype(np.uint8))
    d1, d2 = dev(rng.random((1, 1, 1, 64), dtype=np.float32)), dev(rng.random((1, 1, 1, 64), dtype=np.float32))
    hom = dev(np.array([IDENTITY], np.float32))
    fwd, coef = dev(np.ones((1, 8))), dev(np.ones(8))
    keep = (logits, kp, d1, d2, hom, fwd, coef)
    if entry == 'mp_detector_loss':
        res = out(2, torch.float64)
        return Case(need, lambda w, n: lib.mp_detector_loss(
            h.ptr, p(logits), 1, 1, 1, p(kp), None, 8, 8, 1, None, 0, w, n, p(res), s), [res, keep])
    if entry == 'mp_descriptor_loss':
        res = out(8, torch.float64)
        return Case(need, lambda w, n: lib.mp_descriptor_loss(
            h.ptr, p(d1), p(d2), 1, 1, 1, 64, p(hom), p(hom), None, None, 8, 8, 8.0, 1.0, 0.2, 250.0, 0, w, n, p(res), None, s),
            [res, keep])
    if entry == 'mp_detector_loss_backward':
        grad = out(65, torch.float32)
        return Case(need, lambda w, n: lib.mp_detector_loss_backward(
            h.ptr, p(logits), 1, 1, 1, p(kp), None, 8, 8, 1, None, 0, p(fwd), p(coef), w, n, p(grad), s), [grad, keep])
    g1, g2 = out(64, torch.float32), out(64, torch.float32)
    return Case(need, lambda w, n: lib.mp_descriptor_loss_backward(
        h.ptr, p(d1), p(d2), 1, 1, 1, 64, p(hom), p(hom), None, None, 8, 8, 8.0, 1.0, 0.2, 250.0, 0, p(fwd), p(coef), w, n,
        p(g1), p(g2), s), [g1, g2, keep])


def augment_case(h, s, entry):
    lib, p = h.lib, _lib.ptr
    if entry.startswith('mp_photometric'):                                   # n = 1 at the smallest frame, 1 x 1
        need = sized(lib, 'mp_photometric_workspace_bytes', 1, 1, 1, 0)
        plans = (_lib.PhotometricPlan * 1)()
        src, res = dev(np.array([0.5], np.float32)), out(1, torch.float32)
        if entry == 'mp_photometric_augment':                                # no operation: a copy
            return Case(need, lambda w, n: lib.mp_photometric_augment(
                h.ptr, p(src), p(res), 1, 1, 1, plans, None, 0, None, 0, None, 0, w, n, s), [res, src, plans])
        plans[0].n_ops = 1                                                   # a shade without ellipses, unblurred
        plans[0].op[0].kind, plans[0].op[0].ksize = MP_PHOTO_SHADE, 1
        return Case(need, lambda w, n: lib.mp_photometric_shade_mask(
            h.ptr, 1, 1, 1, plans, None, 0, 0, 0, p(res), w, n, s), [res, plans])
    need = sized(lib, 'mp_shapes_workspace_bytes', 1, 1, 1, 0, 0, 0)         # n = 1 at 1 x 1, no command
    canvas = dev(np.array([0.25], np.float32))
    if entry == 'mp_shapes_render':
        cmds, offsets, mean = (_lib.ShapesCmd * 1)(), ints(0, 0), out(1, torch.float64)
        return Case(need, lambda w, n: lib.mp_shapes_render(
            h.ptr, p(canvas), p(mean), 1, 1, 1, cmds, ctypes.cast(offsets, ctypes.c_void_p), None, 0, None, None, 0, None, 0, w, n, s),
            [mean, canvas, cmds, offsets])
    blur, res = ints(0), out(1, torch.float32)
    return Case(need, lambda w, n: lib.mp_shapes_finish(
        h.ptr, p(canvas), 1, 1, 1, ctypes.cast(blur, ctypes.c_void_p), ctypes.cast(blur, ctypes.c_void_p), p(res), 1, 1, w, n, s),
        [res, canvas, blur])


ENTRIES = {
    'mp_ecc_sums': ecc_case, 'mp_ecc_begin': ecc_case, 'mp_ecc_pooled_sums': ecc_case, 'mp_ecc_pooled_begin': ecc_case,
    'mp_mi_joint_histogram': mi_case, 'mp_mi_objective': mi_case, 'mp_mi_refine_begin': mi_case,
    'mp_sift_scale_space': sift_case, 'mp_sift_detect': sift_case, 'mp_sift_describe': sift_case,
    'mp_lghd_orientation': fft_case, 'mp_phase_congruency': fft_case,
    'mp_register_peak': small_case, 'mp_thermal_rescale': small_case, 'mp_field_fit': small_case,
    'mp_pool_matches': pooled_case, 'mp_find_homography_pooled': pooled_case, 'mp_find_transform_pooled': pooled_case,
    'mp_detector_loss': loss_case, 'mp_descriptor_loss': loss_case, 'mp_detector_loss_backward': loss_case,
    'mp_descriptor_loss_backward': loss_case,
    'mp_photometric_augment': augment_case, 'mp_photometric_shade_mask': augment_case,
    'mp_shapes_render': augment_case, 'mp_shapes_finish': augment_case,
}


def test_every_entry_with_a_workspace_is_listed():
    """the public header's entries with a `workspace_bytes` argument; the two that only forward to a listed twin are not repeated"""
    import os
    import re
    header = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'multipoint_hip.h')
    with open(header) as f:
        declared = set(re.findall(r'^int (mp_\w+)\([^;]*\bworkspace_bytes\b[^;]*\);', f.read(), re.M))
    assert declared - {'mp_pool_matches_f', 'mp_mi_refine_begin_model'} == set(ENTRIES)


@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_short_workspace_is_refused_before_any_launch(entry):
    h = _lib.get_handle(torch.device(DEV))
    with torch.cuda.device(DEV):
        s = _lib.stream_ptr(torch.device(DEV))
        case = ENTRIES[entry](h, s, entry)
        assert case.need > 0
        ws = torch.zeros(case.need, dtype=torch.uint8, device=DEV)
        outs = [t for t in case.outs if isinstance(t, torch.Tensor)]
        before = [t.clone() for t in outs]
        with pytest.raises(ValueError, match='workspace'):
            h.check(case.call(_lib.ptr(ws), case.need - 1))
        torch.cuda.synchronize()
        for t, b in zip(outs, before):
            assert torch.equal(t.view(torch.uint8), b.view(torch.uint8))
        assert not ws.any()                                                  # ... and nothing was written into the workspace
        h.check(case.call(_lib.ptr(ws), case.need))
        torch.cuda.synchronize()
