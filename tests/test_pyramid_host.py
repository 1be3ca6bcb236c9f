"""CPU: the restatement of the image pyramid and the staged mutual-information alignment (tests/pyramid_restatement.py), and the
host logic of multipoint_amd.utils.alignment on top of it: weights, level sizes, scale_transform, the stage sequence driven by
an aligner that fails on command, and the claim the GPU recovery test rests on."""
import numpy as np
import pytest

import mi_restatement as R
import pyramid_restatement as P
from photometric_restatement import gaussian_kernel


def test_weights():
    from multipoint_amd.utils import alignment as A
    for k in (1, 3, 5, 7):
        w = P.gaussian_weights(k)
        assert w.dtype == np.float32 and w.shape == (k,)
        s = np.float32(0)
        for v in w:                                  # dyadic fractions: every partial sum is exact in float32
            s = np.float32(s + v)
        assert s == np.float32(1.0) and float(np.sum(w.astype(np.float64))) == 1.0
        assert np.array_equal(w, w[::-1])
    for k in (9, 15, 31):
        assert np.array_equal(P.gaussian_weights(k).view(np.uint32), gaussian_kernel(k).view(np.uint32))
    # the library computes the same weights on the host (needs no device)
    for k in range(1, 32, 2):
        assert np.array_equal(A.gaussian_weights(k).view(np.uint32), P.gaussian_weights(k).view(np.uint32)), k
    for k in (0, 2, 8, 33, -1):
        with pytest.raises(ValueError):
            A.gaussian_weights(k)


LEVELS = {  # (H, W, filter_size) -> levels 1..3: (height, width, ksize)
    (96, 128, 5): [(48, 64, 3), (24, 32, 3), (12, 16, 1)],
    (97, 131, 5): [(49, 66, 3), (25, 33, 3), (13, 17, 1)],
    (96, 128, 9): [(48, 64, 5), (24, 32, 3), (12, 16, 3)],
    (97, 131, 9): [(49, 66, 5), (25, 33, 3), (13, 17, 3)],
}


@pytest.mark.parametrize('case', sorted(LEVELS))
def test_level_sizes(case):
    from multipoint_amd.utils import alignment as A
    H, W, fs = case
    for n in (1, 2, 3):
        assert A.pyramid_levels(H, W, fs, n) == LEVELS[case][:n]
        assert P.pyramid_levels(H, W, fs, n) == LEVELS[case][:n]
    # the sizes are those of [::2, ::2]
    x = np.zeros((H, W), np.float32)
    for h, w, k in LEVELS[case]:
        x = P.gaussian_blur(x, k, True)
        assert x.shape == (h, w)


def test_scale_transform():
    from multipoint_amd.utils import alignment as A
    rng = np.random.default_rng(0)
    for trial in range(20):
        T = np.eye(3) + rng.normal(0, 0.05, (3, 3))
        T[:2, 2] = rng.uniform(-20, 20, 2)
        T[2, :2] = rng.normal(0, 1e-4, 2)
        for full, level in (((96, 128), (48, 64)), ((96, 128), (24, 32)), ((97, 131), (49, 66)), ((97, 131), (25, 33))):
            keep = T.copy()
            d = A.scale_transform(T, level, full, True)
            assert np.array_equal(T, keep)                                  # a new array: the input is left alone
            assert np.array_equal(d, P.scale_transform(T, level, full, True))
            u = A.scale_transform(d, level, full, False)
            assert np.array_equal(u, P.scale_transform(d, level, full, False))
            assert np.all(np.abs(u - T) <= 1e-15 * np.abs(T))
            if full == (96, 128):
                r = level[0] / full[0]
                S = np.diag([r, r, 1.0])
                assert np.allclose(d, S @ T @ np.linalg.inv(S), rtol=1e-14, atol=0)
    # ratio_x comes from the ROW counts and scales the first row's last two entries, as the reference writes it
    d = A.scale_transform(np.ones((3, 3)), (1, 1), (2, 4), True)
    assert np.array_equal(d, [[1.0, 0.5 / 0.25, 0.5], [0.25 / 0.5, 1.0, 0.25], [2.0, 4.0, 1.0]])


# ---- the stage sequence, with an aligner that fails on command ----
class FakeAligner:
    """align(): pair b (told apart by the frames' first pixel) succeeds unless (stage kind, b) is in `fail`; a success adds
    1 to entry [0, 2] of the start at the size it is called at.  The calls are recorded."""

    def __init__(self, fail, full):
        self.fail, self.full, self.calls = set(fail), full, []

    def blur(self, frames, k, decimate):
        out = frames[:, ::2, ::2].copy() if decimate else frames.copy()
        out[:, 1, 1] += 100 + k                    # marks a blurred frame; pixel (0, 0) keeps the pair's number
        self.calls.append(('blur', k, bool(decimate), frames.shape))
        return out

    def __call__(self, optical, thermal, T, params, filter_images):
        assert optical.shape == thermal.shape and T.shape == (optical.shape[0], 3, 3)
        kind = 'smoothing' if filter_images else ('level%dx%d' % optical.shape[1:] if optical.shape[1:] != self.full else 'full')
        pairs = [int(v) for v in optical[:, 0, 0]]
        self.calls.append((kind, pairs, T.copy()))
        Ts, kinds, cands = [], [], []
        for j, b in enumerate(pairs):
            if (kind, b) in self.fail:
                Ts.append(None); kinds.append(None); cands.append([])
            else:
                new = T[j].copy()
                new[0, 2] += 1.0
                Ts.append(new); kinds.append('bin16_s0'); cands.append([{'type': 'bin16_s0', 'transform': new}])
        return Ts, kinds, cands


def _run(fail, params, B=3, full=(8, 12), t_init=None):
    from multipoint_amd.utils import alignment as A
    frames = np.zeros((B,) + full)
    frames[:, 0, 0] = np.arange(B)
    if t_init is None:
        t_init = np.stack([np.eye(3) + np.array([[0, 0, 10.0 * b], [0, 0, 2.0], [0, 0, 0]]) for b in range(B)])
    fake = FakeAligner(fail, full)
    p = dict({'alignment/filter_size': 5, 'alignment/n_pyramid_levels': 2}, **params)
    out = A.run_alignment_stages(frames, frames.copy(), t_init, p, fake, fake.blur)
    return out, fake, t_init


def _names(stages):
    return [s['name'] for s in stages]


def test_stages_all_succeed_and_lockstep():
    from multipoint_amd.utils import alignment as A
    out, fake, T0 = _run([], {'use_image_pyramid': True, 'use_smoothing_stage': True})
    # both frames are blurred and decimated twice (kernel 3, then 3), then the four batched calls
    assert [c[:3] for c in fake.calls if c[0] == 'blur'] == [('blur', 3, True)] * 4
    calls = [c for c in fake.calls if c[0] != 'blur']
    assert [c[0] for c in calls] == ['level2x3', 'level4x6', 'smoothing', 'full']
    assert all(c[1] == [0, 1, 2] for c in calls)                        # ONE call per stage, every pair in it
    for b, (ok, T, kind, cands, stages) in enumerate(out):
        assert ok and kind == 'bin16_s0' and cands[0]['type'] == 'bin16_s0'
        assert _names(stages) == ['pyramid2', 'pyramid1', 'smoothing', 'final']
        assert [s['shape'] for s in stages] == [(2, 3), (4, 6), (8, 12), (8, 12)]
        assert all(s['success'] and s['type'] == 'bin16_s0' for s in stages)
        # each pair got its own start: its t_init scaled down to the level
        assert np.array_equal(stages[0]['start'], A.scale_transform(T0[b], (2, 3), (8, 12), True))
        assert np.array_equal(calls[0][2][b], stages[0]['start'])
        assert stages[0]['start'][0, 2] == 0.25 * 10.0 * b
        # +1 at quarter size is +4 at full size, +1 at half size +2, then +1 and +1
        up = A.scale_transform(stages[0]['start'] + np.array([[0, 0, 1.0], [0, 0, 0], [0, 0, 0]]), (2, 3), (8, 12), False)
        assert np.array_equal(stages[1]['start'], A.scale_transform(up, (4, 6), (8, 12), True))
        assert T[0, 2] == 10.0 * b + 4 + 2 + 1 + 1 and T[1, 2] == 2.0


def test_a_failed_level_restarts_from_t_init():
    from multipoint_amd.utils import alignment as A
    out, fake, T0 = _run([('level2x3', 1)], {'use_image_pyramid': True})
    ok, T, kind, _, stages = out[1]
    assert _names(stages) == ['pyramid2', 'pyramid1', 'final']
    assert not stages[0]['success'] and stages[0]['type'] is None
    assert np.array_equal(stages[1]['start'], A.scale_transform(T0[1], (4, 6), (8, 12), True))     # from t_init again
    assert ok and T[0, 2] == 10.0 + 2 + 1
    assert out[0][1][0, 2] == 0.0 + 4 + 2 + 1 and out[2][1][0, 2] == 20.0 + 4 + 2 + 1               # the others are untouched
    # the LAST level fails: the final stage starts from t_init, and since it does there is no retry
    out, fake, T0 = _run([('level4x6', 2), ('full', 2)], {'use_image_pyramid': True})
    ok, T, kind, cands, stages = out[2]
    assert _names(stages) == ['pyramid2', 'pyramid1', 'final']
    assert np.array_equal(stages[2]['start'], T0[2]) and not ok and T is None and kind is None and cands == []
    assert [c[0] for c in fake.calls if c[0] != 'blur'] == ['level2x3', 'level4x6', 'full']


def test_a_failed_smoothing_stage_resets():
    out, fake, T0 = _run([('smoothing', 0)], {'use_image_pyramid': True, 'use_smoothing_stage': True})
    ok, T, _, _, stages = out[0]
    assert _names(stages) == ['pyramid2', 'pyramid1', 'smoothing', 'final']
    assert not stages[2]['success'] and np.array_equal(stages[3]['start'], T0[0]) and ok and T[0, 2] == 1.0
    assert np.array_equal(out[1][4][3]['start'], T0[1] + np.array([[0, 0, 7.0], [0, 0, 0], [0, 0, 0]]))
    # smoothing alone, blurred inside the aligner: no blur call of the stage sequence
    out, fake, T0 = _run([], {'use_smoothing_stage': True})
    assert [c[0] for c in fake.calls] == ['smoothing', 'full']
    assert _names(out[0][4]) == ['smoothing', 'final']
    # a failed pyramid followed by a smoothing stage that succeeds: the smoothing stage decides
    out, fake, T0 = _run([('level4x6', 1)], {'use_image_pyramid': True, 'use_smoothing_stage': True})
    assert np.array_equal(out[1][4][2]['start'], T0[1]) and out[1][1][0, 2] == 10.0 + 1 + 1


def test_the_final_retry():
    # pair 0 fails the final stage from a refined start: retried from t_init, alone; pair 1 fails it from t_init (its level
    # failed): no retry; pair 2 succeeds
    out, fake, T0 = _run([('full', 0), ('full', 1), ('level4x6', 1)], {'use_image_pyramid': True, 'alignment/n_pyramid_levels': 1})
    calls = [c for c in fake.calls if c[0] != 'blur']
    assert [(c[0], c[1]) for c in calls] == [('level4x6', [0, 1, 2]), ('full', [0, 1, 2]), ('full', [0])]
    assert np.array_equal(calls[2][2][0], T0[0])
    assert _names(out[0][4]) == ['pyramid1', 'final', 'retry'] and not out[0][0]          # (it fails there again)
    assert np.array_equal(out[0][4][2]['start'], T0[0])
    assert _names(out[1][4]) == ['pyramid1', 'final'] and not out[1][0]
    assert _names(out[2][4]) == ['pyramid1', 'final'] and out[2][0]
    # no stage before the final one: it starts from t_init, so a failure is final
    out, fake, T0 = _run([('full', 1)], {})
    assert [c[0] for c in fake.calls] == ['full'] and [o[0] for o in out] == [True, False, True]


def test_stages_are_the_restatements():
    """The module's lockstep sequence against the restated single-pair one, pair by pair, over every failure pattern of a
    two-level pyramid with a smoothing stage."""
    import itertools
    full = (8, 12)
    kinds = ['level2x3', 'level4x6', 'smoothing', 'full']
    params = {'use_image_pyramid': True, 'use_smoothing_stage': True, 'alignment/filter_size': 5, 'alignment/n_pyramid_levels': 2}
    for pattern in itertools.product([False, True], repeat=4):
        fail = [(k, 0) for k, f in zip(kinds, pattern) if f]
        out, fake, T0 = _run(fail, params, B=2)
        one = FakeAligner(fail, full)
        frame = np.zeros(full)

        def align(o, t, T, p, filter_images):
            Ts, ks, _ = one(o[None], t[None], np.asarray(T)[None], p, filter_images)
            return Ts[0], ks[0]
        ok, T, kind, stages = P.staged(frame, frame.copy(), T0[0], params, align=align)
        got = out[0]
        assert (got[0], got[2]) == (ok, kind) and (T is None) == (got[1] is None)
        assert T is None or np.array_equal(T, got[1])
        assert [(s['name'], s['success']) for s in got[4]] == [(s[0], s[4]) for s in stages]
        assert all(np.array_equal(a['start'], b[2]) for a, b in zip(got[4], stages))
        assert out[1][0] and _names(out[1][4]) == ['pyramid2', 'pyramid1', 'smoothing', 'final']


def test_settings():
    from multipoint_amd.utils import alignment as A
    frames = np.zeros((1, 8, 12))
    fake = FakeAligner([], (8, 12))
    with pytest.raises(NotImplementedError, match='warpAffine'):
        A.run_alignment_stages(frames, frames, np.eye(3)[None], {'perspective': False}, fake, fake.blur)
    with pytest.raises(NotImplementedError, match='warpAffine'):
        A.run_alignment_stages(frames, frames, np.eye(3)[None], {'alignment/decomposed_transformation': True}, fake, fake.blur)
    ignored = {'alignment/use_multiprocess': True, 'alignment/optimization_timeout': 1, 'show_results': True, 'verbose': True,
               'perspective': True}
    out = A.run_alignment_stages(frames, frames, np.eye(3)[None], ignored, fake, fake.blur)
    assert out[0][0] and _names(out[0][4]) == ['final']


def test_blur_restatement_properties():
    """the restated blur: weights of sum 1 leave a constant frame alone, k = 1 is the identity, an impulse spreads the outer
    product of the weights, and the border is BORDER_REFLECT_101"""
    c = np.full((9, 11), np.float32(0.375))
    for k in (1, 3, 5, 7):
        assert np.array_equal(P.gaussian_blur(c, k), c)
    rng = np.random.default_rng(1)
    x = rng.random((9, 11)).astype(np.float32)
    assert np.array_equal(P.gaussian_blur(x, 1), x)
    imp = np.zeros((9, 11), np.float32)
    imp[4, 5] = 1.0
    w = P.gaussian_weights(5)
    assert np.array_equal(P.gaussian_blur(imp, 5)[2:7, 3:8], np.outer(w, w).astype(np.float32))
    row = np.arange(7, dtype=np.float32)[None].repeat(3, 0)            # k = 3 at x = 0 reads x[1], x[0], x[1]
    assert P.gaussian_blur(row, 3)[1, 0] == np.float32(0.5) and P.gaussian_blur(row, 3)[1, 6] == np.float32(5.5)
    assert np.array_equal(P.gaussian_blur(x, 5, True), P.gaussian_blur(x, 5)[::2, ::2])


@pytest.mark.parametrize('seed', [11, 5])
def test_cpu_claim(seed):
    """What the GPU recovery test rests on: from a start 10.53 px off (four-corner error), the restated staged procedure (one
    pyramid level, filter_size 5, then the full-resolution stage) under scipy's Nelder-Mead ends below 0.5 px, the restated
    single-stage align_images above 2 px.  Measured with this float32 restatement: seed 11 0.137 / 3.642 px, seed 5
    0.097 / 3.988 px (with the blur summed in float64: 0.097 / 3.64 and 0.097 / 3.99)."""
    optimize = pytest.importorskip('scipy.optimize')
    o, t, T_true, T_init = P.displaced_pair(seed)
    H, W = t.shape
    e0 = R.corner_error(T_init, T_true, H, W)
    assert abs(e0 - 10.53) < 0.01
    ok, T, kind, stages = P.staged(o, t, T_init, P.PARAMS, optimize.minimize)
    T1, kind1 = P.align_images(o, t, T_init, dict(P.PARAMS, use_image_pyramid=False), False, optimize.minimize)
    e, e1 = R.corner_error(T, T_true, H, W), R.corner_error(T1, T_true, H, W)
    print('seed %d: initial %.3f px, staged %.4f px (%s), single stage %.4f px (%s)' % (seed, e0, e, kind, e1, kind1))
    assert ok and [s[0] for s in stages] == ['pyramid1', 'final']
    assert e < 0.5
    assert e1 > 2.0
