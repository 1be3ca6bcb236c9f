"""CPU: the premises of tests/test_gpu_lghd_shapes.py, without a device.  The Stockham pass of csrc/mp_fft.h, compiled by g++
into tests/fft_host_harness.cpp's emulation of fft_lines_kernel, against np.fft in float64 at all 131 line lengths (this is
where the GPU sweep's bound comes from) and on hand cases with exact answers; the FFT plan against the library's and the Python
wrapper's length rule; what the frames of tests/lghd_shape_cases.py are chosen for; and the condition the orientation tolerance
rests on, on the reference side alone."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import lghd_restatement as R
import lghd_shape_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {'separate': ['-ffp-contract=off'], 'contracted': ['-mfma', '-ffp-contract=fast']}
LENGTHS = S.supported_lengths()


@pytest.fixture(scope='module')
def harness(tmp_path_factory):
    """{build: library}: tests/fft_host_harness.cpp with separate multiplies and adds, and with the multiply-adds contracted as
    the device contracts them (fft.hip carries no contraction pragma)"""
    if 'fma' not in open('/proc/cpuinfo').read().split():
        pytest.fail('this CPU has no FMA instructions: the contracted build of the harness cannot run')
    out = {}
    for name, flags in BUILDS.items():
        so = str(tmp_path_factory.mktemp('fft_' + name) / 'fft_host_harness.so')
        r = subprocess.run(['g++', '-std=c++17', '-O2', '-Wall', '-Wextra', '-Werror', '-shared', '-fPIC'] + flags +
                           ['-I' + os.path.join(ROOT, 'multipoint_amd', 'csrc'), os.path.join(ROOT, 'tests', 'fft_host_harness.cpp'),
                            '-o', so], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        dll = ctypes.CDLL(so)
        dll.fft_host_plan.restype = ctypes.c_int
        dll.fft_host_plan.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        dll.fft_host_lines.restype = ctypes.c_int
        dll.fft_host_lines.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 4
        out[name] = dll
    return out


def _lines(dll, x, inverse, nthr=S.HOST_THREADS):
    """the transform of the bundle x, complex64 [n][C] with C in {1, 2, 4, 8, 16}, along its first axis"""
    n, C = x.shape
    x = np.ascontiguousarray(x, np.complex64)
    out = np.empty_like(x)
    rc = dll.fft_host_lines(x.ctypes.data, out.ctypes.data, n, C.bit_length() - 1, int(inverse), nthr)
    assert rc == 0 and 1 << (C.bit_length() - 1) == C
    return out


def _plan(dll, n):
    npass, radix = ctypes.c_int(-1), (ctypes.c_int * 12)()
    ok = dll.fft_host_plan(n, ctypes.byref(npass), radix)
    return bool(ok), list(radix[:npass.value])


# ---- a. the pass ----

@pytest.fixture(scope='module')
def host_ratios(harness):
    """{(build, n, cshift, inverse): error / error of np.fft in float32}"""
    out = {}
    for n in LENGTHS:
        for cshift in S.HOST_CSHIFTS:
            x = S.complex_noise(n, (n, 1 << cshift))
            for inverse in (False, True):
                for build, dll in harness.items():
                    err, err32 = S.fft_errors(_lines(dll, x, inverse), x, (0,), inverse)
                    assert err32 > 0
                    out[build, n, cshift, inverse] = err / err32
    return out


def test_the_sweep_bound_is_twice_the_host_emulations_worst_ratio(host_ratios):
    """All 131 lengths, forward and inverse, bundles of 1 and 4 lines, 256 emulated threads, both builds.  Measured: the worst
    ratio is 7.02 without contraction (median 3.67) and 6.00 with it (median 3.47)."""
    assert len(host_ratios) == 131 * 2 * 2 * 2
    for build in BUILDS:
        r = {k[1:]: v for k, v in host_ratios.items() if k[0] == build}
        worst = max(r, key=r.get)
        print('%s: worst ratio %.2f at n = %d cshift %d inverse %d, median %.2f' % ((build, r[worst]) + worst + (np.median(list(r.values())),)))
    worst_host = max(host_ratios.values())
    assert S.FFT_SWEEP_BOUND == max(8, math.ceil(2 * worst_host))


@pytest.mark.parametrize('build', list(BUILDS))
def test_thread_count_and_bundle_width_do_not_change_a_line(harness, build):
    """a line's arithmetic does not depend on which thread runs it or on its neighbours in the bundle: 256, 512 and 7 threads and
    bundles of 1 to 16 lines give the same bits"""
    dll = harness[build]
    for n in (8, 45, 120, 625, 1024):
        x = S.complex_noise(n, (n, 16))
        for inverse in (False, True):
            want = _lines(dll, x, inverse)
            for nthr in (512, 7):
                assert np.array_equal(_lines(dll, x, inverse, nthr).view(np.uint32), want.view(np.uint32))
            for C in (1, 2, 4, 8):
                assert np.array_equal(_lines(dll, x[:, 3:3 + C], inverse).view(np.uint32), want[:, 3:3 + C].view(np.uint32))


@pytest.mark.parametrize('build', list(BUILDS))
@pytest.mark.parametrize('n', S.HAND_LENGTHS)
def test_hand_cases(harness, build, n):
    """A delta at 0 gives ones and a constant of small integers gives n at bin 0 and zeros, both exactly: every product is a
    product with 0 or of equal operands.  A delta at p and an exponential at bins 1 and n - 1 are exact up to the rounding of the
    table and of the input: tol = 2^-24 (1 + 4 ceil(log2 n)) relative to the largest output, one rounding of the operand and at
    most four per pass (there are at most log2 n passes)."""
    dll = harness[build]
    tol = 2.0 ** -24 * (1 + 4 * math.ceil(math.log2(n)))
    k = np.arange(n)
    for inverse in (False, True):
        sg = 1 if inverse else -1
        delta = np.zeros((n, 1), np.complex64)
        delta[0] = 1
        assert np.array_equal(_lines(dll, delta, inverse), np.ones((n, 1), np.complex64))
        const = np.full((n, 1), 3 - 2j, np.complex64)
        want = np.zeros((n, 1), np.complex64)
        want[0] = n * (3 - 2j)
        got = _lines(dll, const, inverse)
        assert got[0, 0] == want[0, 0] and np.abs(got - want).max() <= tol * n * abs(3 - 2j)
        if n in (8, 9):                     # radices 4, 2 and 3: the differences of equal values are exact zeros
            assert np.array_equal(got, want)
        for p in (1, n // 2, n - 1):
            delta = np.zeros((n, 1), np.complex64)
            delta[p] = 1
            want = np.exp(sg * 2j * np.pi * k * p / n)[:, None]
            assert np.abs(_lines(dll, delta, inverse) - want).max() <= tol
        for b in (1, n - 1):
            x = np.exp(2j * np.pi * k * b / n)[:, None]
            want = np.zeros((n, 1), np.complex128)
            want[(-b if inverse else b) % n] = n
            assert np.abs(_lines(dll, x.astype(np.complex64), inverse) - want).max() <= tol * n


# ---- b. the plan ----

def test_the_three_length_rules_agree(harness):
    import __graft_entry__ as g
    g.build()
    from multipoint_amd import _lib
    from multipoint_amd.models.classic_detectors import fft_length_ok
    lib = _lib.load_library()
    dll = harness['separate']
    lengths = set(LENGTHS)
    assert len(LENGTHS) == 131 and LENGTHS[0] == 8 and LENGTHS[-1] == 4096
    for n in range(1, 4201):
        ok, radix = _plan(dll, n)
        assert ok == bool(lib.mp_fft_supported(n)) == fft_length_ok(n) == (n in lengths), n
        if ok:
            assert int(np.prod(radix)) == n and 1 <= len(radix) <= 12
            assert radix == sorted(radix, key=[4, 2, 3, 5].index), (n, radix)          # 4s, then 2s, then 3s, then 5s
            assert radix.count(2) <= 1                                                 # 4 first: fewest passes
    for n in (0, -8, 4097, 8192):
        assert not _plan(dll, n)[0] and not lib.mp_fft_supported(n) and not fft_length_ok(n)


def _ns(radix):
    return [int(np.prod(radix[:i])) for i in range(len(radix))]


def test_what_the_lengths_reach(harness):
    """the premises of the issue's gap: of the seven lengths of tests/test_gpu_lghd.py only 120 has a pass whose Ns is no power of
    two; in 9 ... 2187 every pass after the first has one"""
    dll = harness['separate']

    def odd_ns(n):
        return [s for s in _ns(_plan(dll, n)[1]) if s & (s - 1)]
    assert [n for n in (48, 64, 80, 96, 120, 512, 640) if odd_ns(n)] == [120] and odd_ns(120) == [24]
    for n in (9, 15, 25, 27, 45, 75, 125, 243, 625, 675, 2187):
        assert len(odd_ns(n)) == len(_plan(dll, n)[1]) - 1, n
    assert sum(1 for n in LENGTHS if odd_ns(n)) >= 100


def test_what_the_frames_reach():
    """launch_lines' bundle widths and thread counts, and the ARGMAX slots, of the frames and of the sweep's column lengths"""
    assert [S.column_bundle(n) for n in (8, 256, 512, 640, 1024, 2048, 4096)] == \
        [(16, 256), (16, 256), (16, 512), (8, 512), (8, 512), (4, 512), (2, 512)]
    frames = {(H, W): name for name, _, _, H, W in S.FRAMES}
    assert len(S.FRAMES) == 14 and len(frames) == 11 == len(S.FRAME_SIZES)
    assert all(H in LENGTHS and W in LENGTHS for H, W in frames)
    slots = {hw: -(-hw[1] // 256) for hw in frames}
    assert slots[16, 320] == 2 and slots[8, 4096] == 16 and slots[512, 640] == 3
    assert [s for hw, s in slots.items() if hw not in ((16, 320), (8, 4096), (512, 640))] == [1] * 8
    assert 2 * 8 * 4096 == 64 * 1024                                      # the 4096 row: the largest bundle with 256 threads
    assert S.column_bundle(512) == (16, 512) and 24 % 16 == 8
    assert S.column_bundle(640)[0] == 8 and S.column_bundle(2048)[0] == 4 and S.column_bundle(4096)[0] == 2 and 9 % 2 == 1
    assert S.COLUMN_WIDTHS == (19, 3) and all(19 % c for c in (16, 8, 4, 2)) and 2 < 3 < 4          # partial bundles everywhere
    assert [S.column_bundle(n)[0] for n in S.NARROW_LENGTHS] == [16, 16, 8, 2]
    H, W = S.BATCH_FRAME
    assert len(S.BATCH_IMAGES) == 9 and S.image_bytes(H, W) == 25 * 48 * 80 * 8
    lists = S.describe_lists()
    inside = [[S.patch_inside(y, x) for y, x in rows] for rows in lists.tolist()]
    assert [sum(r) for r in inside] == [8, 11, 7]


# ---- c. the orientation tolerance's condition ----

@pytest.mark.parametrize('name', S.FRAME_NAMES)
def test_few_pixels_are_ambiguous_in_float64(name):
    """tests/test_lghd_host.py::test_few_pixels_are_ambiguous_in_float64 on the frames of tests/lghd_shape_cases.py: at most 1 %
    of a scale's pixels have their two largest float64 magnitudes within 16 err32 of each other."""
    u8, bank, m64, err32, want = S.reference(name)
    assert u8.shape == bank.shape[1:] == m64.shape[1:] == want.shape[1:] and want.max() <= 5
    assert 0 < err32 <= 2e-6 * m64.max()
    share = (R.top_two_gap(m64) < 16 * err32).reshape(4, -1).mean(1)
    print(name, 'err32 / max = %.3g' % (err32 / m64.max()), 'share below 16 err32 per scale:', share)
    assert np.all(share <= 0.01)
