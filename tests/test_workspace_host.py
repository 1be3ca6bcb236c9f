"""CPU: the sizes every workspace sizer of the C ABI reports, against the values recorded from the library before the
carving moved into one helper (tests/golden/workspace_sizes.json), and the limits each sizer refuses one step outside.  No
device is touched: the sizers only compute."""
import ctypes
import json
import os

import pytest

from multipoint_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'workspace_sizes.json')
MP_EINVAL = -1
SIFT_LAYOUT_SLOTS = 8 + 4 * 16          # octaves, seven list offsets, four values per octave (16 octaves at most)

# per entry: the smallest admitted shape, a pixel count that is no multiple of 64, a large shape (4096 per side or the
# entry's own maximum), and the extra parameters at both ends
CASES = {
    # P, G, max_iters
    'mp_pooled_workspace_bytes': [(0, 1, 1), (1, 1, 1), (3, 5, 7), (1000003, 65535, 1 << 20), (1 << 30, 1, 1)],
    # B, H, W
    'mp_loss_workspace_bytes': [(1, 8, 8), (3, 24, 40), (2, 4096, 4096), (65535, 8, 8)],
    # n, H, W, n_ellipses
    'mp_photometric_workspace_bytes': [(1, 1, 1, 0), (3, 7, 9, 5), (1, 4096, 4096, 100), (65535, 8, 8, 0),
                                       (1, 1 << 17, 1 << 17, 0)],
    # n, H, W, n_cmds, n_verts, n_circles
    'mp_shapes_workspace_bytes': [(1, 1, 1, 0, 0, 0), (3, 7, 9, 5, 11, 2), (1, 4096, 4096, 100, 1000, 50),
                                  (65535, 8, 8, 0, 0, 0), (4, 32768, 32768, 0, 0, 0)],
    # n_evals, n_pairs, n_thermal_maps, H, W, max_bins, smoothing
    'mp_mi_workspace_bytes': [(1, 1, 1, 1, 1, 1, 0), (1, 1, 1, 8, 8, 1, 0), (1, 1, 1, 8, 8, 1, 1), (10, 1, 1, 7, 9, 256, 0),
                              (10, 1, 1, 7, 9, 256, 1), (30, 3, 6, 120, 160, 64, 1), (10, 1, 1, 4096, 4096, 256, 1),
                              (65535, 65535, 65535, 1, 1, 1, 0), (1, 1, 1, 32767, 32767, 256, 1)],
    # n
    'mp_thermal_rescale_workspace_bytes': [(1,), (3,), (65535,)],
    # B, H, W
    'mp_lghd_workspace_bytes': [(1, 8, 8), (3, 9, 15), (4, 8, 8), (5, 8, 8), (1, 4096, 4096), (65535, 4096, 4096)],
    'mp_rift_workspace_bytes': [(1, 8, 8), (3, 9, 15), (4, 8, 8), (5, 8, 8), (1, 4096, 4096), (65535, 4096, 4096)],
    # B, H, W, capacity
    'mp_sift_workspace_bytes': [(1, 16, 16, 1), (1, 16, 16, 4096), (3, 17, 19, 1), (3, 17, 19, 4096), (1, 4096, 4096, 1),
                                (2, 4096, 4096, 4096), (65535, 16, 16, 1), (1, 16, 16, 1 << 24)],
    'mp_sift_layout': [(1, 16, 16, 1), (1, 16, 16, 4096), (3, 17, 19, 1), (3, 17, 19, 4096), (1, 4096, 4096, 1),
                       (2, 4096, 4096, 4096), (65535, 16, 16, 1), (1, 16, 16, 1 << 24)],
    # G, hh, ww
    'mp_register_peak_workspace_bytes': [(1, 3, 3), (3, 7, 9), (2, 129, 127), (1, 4096, 4096), (65535, 4096, 4096)],
    # n_problems, H, W
    'mp_ecc_workspace_bytes': [(1, 8, 8), (3, 9, 15), (1, 4096, 4096), (4096, 4096, 4096)],
    # n_pairs, n_groups, H, W
    'mp_ecc_pooled_workspace_bytes': [(1, 1, 8, 8), (5, 1, 9, 15), (5, 5, 9, 15), (65535, 1, 4096, 4096),
                                      (4096, 4096, 4096, 4096)],
    # B, gy, gx
    'mp_field_fit_workspace': [(1, 1, 1), (3, 7, 9), (1, 256, 256), (65535, 256, 256)],
}

# one step outside each limit
REFUSED = {
    'mp_pooled_workspace_bytes': [(-1, 1, 1), (0, 0, 1), (0, 65536, 1), (0, 1, 0), (0, 1, (1 << 20) + 1)],
    'mp_loss_workspace_bytes': [(0, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 0), (1, 7, 8), (1, 8, 9)],
    'mp_photometric_workspace_bytes': [(0, 1, 1, 0), (65536, 1, 1, 0), (1, 0, 1, 0), (1, 1, 0, 0), (1, 1, 1, -1),
                                       (1, 1 << 17, (1 << 17) + 1, 0)],
    'mp_shapes_workspace_bytes': [(0, 1, 1, 0, 0, 0), (65536, 1, 1, 0, 0, 0), (1, 0, 1, 0, 0, 0), (1, 1, 0, 0, 0, 0),
                                  (1, 32769, 1, 0, 0, 0), (1, 1, 32769, 0, 0, 0), (5, 32768, 32768, 0, 0, 0),
                                  (1, 1, 1, -1, 0, 0), (1, 1, 1, 0, -1, 0), (1, 1, 1, 0, 0, -1)],
    'mp_mi_workspace_bytes': [(0, 1, 1, 8, 8, 1, 0), (65536, 1, 1, 8, 8, 1, 0), (1, 0, 1, 8, 8, 1, 0), (1, 65536, 1, 8, 8, 1, 0),
                              (1, 1, 0, 8, 8, 1, 0), (1, 1, 1, 0, 8, 1, 0), (1, 1, 1, 8, 0, 1, 0), (1, 1, 1, 32768, 8, 1, 0),
                              (1, 1, 1, 8, 32768, 1, 0), (1, 1, 1, 8, 8, 0, 0), (1, 1, 1, 8, 8, 257, 0)],
    'mp_thermal_rescale_workspace_bytes': [(0,), (65536,)],
    # 6 and 4320 are 5-smooth lengths below and above the FFT's range, 14 has a factor 7
    'mp_lghd_workspace_bytes': [(0, 8, 8), (65536, 8, 8), (1, 6, 8), (1, 8, 6), (1, 7, 8), (1, 8, 7), (1, 14, 8), (1, 4097, 8),
                                (1, 8, 4097), (1, 4320, 8), (1, 8, 4320)],
    'mp_rift_workspace_bytes': [(0, 8, 8), (65536, 8, 8), (1, 6, 8), (1, 8, 6), (1, 7, 8), (1, 8, 7), (1, 14, 8), (1, 4097, 8),
                                (1, 8, 4097), (1, 4320, 8), (1, 8, 4320)],
    'mp_sift_workspace_bytes': [(0, 16, 16, 1), (65536, 16, 16, 1), (1, 15, 16, 1), (1, 16, 15, 1), (1, 4097, 16, 1),
                                (1, 16, 4097, 1), (1, 16, 16, 0), (1, 16, 16, (1 << 24) + 1)],
    'mp_sift_layout': [(0, 16, 16, 1), (65536, 16, 16, 1), (1, 15, 16, 1), (1, 16, 15, 1), (1, 4097, 16, 1), (1, 16, 4097, 1),
                       (1, 16, 16, 0), (1, 16, 16, (1 << 24) + 1)],
    'mp_register_peak_workspace_bytes': [(0, 3, 3), (65536, 3, 3), (1, 2, 3), (1, 3, 2), (1, 4097, 3), (1, 3, 4097)],
    'mp_ecc_workspace_bytes': [(0, 8, 8), (4097, 8, 8), (1, 7, 8), (1, 8, 7), (1, 4097, 8), (1, 8, 4097)],
    'mp_ecc_pooled_workspace_bytes': [(0, 1, 8, 8), (65536, 1, 8, 8), (1, 0, 8, 8), (1, 4097, 8, 8), (1, 1, 7, 8), (1, 1, 8, 7),
                                      (1, 1, 4097, 8), (1, 1, 8, 4097)],
    'mp_field_fit_workspace': [(0, 1, 1), (65536, 1, 1), (1, 0, 1), (1, 1, 0), (1, 257, 1), (1, 1, 257)],
}


def key(name, args):
    return '%s(%s)' % (name, ', '.join(str(a) for a in args))


def call(lib, name, args):
    """(status, value): the sizer's long long, or mp_sift_layout's filled slots as a list"""
    if name == 'mp_sift_layout':
        out = (_lib.c_ll * SIFT_LAYOUT_SLOTS)(*([-1] * SIFT_LAYOUT_SLOTS))
        rc = getattr(lib, name)(*args, out)
        if rc != _lib.MP_OK:
            return rc, [v for v in out if v != -1]                   # empty: a refused call writes nothing
        return rc, list(out[:8 + 4 * out[0]])
    out = _lib.c_ll(-1)
    rc = getattr(lib, name)(*args, ctypes.byref(out))
    return rc, out.value


def measure(lib):
    return {key(name, args): call(lib, name, args)[1] for name, cases in CASES.items() for args in cases}


def test_every_sizer_is_listed():
    sizers = {n for n in _lib.SIGNATURES if n.endswith('_workspace_bytes') or n in ('mp_field_fit_workspace', 'mp_sift_layout')}
    assert sizers == set(CASES) == set(REFUSED)


@pytest.mark.parametrize('name', sorted(CASES))
def test_sizes_are_the_recorded_ones(name):
    lib = _lib.load_library()
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert {k for k in golden if k.startswith(name + '(')} == {key(name, a) for a in CASES[name]}
    for args in CASES[name]:
        rc, value = call(lib, name, args)
        assert rc == _lib.MP_OK, key(name, args)
        assert value == golden[key(name, args)], key(name, args)


@pytest.mark.parametrize('name', sorted(REFUSED))
def test_one_step_outside_each_limit_is_refused(name):
    lib = _lib.load_library()
    for args in REFUSED[name]:
        rc, value = call(lib, name, args)
        assert rc == MP_EINVAL, key(name, args)
        assert value in (-1, []), key(name, args)                    # ... and nothing was written
    assert getattr(lib, name)(*CASES[name][0], None) == MP_EINVAL    # no place for the answer
