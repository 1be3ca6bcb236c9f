"""GPU (MI355X): the default fp32 forward returns the bits recorded before the fused first-block launch (conv_wino43.hip, F1) took the
first block's weights by MFMA broadcast (one register per unit, `cbsz:4 abid:tap`) and kept the second block's taps in registers
(tests/golden/first_block_parent_bits.npz, written by tests/make_golden_first_block.py from the parent build).  The same nine
products in the same order with the bias as the accumulator's initial value: prob and desc are EQUAL, for one-item frames, edge
items, interior items and workgroups that walk many items (MP_DEBUG=ncu=8,nxcd=1)."""
import os

import numpy as np
import pytest

import make_golden_first_block as G

pytestmark = pytest.mark.gpu

_GOLDEN = {}


def _golden():
    if not _GOLDEN:
        with np.load(G.GOLDEN) as z:
            _GOLDEN.update({k: z[k] for k in z.files})
    return _GOLDEN


def _diff(got, want):
    bad = np.argwhere(got != want)
    return '%d of %d differ; first %s: got %r, want %r' % (len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def test_golden_file_has_every_case():
    assert sorted(_golden()) == sorted('%s.%s.%s' % (c, n[0], k) for c, _ in G.CONFIGS for n in G.CASES for k in ('prob', 'desc'))
    assert os.path.getsize(G.GOLDEN) < (1 << 20)


@pytest.mark.parametrize('case', G.CASES, ids=[c[0] for c in G.CASES])
@pytest.mark.parametrize('config', G.CONFIGS, ids=[c[0] for c in G.CONFIGS])
def test_first_block_bits_equal_parent(config, case):
    cname, upd = config
    name, B, H, W, debug = case
    prob, desc = G.run_case(upd, B, H, W, debug)
    want_p, want_d = _golden()['%s.%s.prob' % (cname, name)], _golden()['%s.%s.desc' % (cname, name)]
    assert prob.shape == want_p.shape and desc.shape == want_d.shape
    assert np.array_equal(prob, want_p), (cname, name, 'prob', _diff(prob, want_p))
    assert np.array_equal(desc, want_d), (cname, name, 'desc', _diff(desc, want_d))
