"""CPU: the cases of tests/test_gpu_wino_plan.py against the universe of launch classes of the fp32 Winograd forward, by the
restated planner (tests/wino_plan_restatement.py; the GPU module holds the restatement to the library's own plan), and the power
of their inputs: a geometric error of one pixel, row or column in any 3x3 layer moves an output by at least 4x its bar."""
import pytest
import torch

import wino_plan_restatement as R
from oracle import exact_fixture as X
from oracle import mp_oracle as O
from test_gpu_exact import DESC_TOL, LOGITS_TOL, PROB_TOL

SENSITIVITY = 4.0
GEOMETRIC = ('corner', 'last_row', 'last_col', 'block_edge')

# Class (h), 'a workgroup gets none', cannot occur in the pre-transformed-input launch on any machine: it has 8 output slices, so
# its item count is a multiple of 8 and of every XCD count (1, 2, 4, 8); persistent_grid then never rounds the workgroups up past
# the items, each XCD's range holds at least as many items as the XCD has workgroups, and every workgroup gets one.
# test_unreachable_walks_are_unreachable checks this on the whole grid.
UNREACHABLE_WALKS = {('h', 'vin', 'none')}


def _shipped():
    return O.full_config(X.config('shipped'))


def _case_walks(case):
    out = set()
    if case[0] >= 3:
        for env in R.EMULATED:
            out |= R.walk_classes(R.case_plan('shipped', case, env), R.machine(env)[1])
    return out


def covered():
    """(classes a..g, classes h) the committed cases reach."""
    cfg = _shipped()
    got, walks = set(), set()
    for case in R.CASES + R.IDENTITY_CASES:
        got |= R.classes(R.case_plan('shipped', case), cfg)
        walks |= _case_walks(case)
    zp = O.full_config(X.config('zero_pad'))
    for case in R.CONFIG_CASES['zero_pad']:
        got |= {c for c in R.classes(R.case_plan('zero_pad', case), zp) if c == ('f', 'direct_1x1_zero_pad')}
    return got, walks


def test_restated_walk_hands_out_every_item_once():
    for nxcd in (1, 2, 8):
        for ncu in (nxcd, 4 * nxcd, 6 * nxcd + 1):
            for n in range(1, 90):
                g = R.persistent_grid(n, ncu, nxcd)
                assert g % nxcd == 0 and g <= max(ncu // nxcd * nxcd, nxcd)
                assert sum(R.walk_counts(n, g, nxcd)) == n


def test_cases_cover_the_universe():
    u = R.universe()
    got, walks = covered()
    missing = {c: u[c] for c in u if c not in got}
    assert not missing, 'classes no case reaches (class: a frame that does): %s' % missing
    wmiss = R.walk_universe() - UNREACHABLE_WALKS - walks
    assert not wmiss, wmiss
    # the universe is not trivially small: both kernels, both item shapes, every count of valid tile rows / columns
    for k in R.WINO:
        for pooled in (0, 1):
            assert {c[3] for c in u if c[0] == 'a' and c[1] == (k, 4, pooled) and c[2] == 'rows'} == set(range(1, 9)), (k, pooled)
            assert {c[3] for c in u if c[0] == 'a' and c[1] == (k, 8, pooled) and c[2] == 'cols'} == set(range(1, 9)), (k, pooled)
    assert len(u) >= 180


def test_unreachable_walks_are_unreachable():
    cfg = _shipped()
    seen = set()
    for gen in R.ROUTINGS:
        for H in R.GRID_H:
            for W in R.GRID_W:
                for env in R.EMULATED:
                    e = ','.join(t for t in (R.ROUTINGS[gen], env) if t)
                    seen |= R.walk_classes(R.plan(cfg, 3, H, W, e), R.machine(env)[1])
    assert not (seen & UNREACHABLE_WALKS), seen & UNREACHABLE_WALKS
    assert seen == R.walk_universe() - UNREACHABLE_WALKS


def test_every_case_adds_a_class():
    """No case is dead weight: in the committed order each adds a class the ones before it do not reach."""
    cfg = _shipped()
    have = set()
    for case in R.CASES:
        c = R.classes(R.case_plan('shipped', case), cfg) | _case_walks(case)
        assert c - have, case
        have |= c
    assert len(set(R.CASES)) == len(R.CASES)


@pytest.mark.parametrize('name', R.CONFIGS)
def test_config_cases_cover_their_universe(name):
    assert name in X.CONFIGS
    u = R.config_universe(name)
    got = set()
    for case in R.CONFIG_CASES[name]:
        got |= R.config_classes(R.case_plan(name, case))
    missing = {c: u[c] for c in u if c not in got}
    assert not missing, missing
    assert {(c[1], c[2]) for c in u if c[0] == 'partial'} >= {('wino43b', 0), ('wino43b', 1)}
    if name == 'multispectral':
        cfg = O.full_config(X.config(name))
        assert any(0 < R.n_optical(cfg, B) < B and 2 * R.n_optical(cfg, B) != B for B, _, _, _ in R.CONFIG_CASES[name])


def test_no_case_runs_on_a_flat_image_alone():
    for name, case in all_cases():
        img = R.case_images(0, name, case)
        assert any(img[b].unique().numel() > 1 for b in range(case[0])), (name, case)
        assert img[0].unique().numel() == 9


# ---------------------------------------------------------------------------------------------------------------- inputs
def all_cases():
    return [('shipped', c) for c in R.CASES + R.IDENTITY_CASES] + [(n, c) for n in R.CONFIGS for c in R.CONFIG_CASES[n]]


def layer_names(cfg, enc):
    return ['%s.%d' % (enc, l['conv']) for l in O.encoder_layout(cfg)] + \
        ['detector_head_convolutions.1'] + (['descriptor_head_convolutions.1'] if cfg['descriptor_head'] else [])


def block_edge_places(cfg, p, enc_records):
    """{layer index: (y, x)} in each 3x3 block's OUTPUT frame: the first pixel of the last partial tile block (of the last block
    when none is partial) of the launch that computes the block; no entry where no F(4x4,3x3) launch does."""
    out = {}
    recs = [r for r in enc_records if r['name'] != 'enc.conv1']
    fused = bool(recs[0]['fuse_first'])
    for i, r in enumerate(recs):
        if r['kernel'] not in R.WINO:
            continue
        at = R.last_partial_block(r) or R.blocks(r)[-1][:2]
        if r['name'] == 'enc.conv1+2':
            out[0] = at                               # the first block is evaluated per item of the conv2 launch
        out[i + 1] = (at[0] // 2, at[1] // 2) if r['pooled'] else at
    return out


def _moves(a, b):
    """Does the change from outputs a to b exceed SENSITIVITY x a bar?"""
    if float((a['logits'] - b['logits']).abs().max()) >= SENSITIVITY * LOGITS_TOL:
        return True
    if float((X.prob64(a['logits']) - X.prob64(b['logits'])).abs().max()) >= SENSITIVITY * PROB_TOL:
        return True
    return 'desc_raw' in a and float((X.normalize64(a['desc_raw']) - X.normalize64(b['desc_raw'])).abs().max()) >= SENSITIVITY * DESC_TOL


@pytest.mark.parametrize('name,case', all_cases(), ids=['%s:%dx%dx%d:gen%d' % ((n,) + c) for n, c in all_cases()])
def test_geometric_errors_move_an_output(name, case):
    """corner, last_row, last_col and block_edge (placed at the first pixel of the launch's last partial tile block) in every 3x3
    layer change logits, prob or descriptors by at least 4x the bar on some seed: such a kernel error cannot hide under rounding."""
    missed = missed_errors(name, case)
    assert not missed, missed


def missed_errors(name, case):
    """[(encoder, layer, mutation)] that move no output by SENSITIVITY x its bar on any seed."""
    cfg = O.full_config(X.config(name))
    B, H, W, gen = case
    p = R.case_plan(name, case)
    encs = ['encoder_thermal', 'encoder_optical'] if cfg['multispectral'] else ['encoder']
    heads = p[-1]
    missed = []
    for e, enc in enumerate(encs):
        # the records of this encoder (multispectral: the thermal encoder's come first; one that gets no image has none)
        counts = [B - R.n_optical(cfg, B), R.n_optical(cfg, B)] if cfg['multispectral'] else [B]
        if counts[e] == 0:
            continue
        per = (len(p) - 1) // sum(1 for c in counts if c)
        first = per * sum(1 for c in counts[:e] if c)
        places = block_edge_places(cfg, p, p[first:first + per])
        names = layer_names(cfg, enc)
        nenc = len(O.encoder_layout(cfg))
        if heads['kernel'] in R.WINO:
            at = R.last_partial_block(heads) or R.blocks(heads)[-1][:2]
            for i in range(nenc, len(names)):
                places[i] = at
        todo = {(i, m) for i in range(len(names)) for m in GEOMETRIC}
        for seed in X.SEEDS:
            if not todo:
                break
            sd = R.case_weights(seed, name, case)
            img = R.case_images(seed, name, case)
            kw = {'dtype': torch.float64} if (name, case) in R.DENSE_WEIGHTS else {}
            outs = X.layer_outputs(sd, img, cfg, encoder_name=enc, **kw)
            clean = {k: v for k, v in outs if k in ('logits', 'desc_raw')}
            # a frame of one row (column) has no 'row above' ('column to its left'): the 1 x 1 deepest frame of the 8 x 8 case
            shape = dict((k, v.shape) for k, v in outs)
            todo -= {(i, m) for i, m in todo if (m == 'last_row' and shape[names[i]][2] < 2) or (m == 'last_col' and shape[names[i]][3] < 2)}
            for i, m in sorted(todo):
                mut = (names[i], m, places[i]) if m == 'block_edge' and i in places else (names[i], m)
                got = X.final_outputs(sd, img, cfg, mutate=mut, encoder_name=enc, **kw)
                if _moves(clean, got):
                    todo.discard((i, m))
        missed += [(enc, names[i], m) for i, m in sorted(todo)]
    return missed
