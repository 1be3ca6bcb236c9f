"""GPU (MI355X): what mp_forward launches is what mp_forward_plan reports.  With the per-launch profile on, the names a forward
records must begin with exactly the plan's names in order -- each encoder's "enc.conv1" or "enc.conv1+2", its 3x3 layers,
"heads.conv3x3" last -- and everything behind them is the heads' tail, which is not planned.  One case per branch of the walk over
encoders and layers (forward.hip::plan_forward), fp32 and fp16.  tests/test_gpu_wino_plan.py holds the plan's CONTENT to a restated
planner; this file holds the plan to the launches."""
import pytest
import torch

from oracle import exact_fixture as X

pytestmark = pytest.mark.gpu

TAIL = {'heads.tail', 'det.conv1x1', 'det.softmax_shuffle', 'desc.conv1x1', 'desc.l2norm'}

# (config of oracle/exact_fixture.py, config updates, MP_DEBUG, B, H, W, optical images or None, the branch the case takes:
# first launch's name, launches in the plan)
CASES = [
    ('shipped', {}, '', 1, 32, 32, None, 'enc.conv1+2', 8),                              # fused first block
    ('shipped', {}, 'wino43=0', 1, 32, 32, None, 'enc.conv1', 9),                        # stand-alone first block
    ('shipped', {}, 'no_winograd', 1, 32, 32, None, 'enc.conv1+2', 8),                  # direct kernels (fused first block)
    ('single_conv', {}, '', 1, 32, 32, None, 'enc.conv1', 5),                            # first_pool, three layers
    ('multispectral', {}, '', 3, 32, 32, 2, 'enc.conv1+2', 15),                          # two encoders
    ('multispectral', {}, '', 2, 32, 32, 0, 'enc.conv1+2', 8),                           # the optical encoder absent
    ('no_desc_head', {}, '', 1, 32, 32, None, 'enc.conv1+2', 8),                         # no descriptor head
    ('shipped', {'mixed_precision': True}, '', 1, 32, 32, None, 'enc.conv1+2', 8),       # f16_res
    ('shipped', {'mixed_precision': True}, '', 2, 64, 64, None, 'enc.conv1+2', 8),       # f16_res_slices: one profile entry
]
IDS = ['%s%s:%s:%dx%dx%d:%s' % (c[0], '+f16' if c[1] else '', c[2] or 'default', c[3], c[4], c[5], c[6]) for c in CASES]


def _net(monkeypatch, name, upd, env):
    import multipoint_amd.models as M
    if env:
        monkeypatch.setenv('MP_DEBUG', env)
    else:
        monkeypatch.delenv('MP_DEBUG', raising=False)
    cfg = X.config(name, **upd)
    net = M.MultiPoint(cfg); net.load_state_dict(X.exact_weights(0, cfg)); net.to('cuda'); net.eval()
    monkeypatch.delenv('MP_DEBUG', raising=False)
    return net


def _data(B, H, W, n_optical):
    data = {'image': X.exact_images(1, B, H, W, flat_last=False).cuda()}
    if n_optical is not None:
        data['is_optical'] = torch.tensor([[b < n_optical] for b in range(B)]).cuda()
    return data


def _outputs(net, data):
    return {k: v.cpu() for k, v in net(data).items() if v is not None}


@pytest.mark.parametrize('name,upd,env,B,H,W,n_optical,first,count', CASES, ids=IDS)
def test_profiled_launches_begin_with_the_plan(monkeypatch, name, upd, env, B, H, W, n_optical, first, count):
    net = _net(monkeypatch, name, upd, env)
    data = _data(B, H, W, n_optical)
    before = _outputs(net, data)
    plan = net._handle.forward_plan(B, H, W, n_optical)
    planned = [r['name'] for r in plan]
    net.profile(True)
    net.profile_read()
    after = _outputs(net, data)
    ran = [r[0] for r in net.profile_read()]
    net.profile(False)
    print('[plan is what runs %s %s] plan %s, tail %s' % (name, env or 'default', planned, ran[len(planned):]))

    assert ran[:len(planned)] == planned, (ran, planned)
    assert planned[-1] == 'heads.conv3x3'
    rest = ran[len(planned):]
    assert rest and set(rest) <= TAIL, rest
    # one first-block name per encoder that has images, in front of that encoder's layers
    encoders = 1 if n_optical is None else (n_optical > 0) + (n_optical < B)
    starts = [i for i, n in enumerate(planned) if n in ('enc.conv1', 'enc.conv1+2')]
    assert len(starts) == encoders and starts[0] == 0, planned
    # the branch the case is here for
    assert planned[0] == first and len(planned) == count, planned
    if env == 'no_winograd':
        assert all(r['kernel'] in ('first', 'direct') for r in plan), plan
    if upd.get('mixed_precision'):
        kernels = {r['kernel'] for r in plan}
        assert 'f16_res' in kernels and 'f16_res_slices' in kernels and kernels <= {'f16', 'f16_res', 'f16_res_slices'}, plan
        sliced = [r['name'] for r in plan if r['kernel'] == 'f16_res_slices']
        assert all(ran.count(n) == 1 for n in sliced), (sliced, ran)        # one entry for the launches of all its slices
    # reading the plan between two forwards of one handle changes nothing the second one computes
    assert before.keys() == after.keys()
    for k in before:
        assert torch.equal(before[k], after[k]), (name, env, k)
