"""TEST INFRASTRUCTURE: the launch plan of the fp32 forward (forward.hip: wino43_kind, plan_split_vin, plan_encoder, plan_heads;
mp_wino43.h: w43_cover, w43_launch_tc4, w43_launch_items; mp_common.h: persistent_grid, xcd_range) restated in plain Python, and
the CLASSES of launch geometry a case reaches.  tests/test_wino_plan_host.py holds the committed cases to the universe of classes on
the CPU; tests/test_gpu_wino_plan.py holds this restatement to the library's own plan (mp_forward_plan) and runs the cases.

A plan is a list of dicts with the fields of mp_plan_launch ('name', 'kernel', 'images', 'H', 'W', 'pooled', 'tc4', 'ks_shift',
'vin', 'fuse_first', 'in_layout', 'out_layout', 'workgroups', 'items'), in launch order."""
from oracle import exact_fixture as X
from oracle import mp_oracle as O

ENC_NAMES = ['enc.conv2', 'enc.conv3', 'enc.conv4', 'enc.conv5', 'enc.conv6', 'enc.conv7', 'enc.conv8']
WINO = ('wino43', 'wino43b')
MACHINE = (256, 8)                      # compute units, XCDs of an un-partitioned MI355X


# ------------------------------------------------------------------------------------------------------------------ the model
def _pad(c, g):
    return -(-c // g) * g


def model_layers(cfg):
    """What model_load.hip builds for an fp32 model: {'first_pool', 'first_channels', 'conv': [{name, cin, cout, nslices, pool}],
    'heads3': {...}} with channel counts including their zero padding."""
    cfg = O.full_config(cfg)
    ch, head = O._channels(cfg)
    dbl = bool(cfg['double_convolution'])
    chan = [1, ch[1], ch[1], ch[2], ch[2], ch[3], ch[3], ch[4], ch[4]] if dbl else [1, ch[1], ch[2], ch[3], ch[4]]
    pool = [False, True, False, True, False, True, False, False] if dbl else [True, True, True, False]
    conv = []
    for i in range(1, len(chan) - 1):
        conv.append({'name': ENC_NAMES[i - 1], 'cin': _pad(chan[i], 32), 'cout': _pad(chan[i + 1], 32),
                     'nslices': _pad(chan[i + 1], 64) // 64, 'pool': pool[i]})
    hcout = 2 * head if cfg['descriptor_head'] else head
    heads3 = {'name': 'heads.conv3x3', 'cin': conv[-1]['cout'], 'cout': hcout, 'nslices': _pad(hcout, 64) // 64, 'pool': False}
    # the fused first block's folded weights (build_encoder): channel_version 0, double convolution, reflection padding
    f1 = dbl and cfg['channel_version'] == 0 and bool(cfg['reflection_pad'])
    return {'first_pool': pool[0], 'first_channels': _pad(chan[1], 32), 'conv': conv, 'heads3': heads3, 'u43pack_f1': f1}


def switches(env=''):
    """The MP_DEBUG keys the fp32 plan reads (api.hip: mp_create)."""
    d = {'winograd': True, 'wino43': True, 'wino43_gen': 0, 'fuse_first': True, 'fuse43': True, 'vin': True, 'planar': True,
         'xplanar': True, 'splitk_max': 8, 'ncu': None, 'nxcd': None}
    for tok in (env or '').split(','):
        k, eq, v = tok.strip().partition('=')
        if k == 'no_winograd':
            d['winograd'] = False
        elif k == 'wino43' and eq and int(v) == 0:
            d['wino43'] = False
        elif k == 'wino43_gen' and eq and 0 <= int(v) <= 2:
            d['wino43_gen'] = int(v)
        elif k == 'no_fuse':
            d['fuse_first'] = False
        elif k == 'no_fuse43':
            d['fuse43'] = False
        elif k == 'no_vin':
            d['vin'] = False
        elif k == 'no_planar':
            d['planar'] = False
        elif k == 'no_xplanar':
            d['xplanar'] = False
        elif k == 'splitk_max' and eq and 1 <= int(v) <= 8:
            d['splitk_max'] = int(v)
        elif k in ('ncu', 'nxcd') and eq and int(v) > 0:
            d[k] = int(v)
    d['xplanar'] = d['xplanar'] and d['planar']
    return d


def machine(env='', device=MACHINE):
    """(compute units, XCDs) in effect: the device's, overridden by MP_DEBUG=ncu / nxcd (ncu only downwards)."""
    d = switches(env)
    ncu, nxcd = device
    if d['ncu'] and d['ncu'] <= ncu:
        ncu = d['ncu']
    if d['nxcd']:
        nxcd = d['nxcd']
    return ncu, nxcd


ALGORITHMS = {'auto': 0, 'winograd43': 1, 'winograd43_general': 2, 'direct': 3}


def policy(cfg, d):
    """model_load.hip conv_policy."""
    alg = ALGORITHMS[cfg.get('conv_algorithm', 'auto')]
    direct = alg == 3 or (alg == 0 and not d['winograd'])
    return {'direct': direct, 'wino43': not direct and (alg != 0 or d['wino43']),
            'wino43_gen': 0 if alg == 1 else 2 if alg == 2 else d['wino43_gen'],
            'splitk_max': 1 if cfg.get('batch_invariant') else d['splitk_max']}


# ------------------------------------------------------------------------------------------------------------------ the planner
def w43_cover(H, W):
    """(tc4, tile blocks of an image): the item shape that covers the frame with fewer items, 16 x 32 pixels on a tie."""
    wide = -(-W // 32) * -(-H // 16)
    tall = -(-W // 16) * -(-H // 32)
    return (4, tall) if tall < wide else (8, wide)


def item_pixels(tc4):
    """(OY, OX): output pixels of an item."""
    return 4 * (32 // tc4), 4 * tc4


def persistent_grid(nitems, ncu, nxcd):
    full = ncu // nxcd * nxcd
    need = -(-nitems // nxcd) * nxcd
    return min(need, full)


def walk_counts(nitems, grid, nxcd):
    """Items each workgroup of a persistent launch walks (xcd_range): the items are cut into one contiguous range per XCD, the
    workgroups of an XCD (blockIdx mod nxcd) walk it with the stride of their number."""
    per = -(-nitems // nxcd)
    stride = grid // nxcd
    out = []
    for b in range(grid):
        xcd = b % nxcd
        first, end = xcd * per + b // nxcd, min((xcd + 1) * per, nitems)
        out.append(max(0, -(-(end - first) // stride)))
    assert sum(out) == nitems, (nitems, grid, nxcd)
    return out


def _wino43_kind(cfg, pol, L, H, W):
    if not pol['wino43'] or L['cin'] % 8:
        return 'direct'
    pad_zero = not cfg['reflection_pad']
    ok = L['cin'] % 8 == 0 and L['cout'] % 4 == 0
    if pol['wino43_gen'] != 2 and ok and not pad_zero and H % 4 == 0 and W % 4 == 0 and H >= 4 and W >= 4:
        return 'wino43'
    if pol['wino43_gen'] != 1 and ok and H >= 2 and W >= 2:
        return 'wino43b'
    return 'direct'


def _split_vin(pol, d, L, c, B, H, W, fwd_batch, ncu):
    if c['kernel'] not in WINO or c['fuse_first']:
        return
    if fwd_batch <= 2 and pol['splitk_max'] > 1:
        items = B * w43_cover(H, W)[1] * L['nslices']
        units = L['cin'] // 4
        ks = 0
        while ((items << (ks + 1)) <= ncu and (2 << ks) <= pol['splitk_max'] and (units >> (ks + 1)) >= 4 and
               ((units >> (ks + 1)) & 1) == 0 and ((units >> (ks + 1)) << (ks + 1)) == units):
            ks += 1
        if ks > 0 and items <= 1024:
            c['ks_shift'] = ks
    c['vin'] = int(c['kernel'] == 'wino43' and not L['pool'] and c['ks_shift'] == 0 and c['in_layout'] == 'nhwc' and
                   L['cin'] % 16 == 0 and 16 <= L['cin'] <= 256 and 256 % (L['cin'] // 2) == 0 and d['vin'] and L['nslices'] >= 4)


def _record(L, c, B, H, W, ncu, nxcd):
    r = {'name': 'enc.conv1+2' if c['fuse_first'] else L['name'], 'kernel': c['kernel'], 'images': B, 'H': H, 'W': W,
         'pooled': int(L['pool']), 'tc4': 0, 'ks_shift': c['ks_shift'], 'vin': c['vin'], 'fuse_first': int(c['fuse_first']),
         'in_layout': c['in_layout'], 'out_layout': c['out_layout'], 'workgroups': 0, 'items': 0}
    if c['kernel'] in WINO:
        r['tc4'] = 8 if c['fuse_first'] else w43_cover(H, W)[0]
        OY, OX = item_pixels(r['tc4'])
        r['items'] = B * -(-H // OY) * -(-W // OX) * (L['nslices'] << c['ks_shift'])
        r['workgroups'] = persistent_grid(r['items'], ncu, nxcd)
    return r


def plan(cfg, B, H, W, env='', n_optical=None, device=MACHINE):
    """The records of mp_forward_plan for an fp32 model `cfg` (a full config), a B x H x W forward, the MP_DEBUG string `env` and a
    device of (compute units, XCDs)."""
    cfg = O.full_config(cfg)
    assert not cfg.get('mixed_precision')
    d = switches(env)
    pol = policy(cfg, d)
    ncu, nxcd = machine(env, device)
    M = model_layers(cfg)
    counts = [B, 0]
    if cfg['multispectral']:
        no = B if n_optical is None else n_optical
        counts = [B - no, no]
    out = []
    for nb in counts:
        if nb == 0:
            continue
        cs = []
        hh, ww = (H // 2, W // 2) if M['first_pool'] else (H, W)
        shapes = []
        for i, L in enumerate(M['conv']):
            c = {'kernel': _wino43_kind(cfg, pol, L, hh, ww), 'fuse_first': False, 'in_layout': 'nhwc', 'out_layout': 'nhwc',
                 'ks_shift': 0, 'vin': 0}
            if i == 0:
                fuse43 = (c['kernel'] == 'wino43' and d['fuse43'] and L['pool'] and L['cin'] == 64 and L['cout'] == 64 and
                          cfg['channel_version'] == 0 and M['u43pack_f1'])
                c['fuse_first'] = bool(d['fuse_first'] and cfg['channel_version'] == 0 and not M['first_pool'] and
                                       (pol['direct'] or fuse43))
            producer = (not M['first_pool']) if i == 0 else (cs[i - 1]['kernel'] != 'direct' and M['conv'][i - 1]['pool'])
            if d['planar'] and c['kernel'] != 'direct' and producer:
                c['in_layout'] = 'planar'
            _split_vin(pol, d, L, c, nb, hh, ww, B, ncu)
            if (i > 0 and d['xplanar'] and not M['conv'][i - 1]['pool'] and cs[i - 1]['kernel'] == 'wino43' and
                    cs[i - 1]['ks_shift'] == 0 and c['kernel'] == 'wino43' and c['ks_shift'] == 0 and not c['vin']):
                c['in_layout'] = 'xplanar'
            if i > 0:
                cs[i - 1]['out_layout'] = c['in_layout']
            cs.append(c)
            shapes.append((hh, ww))
            if L['pool']:
                hh, ww = hh // 2, ww // 2
        if not cs[0]['fuse_first']:
            out.append({'name': 'enc.conv1', 'kernel': 'first', 'images': nb, 'H': H, 'W': W, 'pooled': int(M['first_pool']), 'tc4': 0,
                        'ks_shift': 0, 'vin': 0, 'fuse_first': 0, 'in_layout': 'nhwc', 'out_layout': cs[0]['in_layout'],
                        'workgroups': 0, 'items': 0})
        for L, c, (h1, w1) in zip(M['conv'], cs, shapes):
            out.append(_record(L, c, nb, h1, w1, ncu, nxcd))
    L = M['heads3']
    c = {'kernel': _wino43_kind(cfg, pol, L, H // 8, W // 8), 'fuse_first': False, 'in_layout': 'nhwc', 'out_layout': 'nhwc',
         'ks_shift': 0, 'vin': 0}
    _split_vin(pol, d, L, c, B, H // 8, W // 8, B, ncu)
    out.append(_record(L, c, B, H // 8, W // 8, ncu, nxcd))
    return out


# ------------------------------------------------------------------------------------------------------------------ geometry
def blocks(r):
    """[(y0, x0, rows, cols)] of the tile blocks of one image of F(4x4,3x3) launch r: first output pixel, valid tile rows and columns."""
    OY, OX = item_pixels(r['tc4'])
    out = []
    for y0 in range(0, r['H'], OY):
        for x0 in range(0, r['W'], OX):
            out.append((y0, x0, -(-min(OY, r['H'] - y0) // 4), -(-min(OX, r['W'] - x0) // 4)))
    return out


def last_partial_block(r):
    """First pixel (y0, x0) of the last tile block of launch r that has an invalid tile row or column, or None."""
    if r['kernel'] not in WINO:
        return None
    tr4, tc4 = 32 // r['tc4'], r['tc4']
    part = [(y0, x0) for y0, x0, rows, cols in blocks(r) if rows < tr4 or cols < tc4]
    return part[-1] if part else None


def block_of(r, y, x):
    """Which tile block of launch r the layer-input-resolution pixel (y, x) lies in: (block row, block column, tile row, tile column)."""
    OY, OX = item_pixels(r['tc4'])
    return y // OY, x // OX, (y % OY) // 4, (x % OX) // 4


def family(r):
    """The kernel instantiation family of an F(4x4,3x3) launch (class h)."""
    if r['kernel'] == 'wino43b':
        return 'anyframe_pooled' if r['pooled'] else 'anyframe_unpooled'
    if r['fuse_first']:
        return 'fused_first'
    if r['vin']:
        return 'vin'
    return 'pooled' if r['pooled'] else 'plain'


FAMILIES = ('plain', 'pooled', 'fused_first', 'vin', 'anyframe_pooled', 'anyframe_unpooled')
WALKS = ('walk3', 'uneven', 'none')


def walk_classes(p, nxcd):
    """Class (h) of a plan: per family, some workgroup walks >= 3 items / workgroups of one launch walk different (nonzero) counts /
    a workgroup gets no item."""
    out = set()
    for r in p:
        if r['kernel'] not in WINO:
            continue
        w = walk_counts(r['items'], r['workgroups'], nxcd)
        if max(w) >= 3:
            out.add(('h', family(r), 'walk3'))
        if len({v for v in w if v > 0}) > 1:
            out.add(('h', family(r), 'uneven'))
        if min(w) == 0:
            out.add(('h', family(r), 'none'))
    return out


def classes(p, cfg=None):
    """The classes (a) .. (g) of a plan.  cfg: the model config (for the zero-padding class of f)."""
    out = set()
    for r in p:
        k = r['kernel']
        if k == 'direct' and r['name'] != 'enc.conv1' and (r['H'], r['W']) == (1, 1) and cfg is not None and not cfg['reflection_pad']:
            out.add(('f', 'direct_1x1_zero_pad'))
        if k not in WINO:
            continue
        tr4, tc4 = 32 // r['tc4'], r['tc4']
        OY, OX = item_pixels(tc4)
        by, bx = -(-r['H'] // OY), -(-r['W'] // OX)
        key = (k, tc4, r['pooled'])
        out.add(('a', key, 'rows', -(-(r['H'] - (by - 1) * OY) // 4)))
        out.add(('a', key, 'cols', -(-(r['W'] - (bx - 1) * OX) // 4)))
        if k == 'wino43b':
            out.add(('b', r['pooled'], 'H', r['H'] % 4))
            out.add(('b', r['pooled'], 'W', r['W'] % 4))
        out.add(('c', r['name'], k, r['ks_shift']))
        out.add(('d', k, r['pooled'], r['in_layout']))
        if r['name'] == 'heads.conv3x3' and k == 'wino43':
            out.add(('e', r['vin']))
        if r['H'] < OY and r['W'] < OX:
            out.add(('f', k, 'sub_item'))
        if (r['H'], r['W']) in ((4, 4), (2, 2)):
            out.add(('f', k, 'frame', r['H']))
        out.add(('g', k, 'blocks_y', 'one' if by == 1 else 'several'))
        out.add(('g', k, 'blocks_x', 'one' if bx == 1 else 'several'))
        if any(y0 >= 1 and y0 + OY < r['H'] and x0 >= 1 and x0 + OX < r['W'] for y0, x0, _, _ in blocks(r)):
            out.add(('g', k, 'interior', r['name']))
    return out


def config_classes(p):
    """What the cases of a non-shipped config must reach: (layer, kernel, ks_shift), and a block that is partial in BOTH directions
    per (kernel, pooled)."""
    out = set()
    for r in p:
        if r['kernel'] in WINO:
            out.add(('c', r['name'], r['kernel'], r['ks_shift']))
            tr4, tc4 = 32 // r['tc4'], r['tc4']
            if any(rows < tr4 and cols < tc4 for _, _, rows, cols in blocks(r)):
                out.add(('partial', r['kernel'], r['pooled']))
    return out


# ------------------------------------------------------------------------------------------------------------------ the cases
ROUTINGS = {0: '', 2: 'wino43_gen=2'}
GRID_B, GRID_H, GRID_W = (1, 2, 3), range(16, 137, 8), range(16, 273, 8)
# frames beyond the grid: class (g) 'interior' of the layers below full resolution needs three blocks per direction at that level
# (the deepest: H/8 x W/8 = 48 x 96 has 3 x 3 blocks of 16 x 32)
BIG = [(1, 384, 768, 0), (1, 384, 768, 2)]
# (ncu=5: a workgroup count that does not divide the 24 x blocks items of the pre-transformed-input launch at B = 3)
EMULATED = ('ncu=4,nxcd=1', 'ncu=6,nxcd=2', 'ncu=8,nxcd=8', 'ncu=5,nxcd=1')

# (B, H, W, gen) on the shipped config, in the order a greedy cover of the universe picked them (tests/test_wino_plan_host.py
# recomputes the cover's premise: every case adds a class the cases before it do not reach, or is listed in IDENTITY_CASES)
CASES = [(3, 72, 136, 0), (1, 104, 184, 2), (1, 96, 32, 0), (3, 32, 96, 0), (1, 384, 768, 2), (1, 88, 24, 0), (1, 384, 768, 0),
         (1, 40, 72, 0), (1, 120, 40, 0), (1, 16, 16, 2), (1, 136, 16, 0), (1, 16, 56, 0), (1, 80, 16, 2), (1, 64, 32, 0), (1, 56, 16, 0),
         (1, 80, 16, 0), (1, 88, 16, 2), (2, 72, 216, 2), (2, 136, 264, 0), (1, 16, 16, 0), (1, 16, 24, 0), (1, 96, 16, 2)]
# cases kept for the identities of tests/test_gpu_wino_plan.py alone
IDENTITY_CASES = []
# {config: [(B, H, W, gen)]}; multispectral cases route unevenly (N_OPTICAL)
CONFIG_CASES = {
    'bn_first': [(1, 16, 24, 0), (3, 16, 16, 2), (3, 32, 32, 0), (1, 32, 32, 0), (2, 136, 264, 2), (1, 16, 16, 2), (2, 104, 136, 2)],
    'multispectral': [(1, 16, 24, 0), (3, 16, 16, 2), (3, 32, 32, 0), (1, 32, 32, 0), (2, 136, 264, 2), (1, 16, 16, 2)],
    'zero_pad': [(2, 48, 48, 0), (3, 48, 48, 0), (2, 136, 264, 0), (2, 104, 136, 0), (2, 8, 8, 0)],
    'channel_v2': [(2, 48, 56, 0), (3, 48, 48, 0), (3, 48, 48, 2), (2, 64, 64, 0), (2, 48, 48, 2), (3, 64, 64, 0)],
    'channel_v1': [(1, 16, 24, 0), (3, 16, 16, 0), (3, 16, 16, 2), (1, 32, 32, 0), (1, 16, 16, 2), (3, 32, 32, 0)],
    'single_conv': [(1, 16, 24, 0), (3, 32, 32, 0), (3, 16, 16, 2), (1, 32, 32, 0), (2, 136, 264, 2)],
    'desc256_no_final_bn': [(1, 16, 24, 0), (3, 16, 16, 2), (3, 32, 32, 0), (1, 32, 32, 0), (2, 136, 264, 2), (1, 16, 16, 2),
                            (2, 104, 136, 2)],
}
CONFIGS = ('bn_first', 'multispectral', 'zero_pad', 'channel_v1', 'channel_v2', 'single_conv', 'desc256_no_final_bn')


def n_optical(cfg, B):
    """Images of the optical encoder in a case's batch: an uneven route (0 of 1, 1 of 2, 2 of 3)."""
    return (B // 2 + (1 if B >= 3 else 0)) if cfg['multispectral'] else B


def is_optical(cfg, B):
    """The is_optical flags of a case's batch, or None: the FIRST n_optical images are optical."""
    if not cfg['multispectral']:
        return None
    import torch
    return torch.tensor([[b < n_optical(cfg, B)] for b in range(B)])


# {(config, case): n}: another draw of the case's images.  tests/test_wino_plan_host.py requires that a one-pixel, one-row or
# one-column error in any 3x3 layer moves an output by 4x its bar; where the first draw's images let such an error die in a
# max-pool or a ReLU on every seed, the case takes the first later draw on which none does (searched once, on the CPU)
IMAGE_SALT = {
    ('shipped', (1, 104, 184, 2)): 3, ('shipped', (1, 88, 24, 0)): 1, ('shipped', (1, 40, 72, 0)): 2, ('shipped', (1, 120, 40, 0)): 6,
    ('shipped', (1, 136, 16, 0)): 1, ('shipped', (1, 16, 56, 0)): 2, ('shipped', (1, 80, 16, 2)): 1, ('shipped', (1, 64, 32, 0)): 3,
    ('shipped', (1, 56, 16, 0)): 3, ('shipped', (1, 80, 16, 0)): 1, ('shipped', (1, 88, 16, 2)): 4, ('bn_first', (1, 16, 24, 0)): 1,
    ('bn_first', (1, 32, 32, 0)): 1, ('multispectral', (1, 32, 32, 0)): 2, ('multispectral', (1, 16, 16, 2)): 1,
    ('channel_v1', (1, 16, 24, 0)): 6, ('channel_v1', (1, 32, 32, 0)): 2, ('channel_v1', (1, 16, 16, 2)): 8,
    ('zero_pad', (2, 136, 264, 0)): 1, ('channel_v2', (3, 48, 48, 0)): 9, ('channel_v2', (3, 48, 48, 2)): 9,
    ('channel_v2', (2, 48, 48, 2)): 9, ('channel_v2', (2, 48, 56, 0)): 14,
    ('desc256_no_final_bn', (1, 16, 24, 0)): 7, ('desc256_no_final_bn', (1, 32, 32, 0)): 8,
}


def case_images(seed, name, case):
    """The exact-fixture images of a case for weight seed `seed`: no flat image at B = 1 (a flat image cannot see geometry); at
    B > 1 the last image stays flat, as in tests/test_gpu_exact.py."""
    B, H, W, _ = case
    return X.exact_images(seed + 10 * H + W + 1000 * IMAGE_SALT.get((name, case), 0), B, H, W, flat_last=B > 1)


# Cases on dense weights.  At a 1 x 1 frame with zero padding only the centre tap of a 3x3 filter sees data, and the exact fixture
# gives a filter two or three taps among cin x 9 places: through the three layers that run at 1 x 1 (enc.conv7, enc.conv8, heads) an
# error made further up almost never reaches an output, on any image draw.  The case that reaches the direct fallback at 1 x 1
# therefore runs on oracle.make_weights weights (every tap nonzero), with negative and zero BatchNorm scales injected as
# tests/test_gpu_parity.py::test_pooled_epilogue_with_negative_batchnorm_scales does, and takes its truth from the float64 forward
DENSE_WEIGHTS = {('zero_pad', (2, 8, 8, 0))}


def case_weights(seed, name, case):
    """The state_dict of a case: exact-fixture weights, or dense ones for DENSE_WEIGHTS."""
    cfg = X.config(name)
    if (name, case) not in DENSE_WEIGHTS:
        return X.exact_weights(seed, cfg)
    sd = O.make_weights(seed, cfg)
    for k in list(sd):
        if k.startswith('encoder') and k.endswith('.weight') and sd[k].dim() == 1:
            g = sd[k].clone(); g[::3] *= -1.0; g[1] = 0.0
            sd[k] = g
    return sd


def case_truth(sd, img, name, case, iso=None):
    """{'logits', 'prob', 'desc'} in float64 (logits and raw descriptors exact in fp32 on exact-fixture weights)."""
    cfg = X.config(name)
    B, H, W, _ = case
    if (name, case) not in DENSE_WEIGHTS:
        return X.truth(sd, img, cfg, is_optical=iso, fp32=B * H * W > 3 * 72 * 104)
    c = dict(O.full_config(cfg)); c['mixed_precision'] = False; c['normalize_descriptors'] = False
    r = X.forward64(sd, img, c, is_optical=iso, return_logits=True)
    return {'logits': r['logits'], 'prob': X.prob64(r['logits']), 'desc_raw': r['desc'], 'desc': X.normalize64(r['desc'])}


def case_plan(name, case, env='', device=MACHINE):
    B, H, W, gen = case
    cfg = O.full_config(X.config(name))
    e = ','.join(t for t in (ROUTINGS[gen], env) if t)
    return plan(cfg, B, H, W, e, n_optical(cfg, B), device)


def universe():
    """Every class (a) .. (g) the shipped config reaches on the grid (both routings, 256 CUs in 8 XCDs) and on the BIG frames."""
    cfg = O.full_config(X.config('shipped'))
    u = {}
    for gen in ROUTINGS:
        for B in GRID_B:
            for H in GRID_H:
                for W in GRID_W:
                    for c in classes(plan(cfg, B, H, W, ROUTINGS[gen]), cfg):
                        u.setdefault(c, (B, H, W, gen))
    for case in BIG:
        for c in classes(case_plan('shipped', case), cfg):
            u.setdefault(c, case)
    zp = O.full_config(X.config('zero_pad'))
    for case in CONFIG_CASES['zero_pad']:
        for c in classes(case_plan('zero_pad', case), zp):
            if c == ('f', 'direct_1x1_zero_pad'):
                u.setdefault(c, case)
    assert ('f', 'direct_1x1_zero_pad') in u
    return u


def walk_universe():
    """Class (h): every family x walk."""
    return {('h', f, w) for f in FAMILIES for w in WALKS}


def config_universe(name):
    cfg = O.full_config(X.config(name))
    u = {}
    for gen in ROUTINGS:
        for B in GRID_B:
            for H in GRID_H:
                for W in GRID_W:
                    for c in config_classes(plan(cfg, B, H, W, ROUTINGS[gen], n_optical(cfg, B))):
                        u.setdefault(c, (B, H, W, gen))
    return u
