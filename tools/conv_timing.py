"""Developer tool (GPU box; library built with MP_HIPCC_FLAGS=-DMP_TIMING, MP_LIB pointing at it): where does a convolution
workgroup's time go?

    python tools/conv_timing.py KERNEL        direct | persist | f16 | f16_res | wino43

Prints mean / p10 / p90 cycles per phase, as recorded by the phase timers of the kernel's source:
  direct   conv_mfma.hip's one-tile-per-workgroup kernel, per wave: prologue / chunk 0 / chunk boundary / chunk 1 / epilogue of the
           2-chunk layers.  MP_TIMING_SIMD=1 adds the per-SIMD occupancy of the matrix pipe.
  persist  conv_mfma.hip's persistent fp32 workgroups, per work item, and the shader clock during the kernel
  f16      conv_f16.hip's persistent fp16 workgroups, per work item
  f16_res  conv_f16_res.hip's fused fp16 conv1+conv2 launch (wave 0 of groups 0 / 1), per item.  Every launch of the kernel family
           overwrites the table; no height is selected.
  wino43   conv_wino43.hip's persistent workgroups per work item, as seen by wave 0
MP_TIMING_H selects the launch by input height (a comma-separated list: one report per height); where several launches share a
height the last writer is read.  fp32, 64 x 480 x 640: 480 conv1+2, 240 conv3 then conv4, 120 conv5 / conv6, 60 conv7 / 8 / heads.
wino43: +H a pooled layer (480: conv1+2, 240: conv4, 120: conv6), -H an un-pooled one (-240: conv3, -120: conv5, -60: conv7, conv8,
heads).  fp16, 16 x 1024 x 1280: 1024 enc.conv2, 512 conv3 then conv4, ..."""
import sys, os, ctypes
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import mp_oracle as O
import multipoint_amd.models as models
from multipoint_amd import _lib

# per kernel: model precision, suffix of the mp_debug_* accessors, shape of the table, default MP_TIMING_H (None: no height selector),
# and for the per-item phase tables: row labels (slot i of a row; the last slot counts the items), row format, header / summary line
KERNELS = {
    'direct': dict(fp16=False, suffix='', shape=(8192 * 4, 16), height='480'),
    'persist': dict(fp16=False, suffix='', shape=(512, 8), height='240', row='%-28s', unit='cycles/item',
                    labels=['item start -> first step', 'MFMA steps (all chunks)', 'chunk-end barrier', '(unused)', 'epilogue', '(unused)', '(unused)'],
                    summary='workgroups %(wg)d, items per workgroup %(items).1f, sum %(tot).0f cycles/item (MFMA: 36 steps x 1024 = 36864 per 32-channel chunk)'),
    'f16': dict(fp16=True, suffix='_f16', shape=(512, 8), height='1024', row='%-28s', unit='cycles/item',
                labels=['item start -> first step', 'MFMA steps', 'barrier after steps', 'data landed + LDS write', 'epilogue', 'barrier before next item'],
                summary='items per workgroup %(items).1f, sum %(tot).0f cycles/item (ideal MFMA: 36 steps x 128 = 4608 per 64-channel chunk)'),
    'f16_res': dict(fp16=True, suffix='_f16_res', shape=(512, 8), height=None, row='%-34s', unit='cycles/item',
                    labels=['item start -> first step', 'MFMA steps (2 chunks)', 'barrier behind steps (x2)', 'tile production / LDS write (x2)',
                            'barrier before chunk 1', 'epilogue', 'barrier before next item'],
                    summary='items per group %(items).1f, sum %(tot).0f cycles/item (MFMA time: 36 steps x 128 = 4608)'),
    'wino43': dict(fp16=False, suffix='_wino43', shape=(256, 8), height='240', row='   %-40s', unit='ticks/item',
                   labels=['units incl. barriers', 'DMA / LDS wait in front of the barrier', 'epilogue', 'unit loop of an item', 's_barrier behind the wait',
                           '... in even units', '... in odd units'],
                   header='H %(sel)d wave 0: workgroups %(wg)d, items per workgroup %(items).1f'),
}


def setup(fp16=False, warmup=2):
    """The shipped model on synthetic weights, the timing library and a benchmark-sized batch (fp32 64 x 480 x 640, fp16
    16 x 1024 x 1280), warmed up."""
    cfg = dict(O.SHIPPED_MODEL_CONFIG)
    if fp16:
        cfg['mixed_precision'] = True
    net = models.MultiPoint(cfg); net.load_state_dict(O.make_weights(0, cfg)); net.to('cuda'); net.eval()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    img = torch.rand(16, 1, 1024, 1280, device='cuda') if fp16 else torch.rand(64, 1, 480, 640, device='cuda')
    for _ in range(warmup): net({'image': img})
    torch.cuda.synchronize()
    return net, lib, img


def record(net, lib, img, suffix, shape, sel=None):
    """One forward with the launches of input height `sel` recorded; the kernel's table as uint64 [rows][slots]."""
    if sel is not None:
        assert getattr(lib, 'mp_debug_select_height' + suffix)(sel) == 0
    net({'image': img}); torch.cuda.synchronize()
    buf = (ctypes.c_ulonglong * (shape[0] * shape[1]))()
    assert getattr(lib, 'mp_debug_read_timing' + suffix)(buf, shape[0] * shape[1]) == 0
    return np.frombuffer(buf, dtype=np.uint64).reshape(shape)


def report_phases(k, sel, raw):
    """Cycle sums per workgroup -> cycles per item and phase.  Returns the rows of the workgroups that ran, and their item counts."""
    t = raw.astype(np.float64)
    t = t[(t[:, 7] > 0) & (t[:, 7] < 1e6)]
    n = t[:, 7]
    vals = dict(sel=sel, wg=len(t), items=n.mean())
    if 'header' in k:
        print(k['header'] % vals)
    tot = 0
    for i, nm in enumerate(k['labels']):
        v = t[:, i] / n
        tot += v.mean()
        print((k['row'] + ' mean %8.0f  p10 %8.0f  p90 %8.0f ' + k['unit']) % (nm, v.mean(), np.percentile(v, 10), np.percentile(v, 90)))
    if 'summary' in k:
        print(k['summary'] % dict(vals, tot=tot))
    return t, n


def report_clock(sel, t, n, prof):
    """persist: the shader clock during the kernel, from the profile of the instrumented forward."""
    layer = {240: 'enc.conv4', 120: 'enc.conv6', 60: 'desc.conv1x1'}.get(sel)
    if layer in prof:
        ticks = (t[:, :7].sum(axis=1)).mean()
        print('%s: %.3f ms in this (instrumented) run, %.0f ticks per workgroup -> %.3f GHz shader clock during the kernel' % (layer, prof[layer], ticks, ticks / prof[layer] * 1e-6))
        nch = {240: 2, 120: 4}.get(sel, 0)
        if nch:
            need = n.mean() * nch * 576 * 64
            print('MFMA cycles needed per SIMD (1 wave) %.0f = %.1f %% of the ticks' % (need, 100 * need / ticks))


def report_direct(raw):
    """Per-wave s_memtime stamps t0..t7 of the first 8192 workgroups (slot 15: HW_ID | XCC_ID << 32)."""
    t = raw.astype(np.float64)
    ok = (t[:, 7] > t[:, 0]) & (t[:, 0] > 0)
    t = t[ok]; raw = raw[ok]
    print('waves', len(t))
    d = {'  index+issue (t1-t0)': t[:, 1] - t[:, 0], '  land+ldswrite (t3-t1)': t[:, 3] - t[:, 1], '  barrier (t2-t3)': t[:, 2] - t[:, 3],
         'prologue (t2-t0)': t[:, 2] - t[:, 0], 'chunk0 (t5-t2)': t[:, 5] - t[:, 2], 'boundary (t4-t5)': t[:, 4] - t[:, 5],
         'chunk1 (t6-t4)': t[:, 6] - t[:, 4], 'epilogue (t7-t6)': t[:, 7] - t[:, 6], 'total (t7-t0)': t[:, 7] - t[:, 0]}
    for k, v in d.items():
        print('%-24s mean %9.0f  p10 %9.0f  p50 %9.0f  p90 %9.0f' % (k, v.mean(), np.percentile(v, 10), np.percentile(v, 50), np.percentile(v, 90)))
    if os.environ.get('MP_TIMING_SIMD') != '1':
        return
    # per-SIMD occupancy of the matrix pipe (2-chunk layers): how much of the time are 0 / 1 / 2 of the resident
    # waves inside their MFMA loops ([t2,t5] and [t4,t6]), and how many waves are resident ([t0,t7])
    hw = raw[:, 15]
    key = ((hw >> np.uint64(32)) & np.uint64(15)) * np.uint64(1 << 16) + ((hw >> np.uint64(8)) & np.uint64(0xff)) * np.uint64(4) \
        + ((hw >> np.uint64(4)) & np.uint64(3))
    acc_s = np.zeros(4); acc_r = np.zeros(4); nsimd = 0
    for k in np.unique(key):
        w = t[key == k]
        if len(w) < 8:
            continue
        starts = np.sort(w[:, 0])
        lo, hi = starts[2], starts[-3]
        if hi <= lo:
            continue
        ev = []
        for r in w:
            ev += [(r[2], 0, 1), (r[5], 0, -1), (r[4], 0, 1), (r[6], 0, -1), (r[0], 1, 1), (r[7], 1, -1)]
        ev.sort()
        cnt = [0, 0]; prev = lo
        for tt, kind, dlt in ev:
            if tt > lo:
                x = min(tt, hi)
                if x > prev:
                    acc_s[min(cnt[0], 3)] += x - prev; acc_r[min(cnt[1], 3)] += x - prev
                    prev = x
            cnt[kind] += dlt
            if tt >= hi:
                break
        nsimd += 1
    print('SIMDs analysed', nsimd)
    print('waves in MFMA loop   0: %.1f %%   1: %.1f %%   2: %.1f %%' % tuple(100 * acc_s[:3] / acc_s.sum()))
    print('waves resident       0: %.1f %%   1: %.1f %%   2: %.1f %%  3+: %.1f %%' % tuple(100 * acc_r / acc_r.sum()))


def main(name):
    k = KERNELS[name]
    net, lib, img = setup(k['fp16'])
    heights = [None] if k['height'] is None else [int(x) for x in os.environ.get('MP_TIMING_H', k['height']).split(',')]
    for sel in heights:
        if name == 'persist':
            net.profile(True)
        raw = record(net, lib, img, k['suffix'], k['shape'], sel)
        if name == 'direct':
            report_direct(raw)
            continue
        if name == 'persist':
            prof = {n: ms for n, ms, fl in net.profile_read()}
            net.profile(False)
        t, n = report_phases(k, sel, raw)
        if name == 'persist':
            report_clock(sel, t, n, prof)


if __name__ == '__main__':
    if len(sys.argv) != 2 or sys.argv[1] not in KERNELS:
        sys.exit('usage: conv_timing.py %s' % ' | '.join(KERNELS))
    main(sys.argv[1])
