"""Developer tool (GPU box; library built with -DMP_TIMING, MP_LIB pointing at it): how evenly conv_wino43.hip's persistent
workgroups finish -- per launch (MP_TIMING_H as in conv_timing.py wino43) the per-workgroup time (unit loops + epilogues of all its
items, s_memtime ticks of 10 ns) as mean / max over the grid and per XCD (workgroup id & 7).  A static item partition ends with its
slowest workgroup: max / mean - 1 is what a dynamic item queue could recover at most."""
import os
import numpy as np
from conv_timing import KERNELS, setup, record
net, lib, img = setup(warmup=3)
for sel in [int(x) for x in os.environ.get('MP_TIMING_H', '480,-240,240,-120,120,-60').split(',')]:
    rows = []
    for rep in range(3):
        t = record(net, lib, img, KERNELS['wino43']['suffix'], KERNELS['wino43']['shape'], sel).astype(np.float64)
        tot = t[:, 3] + t[:, 2]
        n = t[:, 7]
        ok = (n > 0) & (n < 1e6)
        x = np.arange(256) & 7
        rows.append('rep %d: workgroups %d, items/wg %.2f (min %d max %d); wg time mean %.0f max %.0f (+%.2f %%) min %.0f (%.2f %%); per XCD mean: %s'
                    % (rep, ok.sum(), n[ok].mean(), n[ok].min(), n[ok].max(), tot[ok].mean(), tot[ok].max(), 100 * (tot[ok].max() / tot[ok].mean() - 1),
                       tot[ok].min(), 100 * (tot[ok].min() / tot[ok].mean() - 1),
                       ' '.join('%.0f' % tot[ok & (x == k)].mean() for k in range(8))))
    print('H %d' % sel); print('\n'.join('   ' + r for r in rows), flush=True)
