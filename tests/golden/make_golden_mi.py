"""Generate tests/golden/mi_reference.npz: the values the REFERENCE's own mutual_information_2d
(create_dataset/helper_functions/align.py:52-100) returns for seeded sample vectors.  Runs only where the reference checkout
is available; it is imported in place, with import-time stubs for what its module imports and this function never calls
(cv2, sklearn, the helper_functions star imports: other modules than ref_shim.install() stubs for multipoint.*, which this
generator does not import).  The file holds data only: seeds, settings and the returned floats.

    python tests/golden/make_golden_mi.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_shim import REFERENCE_ROOT  # noqa: E402  (where the reference checkout lies; the other generators' shim)
# (seed, samples, bins, sigma, normalized)
CASES = [(1, 4000, 16, 0.0, False), (2, 4000, 32, 1.5, True), (3, 6000, 100, 5.0, False), (4, 6000, 64, 0.0, True),
         (5, 9000, 256, 0.0, False), (6, 5000, 100, 2.0, True)]


def samples(seed, n):
    """two dependent float32 sample vectors, the first with a share of -1 entries like a warped frame's border"""
    rng = np.random.default_rng(seed)
    x = rng.random(n).astype(np.float32)
    y = (np.sin(6.0 * x) * 0.5 + 0.5 + 0.1 * rng.standard_normal(n)).astype(np.float32)
    x[rng.random(n) < 0.1] = -1.0
    return x, y


def reference_available():
    return os.path.isdir(os.path.join(REFERENCE_ROOT, 'create_dataset', 'helper_functions'))


def reference_function():
    for name in ('cv2', 'sklearn', 'sklearn.metrics', 'helper_functions.disp', 'helper_functions.utils'):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules['sklearn.metrics'].mutual_info_score = None
    pkg = types.ModuleType('helper_functions')
    pkg.__path__ = [os.path.join(REFERENCE_ROOT, 'create_dataset', 'helper_functions')]
    sys.modules.setdefault('helper_functions', pkg)
    sys.dont_write_bytecode = True
    import importlib
    return importlib.import_module('helper_functions.align').mutual_information_2d


def reference_values():
    f = reference_function()
    out = []
    for seed, n, bins, sigma, normalized in CASES:
        x, y = samples(seed, n)
        out.append(float(f(x, y, sigma=sigma, bins=bins, normalized=normalized)))
    return np.array(out, np.float64)


if __name__ == '__main__':
    np.savez(os.path.join(HERE, 'mi_reference.npz'), cases=np.array(CASES, np.float64), values=reference_values(),
             numpy_version=np.array(np.__version__))
    print('wrote mi_reference.npz', reference_values())
