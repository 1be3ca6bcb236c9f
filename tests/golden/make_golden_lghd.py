"""Generate tests/golden/lghd.npz: what the REFERENCE's own LGHD (multipoint/models/ClassicDetectors.py) returns for the test
images of tests/lghd_restatement.py.  Runs only where the reference checkout is available; it is imported in place through
ref_shim.install().  What runs is the reference's create_filter_bank / lowpassfilter, its per-keypoint descriptor loop and its
ClassicDetectors.forward; the four cv2 calls it makes, which are absent here, come from the restatement: dft / idft (np.fft in
float64), magnitude, and FastFeatureDetector_create (FAST as DESIGN.md 3.11 specifies it).  The file holds data only.

    python tests/golden/make_golden_lghd.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import lghd_restatement as R  # noqa: E402
from ref_shim import REFERENCE_ROOT, install  # noqa: E402

BANK_SHAPE = (48, 80)


def reference_available():
    return os.path.isfile(os.path.join(REFERENCE_ROOT, 'multipoint', 'models', 'ClassicDetectors.py'))


class _KeyPoint:
    def __init__(self, y, x):
        self.pt = (float(x), float(y))


class _Fast:
    def detect(self, image, mask):
        return [_KeyPoint(y, x) for y, x in R.fast_keypoints(image)]


def reference_models():
    models, _ = install()
    import cv2
    cv2.DFT_COMPLEX_OUTPUT = 16

    def dft(src, flags=None):
        f = np.fft.fft2(np.asarray(src, np.float64))
        return np.stack([f.real, f.imag], -1)

    def idft(src):
        f = np.fft.ifft2(src[..., 0] + 1j * src[..., 1]) * (src.shape[0] * src.shape[1])        # cv2.idft does not scale
        return np.stack([f.real, f.imag], -1)

    cv2.dft, cv2.idft = dft, idft
    cv2.magnitude = lambda a, b: np.sqrt(a * a + b * b)
    cv2.FastFeatureDetector_create = _Fast
    return models


def generate():
    import torch
    models = reference_models()
    out = {'names': np.array([n for n, *_ in R.IMAGES]), 'numpy_version': np.array(np.__version__)}
    from multipoint.models.ClassicDetectors import LGHD
    out['bank_48x80'] = LGHD(*BANK_SHAPE).filter_bank.astype(np.float32)
    for name, kind, seed, H, W in R.IMAGES:
        image = R.make_image(kind, seed, H, W)
        net = models.ClassicDetectors({'method': 'LGHD', 'image_H': H, 'image_W': W, 'min_keypoints': 0})
        kps, desc = net.method.detectAndCompute((image * 255.0).astype(np.uint8), None)
        out['kp_' + name] = np.array([[int(round(k.pt[1])), int(round(k.pt[0]))] for k in kps], np.int16).reshape(-1, 2)
        assert desc.max(initial=0) <= 100
        out['desc_' + name] = desc.astype(np.uint8)
        res = net.forward({'image': torch.from_numpy(image)[None, None]})
        out['prob_kp_' + name] = torch.nonzero(res['prob'][0, 0] == 1.0).numpy().astype(np.int16)
    return out


if __name__ == '__main__':
    path = os.path.join(HERE, 'lghd.npz')
    np.savez_compressed(path, **generate())
    print('wrote', path, os.path.getsize(path), 'bytes')
