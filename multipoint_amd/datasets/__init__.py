# mirrors multipoint/datasets/__init__.py for the prediction path
from .synthetic_pairs import SyntheticPairs  # noqa: F401
from .image_pair_dataset import ImagePairDataset  # noqa: F401
from .synthetic_shapes import SyntheticShapes  # noqa: F401
from .image_file_pairs import ImageFilePairs  # noqa: F401
from . import augmentation  # noqa: F401,E402


def loader_num_workers(dataset, requested):
    """DataLoader worker count for a dataset of this package: samples whose homographic / photometric augmentation runs on the GPU
    must be produced in the main process (forked loader workers cannot use the device), so `prediction.num_worker`
    of the reference configs is honoured only when the dataset does no GPU work."""
    cfg = getattr(dataset, 'config', {}) or {}
    aug = cfg.get('augmentation', {})
    gpu_work = any(bool(aug.get(k, {}).get('enable', False)) for k in ('homographic', 'photometric'))
    if isinstance(dataset, SyntheticShapes) and cfg.get('on-the-fly', True):
        gpu_work = True                                    # the images themselves are rendered on the GPU
    if isinstance(dataset, ImageFilePairs):
        gpu_work = True                                    # the 8- / 16-bit files are converted to fp32 on the GPU
    if gpu_work and requested:
        print('INFO: homographic / photometric augmentation runs on the GPU inside the dataset; using num_workers=0 '
              'instead of {}'.format(requested))
        return 0
    return int(requested)
from .synthetic_weights import make_weights, make_images, SHIPPED_MODEL_CONFIG  # noqa: F401,E402
