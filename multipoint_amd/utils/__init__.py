# mirrors multipoint/utils/__init__.py for the hot path (matching + utils)
from .matching import *  # noqa: F401,F403
from .utils import *  # noqa: F401,F403
from .evaluation import *  # noqa: F401,F403  (compute_descriptor_metrics, pair_metrics, ...)
from .homographies import *  # noqa: F401,F403  (homographic adaptation: export_keypoints.py)
from .frames import *  # noqa: F401,F403  (frame preparation: prepare_images.py)
from .drawing import *  # noqa: F401,F403  (results as pictures: keypoint, match and alignment views)
from .registration import *  # noqa: F401,F403  (keypoint-free initial transform: Fourier-Mellin phase correlation)
from .ecc import *  # noqa: F401,F403  (ECC direct alignment on gradient images)
from .residual import *  # noqa: F401,F403  (local residual field: windowed correlation to pre-screen aligned pairs)
from .field import *  # noqa: F401,F403  (local alignment correction: fit and apply a smooth displacement field)
