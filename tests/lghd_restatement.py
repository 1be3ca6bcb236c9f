"""numpy restatement of the LGHD baseline (reference multipoint/models/ClassicDetectors.py, class LGHD), the model the HIP kernels
of multipoint_amd/csrc/lghd.hip and fft.hip are tested against:

  quantize              (image * 255.0).astype(np.uint8) of a float32 image
  fast_scores           FAST-9/16 corner scores (threshold 10) as DESIGN.md 3.11 specifies them; 0 for non-corners
  fast_corners          ... after the strict 3 x 3 non-maximum suppression
  fast_keypoints        row-major (y, x) list of the corners
  filter_bank           create_filter_bank / lowpassfilter with the reference's defaults, float64 [24][H][W], scale-major
  responses             |ifft2(fft2(u8) * bank)| in float64 (np.fft) or, for the error scale, in complex64
  orientation_maps      arg-max over the 6 orientations of every scale (first maximum), uint8 [4][H][W]
  valid_keypoints       the reference's patch-inside-the-frame rule
  patch_descriptors     40 x 40 patches in 4 x 4 cells of 10 x 10 pixels, 6-bin counts, [scale][cell row][cell col][orientation]
  detect_and_compute    LGHD.detectAndCompute

OpenCV is not available where this was written: FAST follows the written specification, not a comparison against cv2.
"""
import numpy as np

CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0),
          (-3, 1), (-2, 2), (-1, 3)]      # (dx, dy)
THRESHOLD = 10
N_SCALES, N_ANGLES, HALF = 4, 6, 20


def quantize(image):
    return (np.asarray(image, np.float32) * np.float32(255.0)).astype(np.uint8)


def fast_scores(u8):
    """int32 [H][W]: the largest t for which 9 contiguous circle pixels (arcs wrap 15 -> 0) are all > p + t or all < p - t, where
    that is at least THRESHOLD; 0 elsewhere and outside 3 <= y <= H - 4, 3 <= x <= W - 4."""
    im = np.asarray(u8).astype(np.int32)
    H, W = im.shape
    out = np.zeros((H, W), np.int32)
    if H < 7 or W < 7:
        return out
    p = im[3:H - 3, 3:W - 3]
    d = np.stack([im[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] - p for dx, dy in CIRCLE])        # [16][h][w]
    best = np.full(p.shape, -256, np.int32)
    for s in range(16):
        arc = d[[(s + k) % 16 for k in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(0) - 1, -arc.max(0) - 1))
    out[3:H - 3, 3:W - 3] = np.where(best >= THRESHOLD, best, 0)
    return out


def fast_corners(scores):
    """bool [H][W]: score > 0 and strictly greater than the scores of all 8 neighbours."""
    s = np.asarray(scores)
    H, W = s.shape
    pad = np.zeros((H + 2, W + 2), s.dtype)
    pad[1:-1, 1:-1] = s
    keep = s > 0
    for j in range(3):
        for i in range(3):
            if (j, i) != (1, 1):
                keep &= s > pad[j:j + H, i:i + W]
    return keep


def fast_keypoints(u8):
    return np.argwhere(fast_corners(fast_scores(u8)))          # row-major (y, x)


def lowpassfilter(H, W, cutoff, n):
    x, y = np.meshgrid(np.linspace(-0.5, 0.5, W), np.linspace(-0.5, 0.5, H))
    radius = np.fft.ifftshift(np.sqrt(x ** 2 + y ** 2))
    return 1.0 / (1.0 + (radius / cutoff) ** (2 * n))


def filter_bank(H, W, n_scales=N_SCALES, n_angles=N_ANGLES, min_wavelength=3, multiplier=1.6, sigma_onf=0.75):
    x, y = np.meshgrid(np.linspace(-0.5, 0.5, W), np.linspace(-0.5, 0.5, H))
    radius = np.fft.ifftshift(np.sqrt(x ** 2 + y ** 2))
    theta = np.fft.ifftshift(np.arctan2(-y, x))
    sintheta, costheta = np.sin(theta), np.cos(theta)
    lp = lowpassfilter(H, W, 0.45, 15)
    bank = np.zeros((n_scales * n_angles, H, W))
    with np.errstate(divide='ignore'):          # log(0) at the DC term, as in the reference: exp(-inf) = 0
        for sc in range(n_scales):
            wavelength = min_wavelength * multiplier ** sc
            lg = np.exp((-(np.log(radius * wavelength)) ** 2) / (2 * np.log(sigma_onf) ** 2)) * lp
            for o in range(n_angles):
                angle = o * np.pi / n_angles
                ds = sintheta * np.cos(angle) - costheta * np.sin(angle)
                dc = costheta * np.cos(angle) + sintheta * np.sin(angle)
                dtheta = np.minimum(np.abs(np.arctan2(ds, dc)) * n_angles * 0.5, np.pi)
                bank[sc * n_angles + o] = lg * ((np.cos(dtheta) + 1) / 2)
    return bank


def responses(u8, bank, single=False):
    """|idft(bank * dft(u8))| without the 1 / N of np.fft.ifft2 (cv2.idft does not scale): float64 [24][H][W].  single=True runs the
    transforms in complex64 (numpy >= 2 keeps the precision): the float32 error scale of the tolerances."""
    img = np.asarray(u8)
    H, W = img.shape
    if single:
        spec = np.fft.fft2(img.astype(np.complex64))
        r = np.fft.ifft2(spec[None] * np.asarray(bank, np.float32)) * np.float32(H * W)
        assert r.dtype == np.complex64, 'numpy >= 2 is needed for a float32 FFT'
    else:
        spec = np.fft.fft2(img.astype(np.float64))
        r = np.fft.ifft2(spec[None] * np.asarray(bank, np.float64)) * (H * W)
    return np.abs(r).astype(np.float64)


def orientation_maps(mag, n_scales=N_SCALES, n_angles=N_ANGLES):
    H, W = mag.shape[1:]
    return np.argmax(mag.reshape(n_scales, n_angles, H, W), axis=1).astype(np.uint8)


def top_two_gap(mag, n_scales=N_SCALES, n_angles=N_ANGLES):
    """float64 [4][H][W]: largest minus second-largest magnitude among the 6 orientations of a scale."""
    H, W = mag.shape[1:]
    s = np.sort(mag.reshape(n_scales, n_angles, H, W), axis=1)
    return s[:, -1] - s[:, -2]


def valid_keypoints(kp, H, W):
    kp = np.asarray(kp).reshape(-1, 2)
    ok = (kp[:, 0] >= HALF) & (kp[:, 0] <= H - HALF) & (kp[:, 1] >= HALF) & (kp[:, 1] <= W - HALF)
    return kp[ok]


def patch_descriptors(ori, kp):
    """ori uint8 [4][H][W], kp (y, x) rows whose patches lie inside the frame -> float64 [n][384] counts."""
    kp = np.asarray(kp).reshape(-1, 2)
    out = np.zeros((len(kp), N_SCALES, 4, 4, N_ANGLES))
    q = HALF // 2
    for i, (y, x) in enumerate(kp):
        patch = ori[:, y - HALF:y + HALF, x - HALF:x + HALF]
        for s in range(N_SCALES):
            for j in range(4):
                for k in range(4):
                    out[i, s, j, k] = np.bincount(patch[s, j * q:(j + 1) * q, k * q:(k + 1) * q].ravel(), minlength=N_ANGLES)
    return out.reshape(len(kp), -1)


def detect_and_compute(u8, bank=None):
    """(keypoints (y, x) int64 [n][2], descriptors float64 [n][384], orientation uint8 [4][H][W])"""
    u8 = np.asarray(u8)
    H, W = u8.shape
    ori = orientation_maps(responses(u8, filter_bank(H, W) if bank is None else bank))
    kp = valid_keypoints(fast_keypoints(u8), H, W)
    return kp, patch_descriptors(ori, kp), ori


def unit_rows(d):
    n = np.sqrt((d * d).sum(-1, keepdims=True))
    return d / np.maximum(n, 1e-12)


# ---- the test images of tests/test_lghd_host.py and tests/test_gpu_lghd.py ----

def noise_image(seed, H, W):
    """uniform noise 0..255, as the float32 image in [0, 1] the model takes"""
    v = np.random.default_rng(seed).integers(0, 256, (H, W))
    return (v / 255.0).astype(np.float32)


def smooth_image(seed, H, W, passes=2):
    """low-passed noise: a [1 4 6 4 1] / 16 binomial blur (reflecting borders) applied `passes` times, rescaled to 0..255"""
    v = np.random.default_rng(seed).integers(0, 256, (H, W)).astype(np.float64)
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16
    for _ in range(passes):
        p = np.pad(v, 2, mode='reflect')
        v = sum(k[i] * p[i:i + H, 2:-2] for i in range(5))
        p = np.pad(v, 2, mode='reflect')
        v = sum(k[i] * p[2:-2, i:i + W] for i in range(5))
    v = np.round((v - v.min()) / (v.max() - v.min()) * 255.0)
    return (v / 255.0).astype(np.float32)


# (name, kind, seed, H, W): the committed inputs of the golden file and of the GPU tests
IMAGES = [('noise_48x80', 'noise', 11, 48, 80), ('smooth_48x80', 'smooth', 12, 48, 80), ('noise_64x64', 'noise', 13, 64, 64),
          ('smooth_64x64', 'smooth', 14, 64, 64), ('noise_96x120', 'noise', 15, 96, 120), ('smooth_96x120', 'smooth', 16, 96, 120)]


def make_image(kind, seed, H, W):
    return noise_image(seed, H, W) if kind == 'noise' else smooth_image(seed, H, W)
