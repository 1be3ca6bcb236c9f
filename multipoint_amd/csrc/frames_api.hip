// C ABI of the frame preparation (frames.hip): mp_undistort, mp_resize_bgr8, mp_thermal_rescale.  The caller owns every buffer.
#include "host.h"

#pragma clang fp contract(off)

using namespace mp_host;

namespace {

constexpr long long MAX_PIXELS = 1LL << 38;      // per call: the flat pixel index of a launch stays below 2^31 blocks

bool aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// np.percentile's linear method on n values (virtual index (n - 1) q, numpy's _get_indexes): the two ranks quantile q
// interpolates between and the weight of the upper one
void percentile_ranks(long long n, double q, long long* prev, long long* next, double* gamma)
{
    const double vi = (double)(n - 1) * q;
    const double fl = std::floor(vi);
    long long p = (long long)fl, x = p + 1;
    if (vi >= (double)(n - 1)) p = x = n - 1;
    if (vi < 0.0) p = x = 0;
    *prev = p, *next = x, *gamma = vi - fl;
}

}  // namespace

extern "C" {

int mp_undistort(mp_handle* h, const void* src, int dtype, int n, int H, int W, const double* K, const double* D, int n_coeffs,
                 const double* K_new, int rotate180, void* dst, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!src || !dst || !K || !D || !K_new) return fail(h, MP_EINVAL, "mp_undistort: NULL argument");
    if (src == dst) return fail(h, MP_EINVAL, "mp_undistort: src and dst must be different buffers");
    if (dtype != MP_FRAMES_BGR8 && dtype != MP_FRAMES_U16)
        return fail(h, MP_EINVAL, "mp_undistort: dtype must be MP_FRAMES_BGR8 or MP_FRAMES_U16");
    if (n_coeffs != 4 && n_coeffs != 5)
        return fail(h, MP_EINVAL, "mp_undistort: 4 or 5 distortion coefficients (k1, k2, p1, p2[, k3]), got " + std::to_string(n_coeffs));
    if (!frames_ok(n, H, W, 1, 32767) || (long long)n * H * W > MAX_PIXELS)
        return fail(h, MP_EINVAL, "mp_undistort: 1 to 65535 frames of 1 x 1 to 32767 x 32767 pixels, at most 2^38 pixels per call");
    if (!aligned(dst, 4)) return fail(h, MP_EINVAL, "mp_undistort: dst must be 4-byte aligned");
    FramesCamera c{};
    c.fx = K[0], c.fy = K[4], c.cx = K[2], c.cy = K[5];
    c.k1 = D[0], c.k2 = D[1], c.p1 = D[2], c.p2 = D[3], c.k3 = n_coeffs == 5 ? D[4] : 0.0;
    c.nfx = K_new[0], c.nfy = K_new[4], c.ncx = K_new[2], c.ncy = K_new[5];
    const double all[13] = {c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2, c.k3, c.nfx, c.nfy, c.ncx, c.ncy};
    for (double v : all)
        if (!std::isfinite(v)) return fail(h, MP_EINVAL, "mp_undistort: K, D and K_new must be finite");
    if (c.nfx == 0.0 || c.nfy == 0.0) return fail(h, MP_EINVAL, "mp_undistort: the focal lengths of K_new must not be zero");
    MP_HIP(hipSetDevice(h->device));
    launch_undistort(src, dtype == MP_FRAMES_U16, n, H, W, c, rotate180 != 0, dst, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_resize_bgr8(mp_handle* h, const unsigned char* src, int n, int H, int W, int oh, int ow, unsigned char* dst, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!src || !dst) return fail(h, MP_EINVAL, "mp_resize_bgr8: NULL tensor");
    if (src == dst) return fail(h, MP_EINVAL, "mp_resize_bgr8: src and dst must be different buffers");
    if (!frames_ok(n, H, W, 1, 32767) || !frames_ok(n, oh, ow, 1, 32767) || (long long)n * oh * ow > MAX_PIXELS)
        return fail(h, MP_EINVAL, "mp_resize_bgr8: 1 to 65535 frames, source and destination of 1 x 1 to 32767 x 32767 pixels");
    if (!aligned(dst, 4)) return fail(h, MP_EINVAL, "mp_resize_bgr8: dst must be 4-byte aligned");
    MP_HIP(hipSetDevice(h->device));
    launch_resize_bgr8(src, n, H, W, oh, ow, dst, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_thermal_rescale_workspace_bytes(int n, long long* bytes)
{
    if (!bytes || !count_ok(n)) return MP_EINVAL;
    *bytes = (long long)thermal_rescale_workspace_bytes(n);
    return MP_OK;
}

int mp_thermal_rescale(mp_handle* h, const unsigned short* in, int n, int H, int W, int outlier_rejection, unsigned short* clipped,
                       float* rescaled, unsigned short* saved, void* workspace, long long workspace_bytes, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!in || !rescaled || !workspace) return fail(h, MP_EINVAL, "mp_thermal_rescale: NULL tensor");
    if (!frames_ok(n, H, W, 1, 32767)) return fail(h, MP_EINVAL, "mp_thermal_rescale: 1 to 65535 frames of 1 x 1 to 32767 x 32767 pixels");
    if (saved && (saved == in || saved == clipped)) return fail(h, MP_EINVAL, "mp_thermal_rescale: saved must be a buffer of its own");
    if (!aligned(in, 2) || !aligned(clipped, 2) || !aligned(saved, 2) || !aligned(rescaled, 4) || !aligned(workspace, 16))
        return fail(h, MP_EINVAL, "mp_thermal_rescale: misaligned tensor (workspace: 16 bytes)");
    const size_t need = thermal_rescale_workspace_bytes(n);
    if (const int rc = need_workspace(h, "mp_thermal_rescale", workspace_bytes, need, "mp_thermal_rescale_workspace_bytes")) return rc;
    const long long N = (long long)H * W;
    FramesRanks rk{};
    if (outlier_rejection) {
        percentile_ranks(N, 1.0 / 100.0, &rk.rank[0], &rk.rank[1], &rk.gamma[0]);
        percentile_ranks(N, 99.0 / 100.0, &rk.rank[2], &rk.rank[3], &rk.gamma[1]);
    } else {
        rk.rank[0] = rk.rank[1] = 0;              // the bounds are the frame's minimum and maximum: nothing is clipped
        rk.rank[2] = rk.rank[3] = N - 1;
    }
    MP_HIP(hipSetDevice(h->device));
    MP_HIP(hipMemsetAsync(workspace, 0, need, static_cast<hipStream_t>(stream)));
    launch_thermal_rescale(in, n, H, W, rk, clipped, rescaled, saved, workspace, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

}  // extern "C"
