// C ABI of the Fourier-Mellin registration kernels (register.hip).  The caller owns every buffer, the tables
// included; nothing is read back and no entry synchronises.
#include "host.h"
#include "mp_fft.h"

using namespace mp_host;

namespace {

bool plane_ok(int n, int h, int w, int lo) { return frames_ok(n, h, w, lo, MP_FFT_MAX_N); }

}  // namespace

extern "C" {

int mp_register_prepare(mp_handle* h, const float* frames, const float* cs, const float* wy, const float* wx, int n, int H, int W,
                        int N, float* out, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!frames || !wy || !wx || !out) return fail(h, MP_EINVAL, "mp_register_prepare: NULL tensor");
    if (!plane_ok(n, H, W, 1) || N < H || N < W || N > MP_FFT_MAX_N)
        return fail(h, MP_EINVAL, "mp_register_prepare: need 0 < n <= 65535 and max(H, W) <= N <= 4096");
    MP_HIP(hipSetDevice(h->device));
    launch_register_prepare(frames, cs, wy, wx, n, H, W, N, out, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_register_logpolar(mp_handle* h, const float* spectrum, int n, int N, const float* ca, const float* sa, const float* rho,
                         const float* wr, int A, int R, float* out, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!spectrum || !ca || !sa || !rho || !wr || !out) return fail(h, MP_EINVAL, "mp_register_logpolar: NULL tensor");
    if (!plane_ok(n, N, N, 2) || !plane_ok(n, A, R, 1))
        return fail(h, MP_EINVAL, "mp_register_logpolar: need 0 < n <= 65535, 2 <= N <= 4096 and 1 <= A, R <= 4096");
    MP_HIP(hipSetDevice(h->device));
    launch_register_logpolar(spectrum, n, N, ca, sa, rho, wr, A, R, out, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_register_cross_power(mp_handle* h, const float* a, const float* b, const int* group_offsets, int P, int G, int hh, int ww,
                            int accumulate, float* out, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!a || !b || !group_offsets || !out) return fail(h, MP_EINVAL, "mp_register_cross_power: NULL tensor");
    if (P < 0 || (long long)P * hh * ww > 0x7fffffffLL * 64 || !plane_ok(G, hh, ww, 1))
        return fail(h, MP_EINVAL, "mp_register_cross_power: need P >= 0, 0 < G <= 65535 and planes of 1 .. 4096 per side");
    MP_HIP(hipSetDevice(h->device));
    launch_register_cross_power(a, b, group_offsets, P, G, hh, ww, accumulate != 0, out, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_register_peak_workspace_bytes(int G, int hh, int ww, long long* bytes)
{
    if (!bytes || !plane_ok(G, hh, ww, 3)) return MP_EINVAL;
    *bytes = (long long)register_peak_workspace(nullptr, G, hh, ww).bytes;
    return MP_OK;
}

int mp_register_peak(mp_handle* h, const float* planes, int G, int hh, int ww, int stride, int* out_i, float* out_f,
                     void* workspace, long long workspace_bytes, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!planes || !out_i || !out_f || !workspace) return fail(h, MP_EINVAL, "mp_register_peak: NULL tensor");
    long long need = 0;
    if (stride < 1 || stride > 2 || mp_register_peak_workspace_bytes(G, hh, ww, &need) != MP_OK)
        return fail(h, MP_EINVAL, "mp_register_peak: need 0 < G <= 65535, planes of 3 .. 4096 per side and a stride of 1 or 2");
    if (const int rc = need_workspace(h, "mp_register_peak", workspace_bytes, (size_t)need, "mp_register_peak_workspace_bytes")) return rc;
    MP_HIP(hipSetDevice(h->device));
    launch_register_peak(planes, G, hh, ww, stride, out_i, out_f, workspace, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

}  // extern "C"
