// C ABI of the 2-D FFT (fft.hip) and of the LGHD baseline (lghd.hip): quantisation, FAST, orientation maps, descriptors.  The
// caller owns every buffer; the handle only caches the FFT's twiddle tables, one per line length.
#include "host.h"
#include "mp_fft.h"

using namespace mp_host;

// the device table of length n (built on first use: one synchronous upload per length and handle)
int mp_host::fft_twiddle_table(mp_handle* h, int n, const float** table)
{
    auto it = h->fft_tw.find(n);
    if (it == h->fft_tw.end()) {
        std::vector<float> host((size_t)2 * n);
        fft_twiddles(n, host.data());
        DevBuf buf;
        const int rc = ensure(h, buf, host.size() * sizeof(float));
        if (rc != MP_OK) return rc;
        MP_HIP(hipMemcpy(buf.p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
        it = h->fft_tw.emplace(n, std::move(buf)).first;
    }
    *table = static_cast<const float*>(it->second.p);
    return MP_OK;
}

namespace {

int twiddles(mp_handle* h, int n, const float** table) { return fft_twiddle_table(h, n, table); }

// the spectrum and the 24 half-transformed complex planes of n images
struct LghdWorkspace { float *spectrum, *tmp; size_t bytes; };

LghdWorkspace lghd_workspace(void* base, size_t n, int H, int W)
{
    const size_t HW = (size_t)H * W;
    Carver c(base, alignof(float));
    LghdWorkspace w{};
    w.spectrum = c.take<float>(n * HW * 2);
    w.tmp = c.take<float>(n * HW * 48);
    w.bytes = c.bytes();
    return w;
}

}  // namespace

extern "C" {

int mp_fft_supported(int n)
{
    FftPlan p;
    return fft_plan(n, p) ? 1 : 0;
}

int mp_fft2d(mp_handle* h, const float* in, float* out, int planes, int H, int W, int inverse, int axes, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!in || !out) return fail(h, MP_EINVAL, "mp_fft2d: NULL tensor");
    if (!count_ok(planes) || H <= 0 || W <= 0 || axes < 1 || axes > 3)
        return fail(h, MP_EINVAL, "mp_fft2d: need 0 < planes <= 65535, positive sizes and axes in {1, 2, 3}");
    if (((axes & 1) && !mp_fft_supported(W)) || ((axes & 2) && !mp_fft_supported(H)) || H > MP_FFT_MAX_N || W > MP_FFT_MAX_N)
        return fail(h, MP_EINVAL, "mp_fft2d: line lengths must be 2^a 3^b 5^c in [8, 4096]");
    MP_HIP(hipSetDevice(h->device));
    const float *tr = nullptr, *tc = nullptr;
    int rc;
    if ((axes & 1) && (rc = twiddles(h, W, &tr))) return rc;
    if ((axes & 2) && (rc = twiddles(h, H, &tc))) return rc;
    launch_fft2d(in, out, planes, H, W, inverse != 0, axes, tr, tc, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_lghd_quantize(mp_handle* h, const float* image, unsigned char* u8, long long n, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!image || !u8 || n <= 0 || n > 0x7fffffffLL * 256) return fail(h, MP_EINVAL, "mp_lghd_quantize: bad argument");
    MP_HIP(hipSetDevice(h->device));
    launch_lghd_quantize(image, u8, n, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_lghd_detect(mp_handle* h, const unsigned char* u8, int B, int H, int W, unsigned char* score, unsigned char* corners,
                   float* prob, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!u8 || !score || !corners) return fail(h, MP_EINVAL, "mp_lghd_detect: NULL tensor");
    if (!frames_ok(B, H, W, 1, 32767)) return fail(h, MP_EINVAL, "mp_lghd_detect: need 0 < B <= 65535 and frames of at most 32767 x 32767");
    MP_HIP(hipSetDevice(h->device));
    launch_lghd_detect(u8, B, H, W, score, corners, prob, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_lghd_workspace_bytes(int B, int H, int W, long long* bytes)
{
    if (!bytes || !frames_ok(B, H, W, 1, 32767) || !mp_fft_supported(H) || !mp_fft_supported(W)) return MP_EINVAL;
    *bytes = (long long)lghd_workspace(nullptr, B < 4 ? B : 4, H, W).bytes;
    return MP_OK;
}

int mp_lghd_orientation(mp_handle* h, const unsigned char* u8, const float* bank, int B, int H, int W,
                        unsigned char* orientation, void* workspace, long long workspace_bytes, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!u8 || !bank || !orientation || !workspace) return fail(h, MP_EINVAL, "mp_lghd_orientation: NULL tensor");
    if (!frames_ok(B, H, W, 1, 32767)) return fail(h, MP_EINVAL, "mp_lghd_orientation: need 0 < B <= 65535");
    if (!mp_fft_supported(H) || !mp_fft_supported(W))
        return fail(h, MP_EINVAL, "mp_lghd_orientation: frame of " + std::to_string(H) + " x " + std::to_string(W) +
                                      ": both sizes must be 2^a 3^b 5^c in [8, 4096]");
    const size_t per = lghd_workspace(nullptr, 1, H, W).bytes;
    int rc = need_workspace(h, "mp_lghd_orientation", workspace_bytes, per, "mp_lghd_workspace_bytes", "one image ");
    if (rc != MP_OK) return rc;
    const int chunk = workspace_images(workspace_bytes, per, B);
    MP_HIP(hipSetDevice(h->device));
    const float *tr = nullptr, *tc = nullptr;
    if ((rc = twiddles(h, W, &tr)) || (rc = twiddles(h, H, &tc))) return rc;
    const long long HW = (long long)H * W;
    const LghdWorkspace w = lghd_workspace(workspace, chunk, H, W);
    for_image_chunks(B, chunk, [&](long long b0, int nb) {
        launch_lghd_orientation(u8 + b0 * HW, bank, nb, H, W, w.spectrum, w.tmp, orientation + b0 * 4 * HW, tr, tc,
                                static_cast<hipStream_t>(stream));
    });
    return launch_status(h);
}

int mp_lghd_describe(mp_handle* h, const unsigned char* orientation, int B, int H, int W, const int* kp_yx, const int* kp_count,
                     int K, float* raw, float* unit, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!orientation || !kp_yx || !kp_count || (!raw && !unit)) return fail(h, MP_EINVAL, "mp_lghd_describe: NULL tensor");
    if (!frames_ok(B, H, W, 1, 32767) || K <= 0) return fail(h, MP_EINVAL, "mp_lghd_describe: need 0 < B <= 65535, K > 0");
    MP_HIP(hipSetDevice(h->device));
    launch_lghd_describe(orientation, B, H, W, kp_yx, kp_count, K, raw, unit, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

}  // extern "C"
