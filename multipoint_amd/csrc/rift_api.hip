// C ABI of the RIFT baseline: phase-congruency maps, FAST on the maximum-moment map, and the histograms of
// the maximum index map.  The caller owns every buffer; the handle only caches the FFT's twiddle tables (lghd_api.hip).
#include "host.h"
#include "mp_fft.h"

using namespace mp_host;

namespace {

bool fft_frame_ok(int H, int W)
{
    FftPlan p;
    return fft_plan(H, p) && fft_plan(W, p);
}

// the spectrum, the 24 half-transformed complex planes and the six scale-0 amplitude planes of n images
struct RiftWorkspace { float *spectrum, *tmp, *amp; size_t bytes; };

RiftWorkspace rift_workspace(void* base, size_t n, int H, int W)
{
    const size_t HW = (size_t)H * W;
    Carver c(base, alignof(float));
    RiftWorkspace w{};
    w.spectrum = c.take<float>(n * HW * 2);
    w.tmp = c.take<float>(n * HW * 48);
    w.amp = c.take<float>(n * HW * 6);
    w.bytes = c.bytes();
    return w;
}

bool patch_ok(int patch) { return patch > 0 && patch <= MP_RIFT_MAX_PATCH && patch % 12 == 0; }

const char* const PATCH_RULE = ": patch_size must be a positive multiple of 12, at most 156";

}  // namespace

extern "C" {

int mp_rift_workspace_bytes(int B, int H, int W, long long* bytes)
{
    if (!bytes || !frames_ok(B, H, W, 1, 32767) || !fft_frame_ok(H, W)) return MP_EINVAL;
    *bytes = (long long)rift_workspace(nullptr, B < 4 ? B : 4, H, W).bytes;
    return MP_OK;
}

int mp_phase_congruency(mp_handle* h, const unsigned char* u8, const float* bank, int B, int H, int W, float k, float g, float cutoff,
                        float* M, float* m, unsigned char* mim, float* T, float* amp, void* workspace, long long workspace_bytes,
                        void* stream)
{
    if (!h) return MP_EINVAL;
    if (!u8 || !bank || !M || !m || !mim || !T || !workspace) return fail(h, MP_EINVAL, "mp_phase_congruency: NULL tensor");
    if (!frames_ok(B, H, W, 1, 32767)) return fail(h, MP_EINVAL, "mp_phase_congruency: need 0 < B <= 65535");
    if (!fft_frame_ok(H, W))
        return fail(h, MP_EINVAL, "mp_phase_congruency: frame of " + std::to_string(H) + " x " + std::to_string(W) +
                                      ": both sizes must be 2^a 3^b 5^c in [8, 4096]");
    if (!(k >= 0.f) || !std::isfinite(k) || !std::isfinite(g) || !std::isfinite(cutoff))
        return fail(h, MP_EINVAL, "mp_phase_congruency: k must be finite and not negative, g and cutoff finite");
    const size_t per = rift_workspace(nullptr, 1, H, W).bytes;
    int rc = need_workspace(h, "mp_phase_congruency", workspace_bytes, per, "mp_rift_workspace_bytes", "one image ");
    if (rc != MP_OK) return rc;
    const int chunk = workspace_images(workspace_bytes, per, B);
    MP_HIP(hipSetDevice(h->device));
    const float *tr = nullptr, *tc = nullptr;
    if ((rc = fft_twiddle_table(h, W, &tr)) || (rc = fft_twiddle_table(h, H, &tc))) return rc;
    const long long HW = (long long)H * W;
    const RiftWorkspace w = rift_workspace(workspace, chunk, H, W);
    for_image_chunks(B, chunk, [&](long long b0, int nb) {
        launch_rift_phase_congruency(u8 + b0 * HW, bank, nb, H, W, k, g, cutoff, w.spectrum, w.tmp, amp ? amp + b0 * 6 * HW : w.amp,
                                     T + b0 * 6, M + b0 * HW, m + b0 * HW, mim + b0 * HW, tr, tc, static_cast<hipStream_t>(stream));
    });
    return launch_status(h);
}

int mp_rift_detect(mp_handle* h, const float* M, int B, int H, int W, int fast_threshold, int patch_size, unsigned char* u8m,
                   float* range, unsigned char* score, unsigned char* corners, float* prob, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!M || !u8m || !range || !score || !corners) return fail(h, MP_EINVAL, "mp_rift_detect: NULL tensor");
    if (!frames_ok(B, H, W, 1, 32767)) return fail(h, MP_EINVAL, "mp_rift_detect: need 0 < B <= 65535 and frames of at most 32767 x 32767");
    if (fast_threshold < 1 || fast_threshold > 255) return fail(h, MP_EINVAL, "mp_rift_detect: fast_threshold must lie in [1, 255]");
    if (!patch_ok(patch_size)) return fail(h, MP_EINVAL, std::string("mp_rift_detect") + PATCH_RULE);
    MP_HIP(hipSetDevice(h->device));
    launch_rift_detect(M, B, H, W, fast_threshold, patch_size, u8m, range, score, corners, prob, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_rift_describe(mp_handle* h, const unsigned char* mim, int B, int H, int W, int patch_size, const int* kp_yx,
                     const int* kp_count, int K, float* raw, float* unit, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!mim || !kp_yx || !kp_count || (!raw && !unit)) return fail(h, MP_EINVAL, "mp_rift_describe: NULL tensor");
    if (!frames_ok(B, H, W, 1, 32767) || K <= 0) return fail(h, MP_EINVAL, "mp_rift_describe: need 0 < B <= 65535, K > 0");
    if (!patch_ok(patch_size)) return fail(h, MP_EINVAL, std::string("mp_rift_describe") + PATCH_RULE);
    if (patch_size > H || patch_size > W)
        return fail(h, MP_EINVAL, "mp_rift_describe: a frame of " + std::to_string(H) + " x " + std::to_string(W) +
                                      " holds no patch of " + std::to_string(patch_size));
    MP_HIP(hipSetDevice(h->device));
    launch_rift_describe(mim, B, H, W, patch_size, kp_yx, kp_count, K, raw, unit, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

}  // extern "C"
