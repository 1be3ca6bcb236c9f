// C ABI of the SIFT baseline (sift.hip).  The caller owns every buffer: one workspace holds the pyramids, the
// candidate and keypoint lists and the scratch of every stage (sift_layout); the handle keeps nothing.
#include "host.h"

using namespace mp_host;

namespace {

// where everything lies in a workspace for B frames of H x W and `cap` list slots per image
SiftLayout sift_layout(int B, int H, int W, int cap)
{
    SiftLayout L{};
    L.B = B; L.H = H; L.W = W; L.cap = cap;
    const int m = 2 * (H < W ? H : W);
    L.noct = (int)std::lrint(std::log2((double)m) - 2.0) + 1;
    if (L.noct > MP_SIFT_MAX_OCTAVES) L.noct = MP_SIFT_MAX_OCTAVES;
    Carver c(nullptr, 256 * sizeof(float));      // the pyramids start on multiples of 256 floats, the lists after them of 256 bytes
    auto floats = [&](long long n) { const long long p = (long long)(c.at / sizeof(float)); c.take<float>((size_t)n); return p; };
    auto take = [&](long long bytes) { const long long p = (long long)c.at; c.take<char>((size_t)bytes); return p; };
    int h = 2 * H, w = 2 * W;
    L.flat[0] = 0;
    for (int o = 0; o < L.noct; ++o) {
        L.h[o] = h; L.w[o] = w;
        L.gauss[o] = floats((long long)B * MP_SIFT_LAYERS * h * w);
        L.dog[o] = floats((long long)B * 5 * h * w);
        L.flat[o + 1] = L.flat[o] + 3LL * h * w;
        h /= 2; w /= 2;
    }
    L.tmp = floats((long long)B * 4 * H * W);
    L.nblk = (int)((L.flat[L.noct] + 1023) / 1024);
    c.align = 256;
    L.cmask = take((long long)B * L.nblk * 256);
    L.seg_count = take((long long)B * L.nblk * 4);
    L.seg_base = take((long long)B * L.nblk * 4);
    L.cand = take((long long)B * cap * 16);
    L.cand_count = take((long long)B * 4);
    L.crec = take((long long)B * cap * 5 * 4);
    L.cn = take((long long)B * cap * 4);
    L.cang = take((long long)B * cap * MP_SIFT_MAX_ORI * 4);
    L.cinfo = take((long long)B * cap * 16);
    L.list = take((long long)B * cap * 6 * 4);
    L.list_count = take((long long)B * 4);
    L.dup = take((long long)B * cap);
    L.bytes = (long long)c.bytes();
    return L;
}

int sift_check(mp_handle* h, const char* who, int B, int H, int W, int cap, const void* ws, long long ws_bytes, SiftLayout* L)
{
    if (!frames_ok(B, H, W, 16, 4096) || cap < 1 || cap > (1 << 24))
        return fail(h, MP_EINVAL, std::string(who) + ": need 1 <= B <= 65535, frames of 16 x 16 to 4096 x 4096 and 1 <= capacity <= 2^24");
    if (!ws) return fail(h, MP_EINVAL, std::string(who) + ": NULL workspace");
    *L = sift_layout(B, H, W, cap);
    return need_workspace(h, who, ws_bytes, (size_t)L->bytes, "mp_sift_workspace_bytes");
}

}  // namespace

extern "C" {

int mp_sift_workspace_bytes(int B, int H, int W, int capacity, long long* bytes)
{
    if (!bytes || !frames_ok(B, H, W, 16, 4096) || capacity < 1 || capacity > (1 << 24)) return MP_EINVAL;
    *bytes = sift_layout(B, H, W, capacity).bytes;
    return MP_OK;
}

int mp_sift_layout(int B, int H, int W, int capacity, long long* layout)
{
    if (!layout || !frames_ok(B, H, W, 16, 4096) || capacity < 1 || capacity > (1 << 24)) return MP_EINVAL;
    const SiftLayout L = sift_layout(B, H, W, capacity);
    layout[0] = L.noct;
    layout[1] = L.cand; layout[2] = L.cand_count; layout[3] = L.list; layout[4] = L.list_count;
    layout[5] = L.crec; layout[6] = L.cn; layout[7] = L.cinfo;
    for (int o = 0; o < L.noct; ++o) {
        long long* p = layout + 8 + 4 * o;
        p[0] = L.h[o]; p[1] = L.w[o]; p[2] = L.gauss[o] * (long long)sizeof(float); p[3] = L.dog[o] * (long long)sizeof(float);
    }
    return MP_OK;
}

int mp_sift_scale_space(mp_handle* h, const unsigned char* u8, int B, int H, int W, int capacity, void* workspace,
                        long long workspace_bytes, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!u8) return fail(h, MP_EINVAL, "mp_sift_scale_space: NULL tensor");
    SiftLayout L;
    const int rc = sift_check(h, "mp_sift_scale_space", B, H, W, capacity, workspace, workspace_bytes, &L);
    if (rc != MP_OK) return rc;
    MP_HIP(hipSetDevice(h->device));
    launch_sift_scale_space(u8, L, workspace, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_sift_detect(mp_handle* h, const unsigned char* u8, int B, int H, int W, int capacity, int nfeatures, void* workspace,
                   long long workspace_bytes, float* keypoints, int* count, int* flags, int N, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!keypoints || !count || !flags) return fail(h, MP_EINVAL, "mp_sift_detect: NULL tensor");
    if (nfeatures < 1 || N < nfeatures) return fail(h, MP_EINVAL, "mp_sift_detect: need 1 <= nfeatures <= N");
    SiftLayout L;
    const int rc = sift_check(h, "mp_sift_detect", B, H, W, capacity, workspace, workspace_bytes, &L);
    if (rc != MP_OK) return rc;
    MP_HIP(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* base = static_cast<char*>(workspace);
    if (u8) launch_sift_scale_space(u8, L, workspace, s);
    launch_sift_detect(L, workspace, flags, s);
    launch_sift_select(reinterpret_cast<const float*>(base + L.list), reinterpret_cast<const int*>(base + L.list_count), B, capacity,
                       nfeatures, N, keypoints, count, reinterpret_cast<unsigned char*>(base + L.dup), s);
    return launch_status(h);
}

int mp_sift_select(mp_handle* h, const float* records, const int* rec_count, int B, int M, int nfeatures, float* keypoints, int* count,
                   int N, void* scratch, long long scratch_bytes, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!records || !rec_count || !keypoints || !count || !scratch) return fail(h, MP_EINVAL, "mp_sift_select: NULL tensor");
    if (!count_ok(B) || M < 1 || M > (1 << 24) || nfeatures < 1 || N < nfeatures || scratch_bytes < (long long)B * M)
        return fail(h, MP_EINVAL, "mp_sift_select: need 1 <= B <= 65535, 1 <= M <= 2^24, 1 <= nfeatures <= N and B * M bytes of scratch");
    MP_HIP(hipSetDevice(h->device));
    launch_sift_select(records, rec_count, B, M, nfeatures, N, keypoints, count, static_cast<unsigned char*>(scratch),
                       static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_sift_describe(mp_handle* h, int B, int H, int W, int capacity, const void* workspace, long long workspace_bytes,
                     const float* keypoints, const int* count, int N, float* desc, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!keypoints || !count || !desc) return fail(h, MP_EINVAL, "mp_sift_describe: NULL tensor");
    if (N < 1 || N > MAX_GRID_Y * 64) return fail(h, MP_EINVAL, "mp_sift_describe: need 1 <= N <= 4193280");
    SiftLayout L;
    const int rc = sift_check(h, "mp_sift_describe", B, H, W, capacity, workspace, workspace_bytes, &L);
    if (rc != MP_OK) return rc;
    MP_HIP(hipSetDevice(h->device));
    launch_sift_describe(L, workspace, keypoints, count, N, desc, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_sift_scatter(mp_handle* h, const float* keypoints, const int* count, int B, int N, int H, int W, float* prob, int* owner,
                    void* stream)
{
    if (!h) return MP_EINVAL;
    if (!keypoints || !count || !prob || !owner) return fail(h, MP_EINVAL, "mp_sift_scatter: NULL tensor");
    if (!frames_ok(B, H, W, 16, 4096) || N < 1 || N > (1 << 24))
        return fail(h, MP_EINVAL, "mp_sift_scatter: need 1 <= B <= 65535, frames of 16 x 16 to 4096 x 4096 and 1 <= N <= 2^24");
    MP_HIP(hipSetDevice(h->device));
    launch_sift_scatter(keypoints, count, B, N, H, W, prob, owner, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

}  // extern "C"
