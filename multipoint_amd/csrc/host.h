// Host-side state of libmultipoint_hip.so shared by the C ABI's translation units (api.hip, model_load.hip, forward.hip,
// post_api.hip, estimate_api.hip, align_api.hip): the handle, its layers and device buffers, and the error helpers.  Internal:
// the public C ABI is include/multipoint_hip.h.
#pragma once
#include "../../include/multipoint_hip.h"
#include "mp_common.h"
#include "mp_workspace.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

namespace mp_host {

inline std::string g_create_error;      // error of the last mp_create (no handle to hold it)

// one device allocation the handle owns, freed with it (move-only)
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf(void* p_ = nullptr, size_t bytes_ = 0) : p(p_), bytes(bytes_) {}
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    ~DevBuf() { if (p) (void)hipFree(p); }
};

struct ConvLayer {            // one MFMA conv launch
    const char* name = "";
    float *wpack = nullptr, *bias = nullptr, *scale = nullptr, *shift = nullptr;
    float* u43pack = nullptr;     // 3x3 layers: F(4x4,3x3) weights (conv_wino43.hip)
    // enc.conv2 inside the fused conv1+conv2 launch, conv -> ReLU -> BN models: the first block's BatchNorm folded into this layer --
    // U from g2[o][c][tap] * s1[c] (in double, rounded once) and bias + sum_c t1[c] sum_tap g2[o][c][tap] (exact: with reflection
    // padding every tap of every output lands on a real pixel, so the shift's contribution is one constant per output channel)
    float *u43pack_f1 = nullptr, *bias_f1 = nullptr;
    _Float16* wpack_h = nullptr;  // mixed_precision: fp16 fragments (conv_f16.hip) and the fp16-rounded bias
    float* bias_h = nullptr;
    int cin = 0, cout = 0, taps = 9, nslices = 0;
    bool pool = false, relu = true;
};

struct FirstLayer {
    int channels = 64;            // output channels incl. zero padding (64 or 32)
    float *w = nullptr, *bias = nullptr, *scale = nullptr, *shift = nullptr;
    float *w_h = nullptr, *bias_h = nullptr;      // mixed_precision: fp16-representable copies
    // the fused F(4x4,3x3) conv1+conv2 launch produces relu(conv1) only: bn_first models get their BatchNorm folded into the block's own
    // weights (w s, b s + t), the others into conv2 (ConvLayer::u43pack_f1); without BatchNorm these are the plain weights
    float *w_f1 = nullptr, *bias_f1 = nullptr;
};

struct Encoder {
    FirstLayer first;
    ConvLayer conv[7];
    int nconv = 7;                  // 3x3 layers after the first one: 7, or 3 with double_convolution: false (MultiPoint.py:147-148)
    bool first_pool = false;        // ... where MaxPool2d(2,2) follows the first block directly
};

// one BatchNorm2d layer for the batch-statistics forward (mp_forward_batch_stats): its state_dict prefix, real channels, and the
// un-folded affine parameters
struct BnLayer {
    std::string name;
    int channels = 0;
    float *gamma = nullptr, *beta = nullptr;     // device [channels]
    long long offset = 0;                        // float offset of its [2][channels] statistics in the caller's array
};

struct ProfEntry {
    const char* name;
    hipEvent_t a, b;
    double flop;
};

// the MP_DEBUG developer switches, read once by mp_create: each field is the key of that name, or the key that turns it off
// (debug_switch() in api.hip documents them).  A loaded model's own settings are its ConvPolicy.
struct DebugSwitches {
    bool winograd = true, wino43 = true, fuse_first = true, fuse43 = true, head_fuse = true, vin = true, planar = true;
    bool xplanar = true, f16_res = true, f16_fuse1 = true;
    int wino43_gen = 0, persist = 8, splitk_max = 8, f16_res_groups = 3;
};

// The convolution algorithm of the loaded model: conv_policy() of the switches and the model config, recomputed at every
// mp_load_weights (a reload never inherits the previous model's).
struct ConvPolicy {
    bool direct = false;            // the direct kernels for every 3x3 layer, the first block fused into conv2's (conv_algorithm
                                    // 'direct', MP_DEBUG=no_winograd)
    bool wino43 = true;             // F(4x4,3x3) kernels for the 3x3 layers where they apply (MP_DEBUG=wino43=0 alone: none, and
                                    // the first block keeps its own launch)
    int wino43_gen = 0;             // 0 conv_wino43.hip where it applies and conv_wino43b.hip elsewhere; 1 / 2: only that kernel
    int splitk_max = 8;             // most ranges the input channels of a small launch are cut into (1: never)
};

// the arrays of a mutual-information call in the caller's workspace (mi_workspace() in align_api.hip)
struct MiWorkspace {
    MiEval* ev;
    int2* slots;
    int* nact;
    double* M;
    unsigned *keys, *tkeys;
    unsigned short* tmap;
    float* warped;
    unsigned* counts;
    double *smooth_a, *smooth_b, *part, *rowsum, *colpart, *values, *cand, *candp;
    MiNmState* state;
    MiNmOptions* opts;
    double* tinit;
    int* live;
    size_t bytes;
};

// the refinement mp_mi_refine_begin started (align_api.hip)
struct MiRefine {
    void* workspace = nullptr;
    MiWorkspace w{};
    MiLaunch L{};
    int P = 0, normalized = 0;
    int model = 0;                        // MP_MODEL_*: what the candidate points in w.candp parametrise
    double sigma = 0.0;
    long long smooth_stride = 0;
    const double* reg_init = nullptr;     // the matrices of the problems' start parameters when the objective is regularised
};

// the arrays of an ECC call in the caller's workspace (ecc_workspace() in ecc_api.hip)
struct EccWorkspace {
    int* pair;
    EccState* state;
    double* partial;
    size_t bytes;
};

// the refinement mp_ecc_begin started (ecc_api.hip)
struct EccRefine {
    void* workspace = nullptr;
    EccWorkspace w{};
    const float *packed = nullptr, *thermal = nullptr;
    int Ho = 0, Wo = 0, H = 0, W = 0, P = 0, K = 0;
    EccOptions opt{};
};

// the arrays of a pooled ECC call in the caller's workspace (pooled_workspace() in ecc_pooled_api.hip)
struct EccPooledWorkspace {
    int *group, *active, *offsets, *list, *tmask;
    EccGroup* groups;
    EccPairRec* recs;
    double *quant, *partial;
    size_t bytes;
};

// the pooled refinement mp_ecc_pooled_begin started (ecc_pooled_api.hip)
struct EccPooledRefine {
    void* workspace = nullptr;
    EccPooledWorkspace w{};
    const float *packed = nullptr, *thermal = nullptr;
    const unsigned char* tmasks = nullptr;
    int Ho = 0, Wo = 0, H = 0, W = 0, P = 0, G = 0, K = 0;
    EccOptions opt{};
};

}  // namespace mp_host

struct mp_handle {
    mp_handle(int device_, int ncu_, int xcd_shift_, const mp_host::DebugSwitches& dbg_)
        : device(device_), ncu(ncu_), xcd_shift(xcd_shift_), dbg(dbg_) {}
    const int device;
    const int ncu, xcd_shift;       // machine shape: compute units, log2(XCDs) (mp_create: from the device, MP_DEBUG=ncu / nxcd override)
    const mp_host::DebugSwitches dbg;
    std::string err;
    bool loaded = false;
    mp_model_config cfg{};
    mp_host::ConvPolicy policy;     // ... of cfg
    std::vector<mp_host::DevBuf> weights;   // every array of the loaded model (upload())
    mp_host::Encoder enc[2];        // [0] = encoder / encoder_thermal, [1] = encoder_optical
    mp_host::ConvLayer heads3, det1, desc1;
    mp_host::DevBuf fwd_ws;         // forward workspace (fwd_workspace())
    mp_host::DevBuf nms_ws;         // NMS work map + kept lists
    mp_host::DevBuf match_ws;       // matching arg-min arrays
    mp_host::DevBuf metrics_ws;     // pair metrics: warped keypoints + inverse match map
    mp_host::DevBuf split_ws;       // F(4x4,3x3) split launches: the ranges' pre-bias output tiles
    mp_host::DevBuf vin_ws;         // F(4x4,3x3) VIN launches: the pre-transformed input (ConvParams::vglobal)
    mp_host::DevBuf bs_ws;          // batch-statistics forward workspace (bs_workspace())
    std::vector<mp_host::BnLayer> bn_layers;   // every BatchNorm2d of the loaded model, state_dict order (mp_batch_stats_layer)
    float* bn_ident = nullptr;      // device [1024]: 512 ones | 512 zeros, the identity epilogue of the batch-statistics convolutions
    mp_host::DevBuf nms_state;      // 64 round counters + tile flags
    mp_host::DevBuf kp_scratch;     // segment counts + list totals of the keypoint compaction
    mp_host::DevBuf nms_total;      // int: undecided candidates summed over all calls since the last read
    int last_nms_rounds = 0;
    mp_host::DevBuf tie_state;      // 1 + MP_TIE_MAX_IMAGES ints: top-k tie guard (mp_topk_ambiguous)
    float tie_eps = 6e-5f;          // ... a survivor within this of the k-th score counts as 'at the cut' (mp_topk_tie_guard)
    int tie_min = 4;                // ... an image is flagged when at least this many sit at the cut on EACH side of it; 0: guard off
    int tie_last_B = 0;
    mp_host::DevBuf tie_pairs;      // int per image: footprint tie guard, per-image counts of the latest call's NMS (nms.hip)
    int tie_pairs_min = 16;         // ... an image is flagged when at least this many of its NMS decisions fell between scores within tie_eps; 0: off
    int head_channels = 256;        // width of each 3x3 head convolution (MultiPoint.py:38-53)
    mp_host::DevBuf f16_dummy;      // scratch line for masked-off store lanes of the fp16 kernels
    int* pinned = nullptr;          // small pinned host scratch (img lists, counters)
    mp_host::MiRefine mi;           // the running mutual-information refinement (mp_mi_refine_*)
    mp_host::EccRefine ecc;         // the running ECC refinement (mp_ecc_*)
    mp_host::EccPooledRefine ecc_pooled;   // the running pooled ECC refinement (mp_ecc_pooled_*)
    std::map<int, mp_host::DevBuf> fft_tw;    // FFT twiddle tables by line length (lghd_api.hip)
    mp_host::DevBuf draw_ws;        // owner map of mp_draw_matches: one uint32 per canvas pixel, grow-only (draw.hip)
    std::vector<mp_host::DevBuf> draw_retired;   // ... the buffers it outgrew: a launch on another stream may still use one, so
                                                 // they live as long as the handle (each at most half its successor's size)
    bool prof = false;
    bool head_fallback_noted = false;
    std::vector<mp_host::ProfEntry> prof_entries;
    size_t prof_used = 0;
};

namespace mp_host {

inline int fail(mp_handle* h, int code, const std::string& msg)
{
    if (h) h->err = msg; else g_create_error = msg;
    return code;
}

#define MP_HIP(expr)                                                                          \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return fail(h, MP_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e));       \
    } while (0)

// b holds at least `bytes` (its old contents are lost when it grows)
inline int ensure(mp_handle* h, DevBuf& b, size_t bytes)
{
    if (b.bytes >= bytes) return MP_OK;
    if (b.p) { MP_HIP(hipFree(b.p)); b.p = nullptr; b.bytes = 0; }
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(h, MP_ENOMEM, "hipMalloc(" + std::to_string(bytes) + " B): " + hipGetErrorString(e));
    }
    b.bytes = bytes;
    return MP_OK;
}

// ensure(), and a buffer allocated here is zeroed on s
inline int ensure_zeroed(mp_handle* h, DevBuf& b, size_t bytes, hipStream_t s)
{
    if (b.bytes >= bytes) return MP_OK;
    const int rc = ensure(h, b, bytes);
    if (rc == MP_OK) MP_HIP(hipMemsetAsync(b.p, 0, bytes, s));
    return rc;
}

// the result of the launches just queued: MP_OK, or MP_EHIP with the runtime's error
inline int launch_status(mp_handle* h)
{
    MP_HIP(hipGetLastError());
    return MP_OK;
}

// the most workgroups a launch takes in its grid's y and z: what bounds every batch count that becomes one
constexpr int MAX_GRID_Y = 65535;

inline bool count_ok(long long n) { return n >= 1 && n <= MAX_GRID_Y; }
inline bool sides_ok(int H, int W, int lo, int hi) { return H >= lo && W >= lo && H <= hi && W <= hi; }
inline bool frames_ok(int n, int H, int W, int lo, int hi) { return count_ok(n) && sides_ok(H, W, lo, hi); }

// MP_OK when the caller's workspace holds what `sizer` says the call (or `who`, e.g. "one image ") needs
inline int need_workspace(mp_handle* h, const std::string& fn, long long have, size_t need, const char* sizer, const char* who = "")
{
    if (have >= (long long)need) return MP_OK;
    return fail(h, MP_EINVAL, fn + ": workspace of " + std::to_string(have) + " B, " + who + "needs " + std::to_string(need) + " B (" + sizer + ")");
}

// A workspace carved per image (LGHD, RIFT) runs a batch in chunks: the images a workspace of `have` bytes holds at once
// (the caller has refused one that holds none), and launch(first image, images) over all B in chunks of that many
inline int workspace_images(long long have, size_t per_image, int B)
{
    const long long n = have / (long long)per_image;
    return (int)(n < B ? n : B);
}
template <class F> void for_image_chunks(int B, int chunk, F launch)
{
    for (int b0 = 0; b0 < B; b0 += chunk) launch((long long)b0, B - b0 < chunk ? B - b0 : chunk);
}

// MP_OK when `workspace` is the one the handle's running refinement was begun in (`begun`: that session's pointer)
inline int begun_in(mp_handle* h, const char* fn, const void* begun, const void* workspace)
{
    if (begun && begun == workspace) return MP_OK;
    return fail(h, MP_ESTATE, std::string(fn) + ": no refinement was begun in this workspace");
}

// the FFT's twiddle table of length n on the device, cached in the handle (lghd_api.hip)
int fft_twiddle_table(mp_handle* h, int n, const float** table);

}  // namespace mp_host
