// C ABI, everything after the forward: NMS and keypoints with their tie guards, descriptor sampling, matching, pair and
// detector metrics, warps, homographic adaptation, losses and photometric augmentation.  (The RANSAC estimators' entries are in
// estimate_api.hip.)
#include "host.h"

using namespace mp_host;

namespace {

bool footprint(float size, double iou, NmsFootprint& fp)
{
    // torchvision nms CPU kernel arithmetic (fp32) for two size x size boxes offset by (dy,dx):
    //   inter = max(0, size-|dy|) * max(0, size-|dx|); ovr = inter / (area + area - inter) > iou
    // -- the last comparison in DOUBLE: nms_kernel_impl(dets, scores, double iou_threshold) promotes the fp32 ovr (include/multipoint_hip.h: mp_box_nms)
    int R = (int)std::ceil(size) - 1;
    if (R < 0) R = 0;
    if (R > MP_NMS_MAX_R) return false;
    fp.R = R;
    const float half = size * 0.5f;
    for (int dy = -R; dy <= R; ++dy) {
        unsigned m = 0;
        for (int dx = -R; dx <= R; ++dx) {
            // boxes [y-half, x-half, y+half, x+half] at a generic in-image position
            const float y1a = 100.f - half, x1a = 100.f - half, y2a = 100.f + half, x2a = 100.f + half;
            const float y1b = (100.f + dy) - half, x1b = (100.f + dx) - half;
            const float y2b = (100.f + dy) + half, x2b = (100.f + dx) + half;
            const float area_a = (y2a - y1a) * (x2a - x1a), area_b = (y2b - y1b) * (x2b - x1b);
            float w = std::fmin(y2a, y2b) - std::fmax(y1a, y1b); if (w < 0.f) w = 0.f;
            float hh = std::fmin(x2a, x2b) - std::fmax(x1a, x1b); if (hh < 0.f) hh = 0.f;
            const float inter = w * hh;
            const float ovr = inter / (area_a + area_b - inter);
            if ((double)ovr > iou) m |= 1u << (dx + R);
        }
        fp.rowmask[dy + R] = m;
    }
    return true;
}

// how the survivors of the suppression are cut down to keep_top_k
enum SelectMode {
    SELECT_SCORE = 0,       // the k highest scores (keypoints.hip)
    SELECT_SPREAD = 1       // the k largest suppression radii (adaptive non-maximal suppression, keypoints_spread.hip)
};

bool robust_ok(float robust) { return std::isfinite(robust) && robust > 0.f && robust <= 1.f; }

int nms_common(mp_handle* h, const float* prob, const unsigned char* mask, int B, int H, int Wc,
               float size, float min_prob, double iou, int topk, int K, int* kp_yx, float* kp_score,
               int* kp_count, float* prob_nms, int max_rounds, hipStream_t s, SelectMode mode = SELECT_SCORE, float robust = 1.f,
               unsigned* kp_radius2 = nullptr)
{
    if (B <= 0 || H <= 0 || Wc <= 0)
        return fail(h, MP_EINVAL, "box_nms: need B,H,W > 0");
    const bool spread = mode == SELECT_SPREAD;
    if (spread && !robust_ok(robust)) return fail(h, MP_EINVAL, "box_nms (spread): robust must be in (0, 1]");
    if (spread && topk <= 0) return fail(h, MP_EINVAL, "box_nms (spread): keep_top_k must be positive");
    NmsFootprint fp{};
    if (!footprint(size, iou, fp))
        return fail(h, MP_EINVAL, "box_nms: box size > " + std::to_string(MP_NMS_MAX_R + 1) + " unsupported");
    // the work map's rows are the caller's rounded up to a multiple of 4 floats (the kernels move 16-byte groups); the padding
    // columns are never candidates, and row-major order -- the tie-break -- is the same in both geometries.  Wc % 4 != 0 (any H x W
    // is a legal argument of utils.box_nms, utils.py:90-91): round 0 reads the map with the generic kernel's scalar loads
    const int W = (Wc + 3) & ~3;
    const long long n = (long long)B * H * W;
    const int ntiles = B * ((W + 31) / 32) * ((H + 31) / 32);
    // workspace: work map | list_idx | list_score | (spread mode) list_r2
    const size_t bytes = (size_t)n * 4 * (spread ? 4 : 3);
    int rc;
    if ((rc = ensure(h, h->nms_ws, bytes))) return rc;
    if ((rc = ensure(h, h->nms_state, (size_t)(64 + 2 * ntiles) * 4))) return rc;
    if ((rc = ensure(h, h->kp_scratch, keypoint_scratch_ints(B, H, W) * 4))) return rc;
    float* work = static_cast<float*>(h->nms_ws.p);
    int* list_idx = reinterpret_cast<int*>(work + n);
    float* list_score = work + 2 * n;
    int* remaining = static_cast<int*>(h->nms_state.p);
    // footprint tie guard: per-image counters the rounds add to and launch_select_keypoints reads and clears
    int* pairs = nullptr;
    if (h->tie_pairs_min > 0) {
        const size_t need = (size_t)(B < 256 ? 256 : B) * 4;
        // growing: the old counters are freed once s is done with them
        if (h->tie_pairs.p && h->tie_pairs.bytes < need) MP_HIP(hipStreamSynchronize(s));
        if ((rc = ensure_zeroed(h, h->tie_pairs, need, s))) return rc;
        pairs = static_cast<int*>(h->tie_pairs.p);
    }
    // the candidate listing (prob * mask > min_prob) is fused into round 0, which reads the probability map itself
    // Rounds: a fixed number without any host read (max_rounds > 0, at most 64), or groups of 8 with one 4-byte read
    // of the undecided count after each group until it is zero (max_rounds == 0).  A round settles every chain of
    // dependent decisions inside a 32 x 32 tile, so the count of rounds is the longest chain measured in tiles: a
    // handful for detector maps, W / 32 for a monotone ramp across the frame -- hence the generous cap.
    int round = 0;
    const int per = max_rounds > 0 ? (max_rounds < 64 ? max_rounds : 64) : 8;
    const int cap = max_rounds > 0 ? per : 4096;
    for (;;) {
        for (int r = 0; r < per && round < cap; ++r, ++round) {
            if (round == 0) launch_nms_round0(prob, mask, min_prob, work, B, H, W, fp, remaining, s, Wc, h->tie_eps, pairs);
            else launch_nms_round(work, B, H, W, fp, remaining, round, s, h->tie_eps, pairs);
        }
        if (max_rounds > 0 || round >= cap) break;
        launch_nms_accumulate(remaining, B, H, W, round - 1, nullptr, s);          // the tiles' undecided counts -> the round's slot
        MP_HIP(hipMemcpyAsync(h->pinned, remaining + ((round - 1) & 63), 4, hipMemcpyDeviceToHost, s));
        MP_HIP(hipStreamSynchronize(s));
        if (h->pinned[0] == 0) break;
    }
    h->last_nms_rounds = round;
    if ((rc = ensure_zeroed(h, h->nms_total, 4, s))) return rc;
    launch_nms_accumulate(remaining, B, H, W, round - 1, static_cast<int*>(h->nms_total.p), s);
    int* tie = nullptr;
    // (spread mode: the plateau and exact-tie conditions describe a score cut and are not evaluated; the footprint guard is)
    if ((!spread && topk > 0 && h->tie_min > 0) || pairs) {
        if ((rc = ensure_zeroed(h, h->tie_state, (1 + MP_TIE_MAX_IMAGES) * 4, s))) return rc;
        tie = static_cast<int*>(h->tie_state.p);
        h->tie_last_B = B < MP_TIE_MAX_IMAGES ? B : MP_TIE_MAX_IMAGES;
    } else {
        h->tie_last_B = 0;
    }
    if (!spread) {
        launch_select_keypoints(work, B, H, W, topk, K, list_idx, list_score, H * W, kp_yx, kp_score, kp_count,
                                prob_nms, static_cast<int*>(h->kp_scratch.p), s, h->tie_eps, topk > 0 ? h->tie_min : 0, tie, Wc,
                                pairs, h->tie_pairs_min);
    } else {
        // keypoints.hip's compaction with its own selection idle (no cut, no outputs): it leaves the row-major survivor list and
        // its length (the last B ints of the scratch) and evaluates the footprint guard; the spread kernels select from that list
        int* scratch = static_cast<int*>(h->kp_scratch.p);
        launch_select_keypoints(work, B, H, W, 0, 0, list_idx, list_score, H * W, nullptr, nullptr, nullptr, nullptr, scratch, s,
                                h->tie_eps, 0, tie, Wc, pairs, h->tie_pairs_min);
        if (prob_nms) MP_HIP(hipMemsetAsync(prob_nms, 0, (size_t)B * H * Wc * sizeof(float), s));
        launch_select_spread(B, H, W, topk, K, list_idx, list_score, reinterpret_cast<unsigned*>(work + 3 * n), H * W,
                             scratch + keypoint_scratch_ints(B, H, W) - B, robust, kp_yx, kp_score, kp_radius2, kp_count, prob_nms,
                             Wc, s);
    }
    MP_HIP(hipGetLastError());
    if (max_rounds == 0 && round >= cap) {
        MP_HIP(hipMemcpyAsync(h->pinned, remaining + ((round - 1) & 63), 4, hipMemcpyDeviceToHost, s));
        MP_HIP(hipStreamSynchronize(s));
        if (h->pinned[0] != 0) return fail(h, MP_ESTATE, "box_nms did not converge within 4096 rounds");
    }
    return MP_OK;
}

}  // namespace

extern "C" {

int mp_box_nms(mp_handle* h, const float* prob, const unsigned char* valid_mask, int B, int H, int W,
               float size, float min_prob, double iou, int keep_top_k, float* prob_nms, int max_rounds,
               void* stream)
{
    if (!h) return MP_EINVAL;
    if (!prob || !prob_nms) return fail(h, MP_EINVAL, "mp_box_nms: NULL tensor");
    MP_HIP(hipSetDevice(h->device));
    return nms_common(h, prob, valid_mask, B, H, W, size, min_prob, iou, keep_top_k, 0, nullptr, nullptr,
                      nullptr, prob_nms, max_rounds, static_cast<hipStream_t>(stream));
}

int mp_detect_keypoints(mp_handle* h, const float* prob, const unsigned char* valid_mask, int B, int H,
                        int W, float size, float min_prob, double iou, int keep_top_k, int K, int* kp_yx,
                        float* kp_score, int* kp_count, int max_rounds, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!prob || !kp_yx || !kp_count || K <= 0) return fail(h, MP_EINVAL, "mp_detect_keypoints: bad argument");
    MP_HIP(hipSetDevice(h->device));
    return nms_common(h, prob, valid_mask, B, H, W, size, min_prob, iou, keep_top_k, K, kp_yx, kp_score,
                      kp_count, nullptr, max_rounds, static_cast<hipStream_t>(stream));
}

int mp_box_nms_spread(mp_handle* h, const float* prob, const unsigned char* valid_mask, int B, int H, int W,
                      float size, float min_prob, double iou, int keep_top_k, float* prob_nms, int max_rounds,
                      float robust, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!prob || !prob_nms) return fail(h, MP_EINVAL, "mp_box_nms_spread: NULL tensor");
    MP_HIP(hipSetDevice(h->device));
    return nms_common(h, prob, valid_mask, B, H, W, size, min_prob, iou, keep_top_k, 0, nullptr, nullptr,
                      nullptr, prob_nms, max_rounds, static_cast<hipStream_t>(stream), SELECT_SPREAD, robust);
}

int mp_detect_keypoints_spread(mp_handle* h, const float* prob, const unsigned char* valid_mask, int B, int H,
                               int W, float size, float min_prob, double iou, int keep_top_k, int K, int* kp_yx,
                               float* kp_score, int* kp_count, int max_rounds, float robust, unsigned* kp_radius2,
                               void* stream)
{
    if (!h) return MP_EINVAL;
    if (!prob || !kp_yx || !kp_count || K <= 0) return fail(h, MP_EINVAL, "mp_detect_keypoints_spread: bad argument");
    MP_HIP(hipSetDevice(h->device));
    return nms_common(h, prob, valid_mask, B, H, W, size, min_prob, iou, keep_top_k, K, kp_yx, kp_score,
                      kp_count, nullptr, max_rounds, static_cast<hipStream_t>(stream), SELECT_SPREAD, robust, kp_radius2);
}

int mp_suppression_radii(mp_handle* h, const int* kp_yx, const float* kp_score, const int* kp_count, int B, int K,
                         float robust, unsigned* radius2, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!kp_yx || !kp_score || !kp_count || !radius2) return fail(h, MP_EINVAL, "mp_suppression_radii: NULL tensor");
    if (!count_ok(B) || K <= 0) return fail(h, MP_EINVAL, "mp_suppression_radii: need 0 < B <= 65535 and K > 0");
    if (!robust_ok(robust)) return fail(h, MP_EINVAL, "mp_suppression_radii: robust must be in (0, 1]");
    MP_HIP(hipSetDevice(h->device));
    launch_suppression_radii(kp_yx, kp_score, kp_count, B, K, robust, radius2, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_nms_unresolved(mp_handle* h, int* unresolved, void* stream)
{
    if (!h || !unresolved) return MP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    *unresolved = 0;
    if (!h->nms_total.p) return MP_OK;
    MP_HIP(hipMemcpyAsync(h->pinned, h->nms_total.p, 4, hipMemcpyDeviceToHost, s));
    MP_HIP(hipMemsetAsync(h->nms_total.p, 0, 4, s));
    MP_HIP(hipStreamSynchronize(s));
    *unresolved = h->pinned[0];
    return MP_OK;
}

int mp_topk_tie_guard(mp_handle* h, float eps, int min_each_side)
{
    if (!h) return MP_EINVAL;
    if (!(eps >= 0.f) || min_each_side < 0) return fail(h, MP_EINVAL, "mp_topk_tie_guard: eps >= 0 and min_each_side >= 0 (0: off)");
    h->tie_eps = eps; h->tie_min = min_each_side;
    return MP_OK;
}

int mp_nms_tie_guard(mp_handle* h, int min_pairs)
{
    if (!h) return MP_EINVAL;
    if (min_pairs < 0) return fail(h, MP_EINVAL, "mp_nms_tie_guard: min_pairs >= 0 (0: off)");
    h->tie_pairs_min = min_pairs;
    return MP_OK;
}

int mp_topk_ambiguous(mp_handle* h, int* flags, int B, int* total, void* stream)
{
    if (!h || !total || B < 0 || (B > 0 && !flags)) return MP_EINVAL;
    hipStream_t s = static_cast<hipStream_t>(stream);
    *total = 0;
    for (int b = 0; b < B; ++b) flags[b] = 0;
    if (!h->tie_state.p) return MP_OK;
    MP_HIP(hipSetDevice(h->device));
    const int nb = B < h->tie_last_B ? B : h->tie_last_B;       // flags exist for the images of the latest call only
    MP_HIP(hipMemcpyAsync(h->pinned, h->tie_state.p, (size_t)(1 + nb) * 4, hipMemcpyDeviceToHost, s));
    MP_HIP(hipMemsetAsync(h->tie_state.p, 0, 4, s));
    MP_HIP(hipStreamSynchronize(s));
    *total = h->pinned[0];
    for (int b = 0; b < nb; ++b) flags[b] = h->pinned[1 + b];
    return MP_OK;
}

int mp_extract_keypoints(mp_handle* h, const float* map, const unsigned char* valid_mask, int B, int H, int W, float thr,
                         int K, int* kp_yx, float* kp_score, int* kp_count, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!map || !kp_yx || !kp_count || K <= 0 || B <= 0 || H <= 0 || W <= 0)
        return fail(h, MP_EINVAL, "mp_extract_keypoints: bad argument");
    MP_HIP(hipSetDevice(h->device));
    int rc;
    if ((rc = ensure(h, h->kp_scratch, keypoint_scratch_ints(B, H, W) * 4))) return rc;
    launch_extract_threshold(map, valid_mask, B, H, W, thr, K, kp_yx, kp_score, kp_count, static_cast<int*>(h->kp_scratch.p),
                             static_cast<hipStream_t>(stream));
    return launch_status(h);
}

// mp_sample_descriptors / mp_sample_descriptors_f: the same checks and launch on int or float keypoints
extern "C++" {          // (a template cannot have C linkage)
template <class KP>
static int sample_descriptors(mp_handle* h, const std::string& fn, const float* desc, int B, int Hc, int Wc, int D, int H, int W,
                              const KP* kp_yx, const int* kp_count, int K, float* out, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!desc || !kp_yx || !kp_count || !out) return fail(h, MP_EINVAL, fn + ": NULL tensor");
    if (D % 64 != 0 || D > 384 || D <= 0)
        return fail(h, MP_EINVAL, fn + ": D must be a multiple of 64 up to 384");
    MP_HIP(hipSetDevice(h->device));
    launch_sample_desc(desc, B, Hc, Wc, D, H, W, kp_yx, kp_count, K, out, static_cast<hipStream_t>(stream));
    return launch_status(h);
}
}

int mp_sample_descriptors(mp_handle* h, const float* desc, int B, int Hc, int Wc, int D, int H, int W,
                          const int* kp_yx, const int* kp_count, int K, float* out, void* stream)
{
    return sample_descriptors(h, "mp_sample_descriptors", desc, B, Hc, Wc, D, H, W, kp_yx, kp_count, K, out, stream);
}

int mp_sample_descriptors_f(mp_handle* h, const float* desc, int B, int Hc, int Wc, int D, int H, int W,
                            const float* kp_yx_f, const int* kp_count, int K, float* out, void* stream)
{
    return sample_descriptors(h, "mp_sample_descriptors_f", desc, B, Hc, Wc, D, H, W, kp_yx_f, kp_count, K, out, stream);
}

int mp_refine_keypoints(mp_handle* h, const float* prob, int B, int H, int W, const int* kp_yx, const int* kp_count, int K,
                        float* kp_sub_yx, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!prob || !kp_yx || !kp_count || !kp_sub_yx) return fail(h, MP_EINVAL, "mp_refine_keypoints: NULL tensor");
    if (B <= 0 || H <= 0 || W <= 0 || K <= 0) return fail(h, MP_EINVAL, "mp_refine_keypoints: B, H, W, K must be positive");
    MP_HIP(hipSetDevice(h->device));
    launch_refine_keypoints(prob, B, H, W, kp_yx, kp_count, K, kp_sub_yx, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

// what the four matchers share: tensors, the grid's pair bound (gridDim.y = P) and the descriptor width -- the MFMA row kernels
// exist for four widths, the scalar route of match_extra.hip takes any up to 384
static int match_check(mp_handle* h, const char* fn, const void* a, const void* b, const void* c, const void* d,
                       int P, int K, int D, bool mfma_rows)
{
    if (!a || !b || !c || !d) return fail(h, MP_EINVAL, std::string(fn) + ": NULL tensor");
    if (!count_ok(P) || K <= 0) return fail(h, MP_EINVAL, std::string(fn) + ": need 0 < P <= 65535, K > 0");
    if (mfma_rows ? (D != 64 && D != 128 && D != 256 && D != 384) : (D <= 0 || D > 384))
        return fail(h, MP_EINVAL, std::string(fn) + (mfma_rows ? ": D must be 64, 128, 256 or 384" : ": D must be in [1, 384]"));
    return MP_OK;
}

// the MFMA matchers' scratch: packed (distance bits, index) keys, two per row and column share (mutual: one per direction,
// nearest: the two smallest)
static int match_workspace(mp_handle* h, int P, int K)
{
    return ensure(h, h->match_ws, (size_t)P * K * 8 * 2 * MATCH_SHARES);
}

int mp_match_mutual_nn(mp_handle* h, const float* descA, const int* countA, const float* descB,
                       const int* countB, long long pair_stride, int count_stride, int P, int K, int D,
                       float threshold, int* match_idx, float* match_dist, int* match_count, void* stream)
{
    if (!h) return MP_EINVAL;
    int rc;
    if ((rc = match_check(h, "mp_match_mutual_nn", descA, descB, countA, countB, P, K, D, true))) return rc;
    if (!match_idx || !match_dist || !match_count) return fail(h, MP_EINVAL, "mp_match_mutual_nn: NULL tensor");
    MP_HIP(hipSetDevice(h->device));
    if ((rc = match_workspace(h, P, K))) return rc;
    unsigned long long* rowbest = static_cast<unsigned long long*>(h->match_ws.p);
    unsigned long long* colbest = rowbest + (size_t)P * K * MATCH_SHARES;
    launch_match_impl(descA, countA, descB, countB, pair_stride, count_stride, P, K, D, threshold, rowbest,
                      colbest, match_idx, match_dist, match_count, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_match_nearest(mp_handle* h, const float* descA, const int* countA, const float* descB, const int* countB,
                     long long pair_stride, int count_stride, int P, int K, int D, double ratio, int* match_idx,
                     float* match_dist, int* match_count, int* second_idx, float* second_dist, void* stream)
{
    if (!h) return MP_EINVAL;
    int rc;
    if ((rc = match_check(h, "mp_match_nearest", descA, descB, countA, countB, P, K, D, true))) return rc;
    if (!match_idx || !match_dist || !match_count) return fail(h, MP_EINVAL, "mp_match_nearest: NULL tensor");
    if (ratio != ratio) return fail(h, MP_EINVAL, "mp_match_nearest: ratio is NaN");
    MP_HIP(hipSetDevice(h->device));
    if ((rc = match_workspace(h, P, K))) return rc;
    launch_match_nearest(descA, countA, descB, countB, pair_stride, count_stride, P, K, D, ratio,
                         static_cast<unsigned long long*>(h->match_ws.p), match_idx, match_dist, match_count, second_idx,
                         second_dist, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_match_guided(mp_handle* h, const float* descA, const int* countA, const float* descB, const int* countB,
                    long long pair_stride, int count_stride, int P, int K, int D, const int* kpA_yx, const int* kpB_yx,
                    const double* homography, float radius, float threshold, int* match_idx, float* match_dist,
                    int* match_count, void* stream)
{
    if (!h) return MP_EINVAL;
    int rc;
    if ((rc = match_check(h, "mp_match_guided", descA, descB, countA, countB, P, K, D, true))) return rc;
    if (!kpA_yx || !kpB_yx || !homography || !match_idx || !match_dist || !match_count)
        return fail(h, MP_EINVAL, "mp_match_guided: NULL tensor");
    if (!(radius > 0.f) || !std::isfinite(radius)) return fail(h, MP_EINVAL, "mp_match_guided: radius must be finite and positive");
    // (the keypoint rows are addressed in units of descriptor rows: pair p starts pair_stride / D rows behind the first)
    if (pair_stride % D != 0) return fail(h, MP_EINVAL, "mp_match_guided: pair_stride must be a multiple of D");
    MP_HIP(hipSetDevice(h->device));
    // the matchers' key arrays, then the gate's positions [2][P][K][2] fp32
    const size_t keys = (size_t)P * K * 8 * 2 * MATCH_SHARES;
    if ((rc = ensure(h, h->match_ws, keys + (size_t)P * K * 4 * sizeof(float)))) return rc;
    unsigned long long* rowbest = static_cast<unsigned long long*>(h->match_ws.p);
    unsigned long long* colbest = rowbest + (size_t)P * K * MATCH_SHARES;
    float* pos = reinterpret_cast<float*>(static_cast<char*>(h->match_ws.p) + keys);
    launch_match_guided(descA, countA, descB, countB, pair_stride, count_stride, P, K, D, kpA_yx, kpB_yx, homography, radius,
                        threshold, pos, rowbest, colbest, match_idx, match_dist, match_count, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_match_knn2(mp_handle* h, const float* descA, const int* countA, const float* descB, const int* countB,
                  long long pair_stride, int count_stride, int P, int K, int D, int* nn_idx, float* nn_dist,
                  void* stream)
{
    if (!h) return MP_EINVAL;
    int rc;
    if ((rc = match_check(h, "mp_match_knn2", descA, descB, countA, countB, P, K, D, false))) return rc;
    if (!nn_idx || !nn_dist) return fail(h, MP_EINVAL, "mp_match_knn2: NULL output");
    MP_HIP(hipSetDevice(h->device));
    launch_match_knn2(descA, countA, descB, countB, pair_stride, count_stride, P, K, D, nn_idx, nn_dist,
                      static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_match_threshold(mp_handle* h, const float* descA, const int* countA, const float* descB, const int* countB,
                       long long pair_stride, int count_stride, int P, int K, int D, float threshold, int capacity,
                       int* list_ij, float* list_dist, int* list_count, void* stream)
{
    if (!h) return MP_EINVAL;
    int rc;
    if ((rc = match_check(h, "mp_match_threshold", descA, descB, countA, countB, P, K, D, false))) return rc;
    if (!list_ij || !list_dist || !list_count) return fail(h, MP_EINVAL, "mp_match_threshold: NULL output");
    if (capacity <= 0) return fail(h, MP_EINVAL, "mp_match_threshold: capacity must be positive");
    if (!(threshold >= 0.f)) return fail(h, MP_EINVAL, "mp_match_threshold: threshold must be non-negative");
    hipStream_t s = static_cast<hipStream_t>(stream);
    MP_HIP(hipSetDevice(h->device));
    MP_HIP(hipMemsetAsync(list_count, 0, (size_t)P * sizeof(int), s));
    launch_match_threshold(descA, countA, descB, countB, pair_stride, count_stride, P, K, D, threshold, capacity, list_ij,
                           list_dist, list_count, s);
    return launch_status(h);
}

int mp_pair_metrics(mp_handle* h, const int* kp_yx, const int* kp_count, const int* match_idx, const double* homography,
                    int P, int K, int H, int W, float threshold_keypoints, int* metrics, unsigned char* tp,
                    void* stream)
{
    if (!h) return MP_EINVAL;
    if (!kp_yx || !kp_count || !match_idx || !homography || !metrics || !tp)
        return fail(h, MP_EINVAL, "mp_pair_metrics: NULL tensor");
    if (P <= 0 || K <= 0 || H <= 0 || W <= 0) return fail(h, MP_EINVAL, "mp_pair_metrics: P, K, H, W must be positive");
    if (!(threshold_keypoints >= 0.f)) return fail(h, MP_EINVAL, "mp_pair_metrics: threshold must be non-negative");
    hipStream_t s = static_cast<hipStream_t>(stream);
    MP_HIP(hipSetDevice(h->device));
    // scratch: warped [2P][K][2] double | inv_idx [P][K] int
    const size_t nw = (size_t)2 * P * K * 2 * sizeof(double), ni = (size_t)P * K * sizeof(int);
    int rc;
    if ((rc = ensure(h, h->metrics_ws, nw + ni))) return rc;
    double* warped = static_cast<double*>(h->metrics_ws.p);
    int* inv_idx = reinterpret_cast<int*>(static_cast<char*>(h->metrics_ws.p) + nw);
    MP_HIP(hipMemsetAsync(inv_idx, 0xff, ni, s));
    MP_HIP(hipMemsetAsync(tp, 0, (size_t)2 * P * K, s));
    MP_HIP(hipMemsetAsync(metrics, 0, (size_t)P * 8 * sizeof(int), s));
    launch_pair_metrics(kp_yx, kp_count, match_idx, homography, P, K, H, W, threshold_keypoints, warped, inv_idx, tp,
                        metrics, s);
    return launch_status(h);
}

int mp_repeatability(mp_handle* h, const int* kp_yx, const int* kp_count, const double* homography, int P, int K, int H,
                     int W, double distance_thresh, int* counts, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!kp_yx || !kp_count || !homography || !counts) return fail(h, MP_EINVAL, "mp_repeatability: NULL tensor");
    if (P <= 0 || K <= 0 || H <= 0 || W <= 0) return fail(h, MP_EINVAL, "mp_repeatability: P, K, H, W must be positive");
    hipStream_t s = static_cast<hipStream_t>(stream);
    MP_HIP(hipSetDevice(h->device));
    int rc;
    if ((rc = ensure(h, h->metrics_ws, (size_t)2 * P * K * 2 * sizeof(long long)))) return rc;
    MP_HIP(hipMemsetAsync(counts, 0, (size_t)P * 4 * sizeof(int), s));
    launch_repeatability(kp_yx, kp_count, homography, P, K, H, W, distance_thresh, static_cast<long long*>(h->metrics_ws.p),
                         counts, s);
    return launch_status(h);
}

int mp_detector_metrics(mp_handle* h, const float* prob, const unsigned char* keypoint_map, int B, int H, int W,
                        float zero_threshold, float distance_thresh, unsigned long long* work, int* rec_index,
                        float* rec_prob, unsigned int* rec_bits, int* rec_count, int* n_gt, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!prob || !keypoint_map || !work || !rec_index || !rec_prob || !rec_bits || !rec_count || !n_gt)
        return fail(h, MP_EINVAL, "mp_detector_metrics: NULL tensor");
    if (!count_ok(B) || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL)
        return fail(h, MP_EINVAL, "mp_detector_metrics: need 0 < B <= 65535, H, W > 0");
    if (!(distance_thresh >= 0.f) || !(distance_thresh < 3.f))
        return fail(h, MP_EINVAL, "mp_detector_metrics: distance_thresh must be in [0, 3) (5 x 5 window)");
    if (!(zero_threshold >= 0.f)) return fail(h, MP_EINVAL, "mp_detector_metrics: zero_threshold must be >= 0");
    MP_HIP(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    MP_HIP(hipMemsetAsync(work, 0, sizeof(unsigned long long) * (size_t)B * H * W, s));
    MP_HIP(hipMemsetAsync(rec_count, 0, sizeof(int) * (size_t)B, s));
    MP_HIP(hipMemsetAsync(n_gt, 0, sizeof(int) * (size_t)B, s));
    launch_detector_metrics(prob, keypoint_map, B, H, W, zero_threshold, distance_thresh, work, rec_index, rec_prob,
                            rec_bits, rec_count, n_gt, s);
    return launch_status(h);
}

int mp_warp_perspective(mp_handle* h, const float* src, int n_src, int H, int W, const double* dst_to_src, int n_out,
                        int Ho, int Wo, int mode, int padding, float* dst, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!src || !dst_to_src || !dst) return fail(h, MP_EINVAL, "mp_warp_perspective: NULL tensor");
    if (n_src <= 0 || n_out <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0 || n_out > MAX_GRID_Y)
        return fail(h, MP_EINVAL, "mp_warp_perspective: sizes must be positive (n_out <= 65535)");
    if ((mode != 0 && mode != 1) || (padding != 0 && padding != 1))
        return fail(h, MP_EINVAL, "mp_warp_perspective: mode must be 0 (bilinear) / 1 (nearest), padding 0 (zeros) / 1 (reflection)");
    MP_HIP(hipSetDevice(h->device));
    launch_warp_perspective(src, n_src, H, W, dst_to_src, n_out, Ho, Wo, mode, padding, dst, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_warp_perspective_cv(mp_handle* h, const float* src, int n, int H, int W, const double* hom_inv, int border,
                           float* dst, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!src || !hom_inv || !dst) return fail(h, MP_EINVAL, "mp_warp_perspective_cv: NULL tensor");
    if (!frames_ok(n, H, W, 1, 32767))
        return fail(h, MP_EINVAL, "mp_warp_perspective_cv: need 0 < n <= 65535 and 0 < H, W <= 32767");
    if (border != 0 && border != 1)
        return fail(h, MP_EINVAL, "mp_warp_perspective_cv: border must be 0 (BORDER_CONSTANT 0) or 1 (BORDER_REFLECT_101)");
    if (src == dst) return fail(h, MP_EINVAL, "mp_warp_perspective_cv: in-place warp is not supported");
    MP_HIP(hipSetDevice(h->device));
    launch_cv_warp_linear(src, n, H, W, hom_inv, border, dst, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_ha_valid_mask(mp_handle* h, const double* hom_inv, int G, int H, int W, int erosion_radius, int mask_border,
                     unsigned char* mask, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!hom_inv || !mask) return fail(h, MP_EINVAL, "mp_ha_valid_mask: NULL tensor");
    if (!count_ok(G) || H <= 0 || W <= 0) return fail(h, MP_EINVAL, "mp_ha_valid_mask: need 0 < G <= 65535, H, W > 0");
    if (erosion_radius < 0 || erosion_radius > 16) return fail(h, MP_EINVAL, "mp_ha_valid_mask: erosion_radius must be in [0, 16]");
    MP_HIP(hipSetDevice(h->device));
    launch_ha_valid_mask(hom_inv, G, H, W, erosion_radius, mask_border != 0, mask, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

static int ha_check(mp_handle* h, const char* fn, const float* pa, const float* pb, int B, int H, int W, int aggregation)
{
    if (!pa || (aggregation != 0 && !pb)) return fail(h, MP_EINVAL, std::string(fn) + ": NULL heat map");
    if (aggregation < 0 || aggregation > 2) return fail(h, MP_EINVAL, std::string(fn) + ": aggregation must be 0 (single), 1 (prod) or 2 (sum)");
    if (!count_ok(B) || H <= 0 || W <= 0) return fail(h, MP_EINVAL, std::string(fn) + ": need 0 < B <= 65535, H, W > 0");
    return MP_OK;
}

int mp_ha_begin(mp_handle* h, const float* prob_a, const float* prob_b, int B, int H, int W, int aggregation,
                float* prob, float* count, void* stream)
{
    if (!h) return MP_EINVAL;
    int rc;
    if ((rc = ha_check(h, "mp_ha_begin", prob_a, prob_b, B, H, W, aggregation))) return rc;
    if (!prob || !count) return fail(h, MP_EINVAL, "mp_ha_begin: NULL tensor");
    MP_HIP(hipSetDevice(h->device));
    launch_ha_begin(prob_a, prob_b, (long long)B * H * W, aggregation, prob, count, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_ha_accumulate(mp_handle* h, const float* prob_a, const float* prob_b, const unsigned char* mask,
                     const double* hom, int G, int B, int H, int W, int aggregation, float* prob, float* count,
                     void* stream)
{
    if (!h) return MP_EINVAL;
    int rc;
    if ((rc = ha_check(h, "mp_ha_accumulate", prob_a, prob_b, B, H, W, aggregation))) return rc;
    if (!mask || !hom || !prob || !count) return fail(h, MP_EINVAL, "mp_ha_accumulate: NULL tensor");
    if (G <= 0) return fail(h, MP_EINVAL, "mp_ha_accumulate: G must be positive");
    MP_HIP(hipSetDevice(h->device));
    launch_ha_accumulate(prob_a, prob_b, mask, hom, G, B, H, W, aggregation, prob, count, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_ha_finalize(mp_handle* h, const float* prob, const float* count, int B, int H, int W, int aggregation,
                   float min_count, float* out, void* stream)
{
    if (!h) return MP_EINVAL;
    int rc;
    if ((rc = ha_check(h, "mp_ha_finalize", prob, count, B, H, W, aggregation))) return rc;
    if (!out) return fail(h, MP_EINVAL, "mp_ha_finalize: NULL tensor");
    MP_HIP(hipSetDevice(h->device));
    launch_ha_finalize(prob, count, (long long)B * H * W, aggregation, min_count, out, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_gaussian_filter(mp_handle* h, const float* in, int B, int H, int W, int ksize, const float* weights, float* out,
                       void* stream)
{
    if (!h) return MP_EINVAL;
    if (!in || !weights || !out) return fail(h, MP_EINVAL, "mp_gaussian_filter: NULL tensor");
    if (in == out) return fail(h, MP_EINVAL, "mp_gaussian_filter: in-place filtering is not supported");
    if (!count_ok(B) || H <= 0 || W <= 0) return fail(h, MP_EINVAL, "mp_gaussian_filter: need 0 < B <= 65535, H, W > 0");
    if (ksize < 1 || ksize > 31 || (ksize & 1) == 0) return fail(h, MP_EINVAL, "mp_gaussian_filter: ksize must be odd and <= 31");
    if ((ksize - 1) / 2 >= H || (ksize - 1) / 2 >= W) return fail(h, MP_EINVAL, "mp_gaussian_filter: reflection padding needs (ksize-1)/2 < H, W");
    MP_HIP(hipSetDevice(h->device));
    launch_gaussian_filter(in, B, H, W, ksize, weights, out, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_loss_workspace_bytes(int B, int H, int W, long long* bytes)
{
    if (!bytes || !count_ok(B) || H <= 0 || W <= 0 || H % 8 || W % 8) return MP_EINVAL;
    *bytes = (long long)loss_workspace_bytes(B, H, W);
    return MP_OK;
}

static int loss_check(mp_handle* h, const char* fn, int B, int Hc, int Wc, int H, int W, void* workspace,
                      long long workspace_bytes)
{
    if (!count_ok(B) || Hc <= 0 || Wc <= 0)
        return fail(h, MP_EINVAL, std::string(fn) + ": need 0 < B <= 65535 and Hc, Wc > 0");
    if (H % 8 || W % 8) return fail(h, MP_EINVAL, std::string(fn) + ": H and W must be multiples of 8");
    if (H != 8 * Hc || W != 8 * Wc)
        return fail(h, MP_EINVAL, std::string(fn) + ": the " + std::to_string(H) + "x" + std::to_string(W) +
                                      " label maps do not match the " + std::to_string(Hc) + "x" + std::to_string(Wc) + " cell grid");
    if ((long long)Hc * Wc > 0x7fffffffLL / 8) return fail(h, MP_EINVAL, std::string(fn) + ": frame too large");
    if (!workspace || workspace_bytes < (long long)loss_workspace_bytes(B, H, W))
        return fail(h, MP_EINVAL, std::string(fn) + ": workspace smaller than mp_loss_workspace_bytes");
    return MP_OK;
}

int mp_detector_loss(mp_handle* h, const float* logits, int B, int Hc, int Wc, const unsigned char* keypoints,
                     const unsigned char* valid_mask, int H, int W, int use_cross_entropy, const float* noise,
                     unsigned long long noise_seed, void* workspace, long long workspace_bytes, double* out, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!logits || !keypoints || !out) return fail(h, MP_EINVAL, "mp_detector_loss: NULL tensor");
    const int rc = loss_check(h, "mp_detector_loss", B, Hc, Wc, H, W, workspace, workspace_bytes);
    if (rc != MP_OK) return rc;
    MP_HIP(hipSetDevice(h->device));
    launch_detector_loss(logits, keypoints, valid_mask, noise, noise_seed, B, H, W, use_cross_entropy != 0, workspace, out,
                         static_cast<hipStream_t>(stream));
    return launch_status(h);
}

// largest float s with sqrt_rn(s) <= thr (sqrt_rn is monotone: dist <= thr  <=>  dy^2 + dx^2 <= s); -1 when no distance is
// <= thr (thr negative or NaN)
static float corr_bound(float thr)
{
    if (!(thr >= 0.f)) return -1.f;
    if (std::isinf(thr)) return thr;
    float s = (float)((double)thr * thr);
    while (s > 0.f && !(std::sqrt(s) <= thr)) s = std::nextafter(s, 0.f);
    while (!std::isinf(s) && std::sqrt(std::nextafter(s, INFINITY)) <= thr) s = std::nextafter(s, INFINITY);
    return s;
}

int mp_descriptor_loss(mp_handle* h, const float* desc1, const float* desc2, int B, int Hc, int Wc, int D,
                       const float* hom1, const float* hom2, const unsigned char* valid1, const unsigned char* valid2,
                       int H, int W, float threshold, float positive_margin, float negative_margin, float lambda_d,
                       int use_mask, void* workspace, long long workspace_bytes, double* out, float* warped,
                       void* stream)
{
    if (!h) return MP_EINVAL;
    if (!desc1 || !desc2 || !out) return fail(h, MP_EINVAL, "mp_descriptor_loss: NULL tensor");
    if (D != 64 && D != 128 && D != 256) return fail(h, MP_EINVAL, "mp_descriptor_loss: D must be 64, 128 or 256");
    const int rc = loss_check(h, "mp_descriptor_loss", B, Hc, Wc, H, W, workspace, workspace_bytes);
    if (rc != MP_OK) return rc;
    MP_HIP(hipSetDevice(h->device));
    launch_descriptor_loss(desc1, desc2, hom1, hom2, valid1, valid2, B, H, W, D, corr_bound(threshold), positive_margin,
                           negative_margin, (double)lambda_d, use_mask != 0, workspace, out, warped,
                           static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_detector_loss_backward(mp_handle* h, const float* logits, int B, int Hc, int Wc, const unsigned char* keypoints,
                              const unsigned char* valid_mask, int H, int W, int use_cross_entropy, const float* noise,
                              unsigned long long noise_seed, const double* forward_out, const double* coef,
                              void* workspace, long long workspace_bytes, float* grad_logits, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!logits || !keypoints || !forward_out || !coef || !grad_logits)
        return fail(h, MP_EINVAL, "mp_detector_loss_backward: NULL tensor");
    const int rc = loss_check(h, "mp_detector_loss_backward", B, Hc, Wc, H, W, workspace, workspace_bytes);
    if (rc != MP_OK) return rc;
    MP_HIP(hipSetDevice(h->device));
    launch_detector_loss_backward(logits, keypoints, valid_mask, noise, noise_seed, B, H, W, use_cross_entropy != 0,
                                  forward_out, coef, grad_logits, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_descriptor_loss_backward(mp_handle* h, const float* desc1, const float* desc2, int B, int Hc, int Wc, int D,
                                const float* hom1, const float* hom2, const unsigned char* valid1,
                                const unsigned char* valid2, int H, int W, float threshold, float positive_margin,
                                float negative_margin, float lambda_d, int use_mask, const double* forward_out,
                                const double* coef, void* workspace, long long workspace_bytes, float* grad1,
                                float* grad2, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!desc1 || !desc2 || !forward_out || !coef || (!grad1 && !grad2))
        return fail(h, MP_EINVAL, "mp_descriptor_loss_backward: NULL tensor");
    if (D != 64 && D != 128 && D != 256) return fail(h, MP_EINVAL, "mp_descriptor_loss_backward: D must be 64, 128 or 256");
    const int rc = loss_check(h, "mp_descriptor_loss_backward", B, Hc, Wc, H, W, workspace, workspace_bytes);
    if (rc != MP_OK) return rc;
    MP_HIP(hipSetDevice(h->device));
    launch_descriptor_loss_backward(desc1, desc2, hom1, hom2, valid1, valid2, B, H, W, D, corr_bound(threshold),
                                    positive_margin, negative_margin, lambda_d, use_mask != 0, forward_out, coef, workspace,
                                    grad1, grad2, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_photometric_workspace_bytes(int n, int H, int W, int n_ellipses, long long* bytes)
{
    if (!bytes || !count_ok(n) || H <= 0 || W <= 0 || n_ellipses < 0 || (long long)n * H * W > (1LL << 34))
        return MP_EINVAL;
    *bytes = (long long)photometric_workspace_bytes(n, H, W, n_ellipses);
    return MP_OK;
}

// the plans' ops, ellipse ranges, kernel sizes and noise planes against the buffers they index
static int photometric_check(mp_handle* h, const char* fn, int n, int H, int W, const mp_photometric_plan* plans,
                             const int* ellipses, int n_ellipses, int n_normal, int n_uniform, void* workspace,
                             long long workspace_bytes)
{
    const std::string f(fn);
    if (!count_ok(n) || H <= 0 || W <= 0 || H > 8192 || (long long)n * H * W > (1LL << 34))
        return fail(h, MP_EINVAL, f + ": need 0 < n <= 65535, 0 < H <= 8192, W > 0");
    if (!plans) return fail(h, MP_EINVAL, f + ": NULL plans");
    if (n_ellipses < 0 || (n_ellipses > 0 && !ellipses)) return fail(h, MP_EINVAL, f + ": bad ellipse table");
    for (int i = 0; i < n; ++i) {
        const mp_photometric_plan& p = plans[i];
        if (p.n_ops < 0 || p.n_ops > MP_PHOTO_MAX_OPS) return fail(h, MP_EINVAL, f + ": n_ops outside 0.." + std::to_string(MP_PHOTO_MAX_OPS));
        for (int s = 0; s < p.n_ops; ++s) {
            const mp_photometric_op& o = p.op[s];
            const std::string at = f + ": plan " + std::to_string(i) + " op " + std::to_string(s);
            switch (o.kind) {
            case MP_PHOTO_GAUSSIAN_NOISE:
            case MP_PHOTO_GAUSSIAN_ADD:
                if (!p.noise_device && (o.field < 0 || o.field >= n_normal)) return fail(h, MP_EINVAL, at + ": normal field out of range");
                break;
            case MP_PHOTO_SPECKLE:
                if (!p.noise_device && (o.field < 0 || o.field >= n_uniform)) return fail(h, MP_EINVAL, at + ": uniform field out of range");
                break;
            case MP_PHOTO_BRIGHTNESS:
            case MP_PHOTO_CONTRAST:
                break;
            case MP_PHOTO_SHADE:
                if (o.ksize < 1 || o.ksize > MP_PHOTO_MAX_BLUR || (o.ksize & 1) == 0)
                    return fail(h, MP_EINVAL, at + ": blur size must be odd and <= " + std::to_string(MP_PHOTO_MAX_BLUR));
                if (o.ellipse_count < 0 || o.ellipse_offset < 0 || (long long)o.ellipse_offset + o.ellipse_count > n_ellipses)
                    return fail(h, MP_EINVAL, at + ": ellipses outside the table");
                break;
            case MP_PHOTO_MOTION_BLUR:
                if (o.ksize < 1 || o.ksize > MP_PHOTO_MAX_TAPS || (o.ksize & 1) == 0 || o.mode < 0 || o.mode > 3)
                    return fail(h, MP_EINVAL, at + ": motion blur needs an odd size <= 11 and mode 0..3");
                break;
            default:
                return fail(h, MP_EINVAL, at + ": unknown primitive " + std::to_string(o.kind));
            }
        }
    }
    if (photometric_lds_bytes(plans, n, H, W) > 65536) return fail(h, MP_EINVAL, f + ": frame too wide for the blur size, or too high for the ellipse spans, to fit the LDS");
    if (!workspace || workspace_bytes < (long long)photometric_workspace_bytes(n, H, W, n_ellipses))
        return fail(h, MP_EINVAL, f + ": workspace smaller than mp_photometric_workspace_bytes");
    return MP_OK;
}

int mp_photometric_augment(mp_handle* h, const float* in, float* out, int n, int H, int W, const mp_photometric_plan* plans,
                           const int* ellipses, int n_ellipses, const double* normal, int n_normal, const double* uniform,
                           int n_uniform, void* workspace, long long workspace_bytes, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!in || !out) return fail(h, MP_EINVAL, "mp_photometric_augment: NULL tensor");
    if (n_normal < 0 || n_uniform < 0 || (n_normal && !normal) || (n_uniform && !uniform))
        return fail(h, MP_EINVAL, "mp_photometric_augment: bad noise fields");
    const int rc = photometric_check(h, "mp_photometric_augment", n, H, W, plans, ellipses, n_ellipses, n_normal, n_uniform,
                                     workspace, workspace_bytes);
    if (rc != MP_OK) return rc;
    MP_HIP(hipSetDevice(h->device));
    launch_photometric(in, out, n, H, W, plans, ellipses, n_ellipses, normal, uniform, workspace,
                       static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_photometric_shade_mask(mp_handle* h, int n, int H, int W, const mp_photometric_plan* plans, const int* ellipses,
                              int n_ellipses, int op_index, int blurred, float* out, void* workspace,
                              long long workspace_bytes, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!out) return fail(h, MP_EINVAL, "mp_photometric_shade_mask: NULL tensor");
    if (op_index < 0 || op_index >= MP_PHOTO_MAX_OPS) return fail(h, MP_EINVAL, "mp_photometric_shade_mask: op_index out of range");
    const int rc = photometric_check(h, "mp_photometric_shade_mask", n, H, W, plans, ellipses, n_ellipses, 1 << 30, 1 << 30,
                                     workspace, workspace_bytes);
    if (rc != MP_OK) return rc;
    MP_HIP(hipSetDevice(h->device));
    launch_photometric_shade_mask(n, H, W, plans, ellipses, n_ellipses, op_index, blurred, out, workspace,
                                  static_cast<hipStream_t>(stream));
    return launch_status(h);
}


}  // extern "C"
