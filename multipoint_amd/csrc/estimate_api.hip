// C ABI of the RANSAC estimators: one model per pair (mp_find_* / mp_refine_*, on int keypoints or, with _f, float ones) and one
// per group of pairs from their pooled matches (mp_pool_matches, mp_*_pooled).  An estimate is one of four checked bodies -- pair
// find, pair refine, pooled find, pooled refine -- that validates, prepares the buffers and only then chooses the model's
// launcher: the homography's (homography*.hip) or the similarity / affine ones (transform*.hip).  The mp_*_homography* entries
// are those bodies at MP_MODEL_HOMOGRAPHY.
#include "host.h"

#include <algorithm>

using namespace mp_host;

namespace {

bool transform_model_known(int model)
{
    return model == MP_MODEL_HOMOGRAPHY || model == MP_MODEL_SIMILARITY || model == MP_MODEL_AFFINE;
}

// the checks the four per-pair entries share, after the handle's; fn: the entry's name
template <class KP>
int pair_check(mp_handle* h, const std::string& fn, int model, const KP* kp_yx, const int* kp_count, const int* match_idx, int P, int K,
               const double* transform, const unsigned char* inlier_mask, const int* n_inliers)
{
    if (!transform_model_known(model)) return fail(h, MP_EINVAL, fn + ": unknown model " + std::to_string(model));
    if (!kp_yx || !kp_count || !match_idx || !transform || !inlier_mask || !n_inliers)
        return fail(h, MP_EINVAL, fn + ": NULL tensor");
    if (P <= 0 || K <= 0 || K > 3200) return fail(h, MP_EINVAL, fn + ": need P > 0 and 0 < K <= 3200");
    return MP_OK;
}

// mp_find_homography{,_f}, mp_find_transform{,_f}
template <class KP>
int pair_find(mp_handle* h, const std::string& fn, int model, const KP* kp_yx, const int* kp_count, const int* match_idx, int P, int K,
              double reproj_threshold, int max_iters, unsigned long long seed, double* transform, unsigned char* inlier_mask,
              int* n_inliers, void* stream)
{
    if (!h) return MP_EINVAL;
    int rc;
    if ((rc = pair_check(h, fn, model, kp_yx, kp_count, match_idx, P, K, transform, inlier_mask, n_inliers))) return rc;
    if (max_iters <= 0 || max_iters > (1 << 20)) return fail(h, MP_EINVAL, fn + ": max_iters must be in [1, 2^20]");
    if (!(reproj_threshold > 0.0)) return fail(h, MP_EINVAL, fn + ": threshold must be positive");
    hipStream_t s = static_cast<hipStream_t>(stream);
    MP_HIP(hipSetDevice(h->device));
    if ((rc = ensure(h, h->metrics_ws, (size_t)P * sizeof(unsigned long long)))) return rc;
    unsigned long long* best = static_cast<unsigned long long*>(h->metrics_ws.p);
    MP_HIP(hipMemsetAsync(best, 0, (size_t)P * sizeof(unsigned long long), s));
    MP_HIP(hipMemsetAsync(inlier_mask, 0, (size_t)P * K, s));
    if (model == MP_MODEL_HOMOGRAPHY)
        launch_ransac_homography(kp_yx, kp_count, match_idx, P, K, max_iters, reproj_threshold, seed, best, transform, inlier_mask,
                                 n_inliers, s);
    else
        launch_find_transform(model, kp_yx, kp_count, match_idx, P, K, max_iters, reproj_threshold, seed, best, transform,
                              inlier_mask, n_inliers, s);
    return launch_status(h);
}

// mp_refine_homography{,_f}, mp_refine_transform{,_f}; count: what the entry calls its count argument (iters / rounds)
template <class KP>
int pair_refine(mp_handle* h, const std::string& fn, int model, const char* count, const KP* kp_yx, const int* kp_count,
                const int* match_idx, int P, int K, double reproj_threshold, int rounds, double* transform,
                unsigned char* inlier_mask, int* n_inliers, double* cost, void* stream)
{
    if (!h) return MP_EINVAL;
    int rc;
    if ((rc = pair_check(h, fn, model, kp_yx, kp_count, match_idx, P, K, transform, inlier_mask, n_inliers))) return rc;
    if (rounds < 0 || rounds > 1000) return fail(h, MP_EINVAL, fn + ": " + count + " must be in [0, 1000]");
    if (!(reproj_threshold > 0.0)) return fail(h, MP_EINVAL, fn + ": threshold must be positive");
    hipStream_t s = static_cast<hipStream_t>(stream);
    MP_HIP(hipSetDevice(h->device));
    MP_HIP(hipMemsetAsync(inlier_mask, 0, (size_t)P * K, s));
    if (model == MP_MODEL_HOMOGRAPHY)
        launch_refine_homography(kp_yx, kp_count, match_idx, P, K, reproj_threshold, rounds, transform, inlier_mask, n_inliers, cost,
                                 s);
    else
        launch_refine_transform(model, kp_yx, kp_count, match_idx, P, K, reproj_threshold, rounds, transform, inlier_mask, n_inliers,
                                cost, s);
    return launch_status(h);
}

// ---- pooled: one model per group of pairs (homography_pooled.hip, transform_pooled.hip) ----
constexpr long long POOLED_MAX_N = 1ll << 24;

// the workspace is scratch without state between calls: pooling uses pair_cnt [P] int, the estimate counts [G][T] uint32 |
// best [G] uint64 (16-byte aligned), both from its start
// the pooled RANSAC's inlier counts of T hypotheses per group, and behind them (on a multiple of 16 bytes) each group's best
struct PooledFindWorkspace { unsigned int* counts; unsigned long long* best; size_t bytes; };
PooledFindWorkspace pooled_find_workspace(void* base, int G, int T)
{
    Carver c(base, 16);
    PooledFindWorkspace w{};
    w.counts = c.take<unsigned int>((size_t)G * T);
    c.align = alignof(unsigned long long);
    w.best = c.take<unsigned long long>(G);
    w.bytes = c.bytes();
    return w;
}
size_t pooled_pool_bytes(int P) { return (size_t)P * sizeof(int); }

// the checks the four pooled entries share, after the handle's
int pooled_check(mp_handle* h, const std::string& fn, int model, const float* pts, const int* group_offsets, long long N, int G,
                 double reproj_threshold, const double* transform, const unsigned char* inlier_mask, const int* n_inliers)
{
    if (!transform_model_known(model)) return fail(h, MP_EINVAL, fn + ": unknown model " + std::to_string(model));
    if (!group_offsets || !transform || !n_inliers) return fail(h, MP_EINVAL, fn + ": NULL tensor");
    if (N < 0 || N >= POOLED_MAX_N) return fail(h, MP_EINVAL, fn + ": need 0 <= N < 2^24 correspondences per call");
    if (N > 0 && (!pts || !inlier_mask)) return fail(h, MP_EINVAL, fn + ": NULL tensor");
    if ((reinterpret_cast<uintptr_t>(pts) & 15) != 0) return fail(h, MP_EINVAL, fn + ": pts must be 16-byte aligned");
    if (!count_ok(G)) return fail(h, MP_EINVAL, fn + ": need 0 < G <= 65535 groups");
    if (!(reproj_threshold > 0.0)) return fail(h, MP_EINVAL, fn + ": threshold must be positive");
    return MP_OK;
}

// mp_find_homography_pooled, mp_find_transform_pooled
int pooled_find(mp_handle* h, const std::string& fn, int model, const float* pts, const int* group_offsets, long long N, int G,
                double reproj_threshold, int max_iters, unsigned long long seed, double* transform, unsigned char* inlier_mask,
                int* n_inliers, void* workspace, long long workspace_bytes, void* stream)
{
    if (!h) return MP_EINVAL;
    const int rc = pooled_check(h, fn, model, pts, group_offsets, N, G, reproj_threshold, transform, inlier_mask, n_inliers);
    if (rc) return rc;
    if (max_iters <= 0 || max_iters > (1 << 20)) return fail(h, MP_EINVAL, fn + ": max_iters must be in [1, 2^20]");
    const PooledFindWorkspace w = pooled_find_workspace(workspace, G, max_iters);
    if (!workspace || workspace_bytes < (long long)w.bytes)
        return fail(h, MP_EINVAL, fn + ": workspace smaller than mp_pooled_workspace_bytes");
    hipStream_t s = static_cast<hipStream_t>(stream);
    MP_HIP(hipSetDevice(h->device));
    MP_HIP(hipMemsetAsync(w.counts, 0, (size_t)G * max_iters * sizeof(unsigned int), s));
    if (N > 0) MP_HIP(hipMemsetAsync(inlier_mask, 0, (size_t)N, s));
    if (model == MP_MODEL_HOMOGRAPHY)
        launch_find_homography_pooled(pts, group_offsets, (int)N, G, max_iters, reproj_threshold, seed, w.counts, w.best, transform,
                                      inlier_mask, n_inliers, s);
    else
        launch_find_transform_pooled(model, pts, group_offsets, (int)N, G, max_iters, reproj_threshold, seed, w.counts, w.best, transform,
                                     inlier_mask, n_inliers, s);
    return launch_status(h);
}

// mp_refine_homography_pooled, mp_refine_transform_pooled; count: as for pair_refine
int pooled_refine(mp_handle* h, const std::string& fn, int model, const char* count, const float* pts, const int* group_offsets,
                  long long N, int G, double reproj_threshold, int rounds, double* transform, unsigned char* inlier_mask,
                  int* n_inliers, double* cost, void* stream)
{
    if (!h) return MP_EINVAL;
    const int rc = pooled_check(h, fn, model, pts, group_offsets, N, G, reproj_threshold, transform, inlier_mask, n_inliers);
    if (rc) return rc;
    if (rounds < 0 || rounds > 1000) return fail(h, MP_EINVAL, fn + ": " + count + " must be in [0, 1000]");
    hipStream_t s = static_cast<hipStream_t>(stream);
    MP_HIP(hipSetDevice(h->device));
    if (N > 0) MP_HIP(hipMemsetAsync(inlier_mask, 0, (size_t)N, s));
    if (model == MP_MODEL_HOMOGRAPHY)
        launch_refine_homography_pooled(pts, group_offsets, (int)N, G, reproj_threshold, rounds, transform, inlier_mask, n_inliers,
                                        cost, s);
    else
        launch_refine_transform_pooled(model, pts, group_offsets, (int)N, G, reproj_threshold, rounds, transform, inlier_mask,
                                       n_inliers, cost, s);
    return launch_status(h);
}

// mp_pool_matches / mp_pool_matches_f
template <class KP>
int pool_matches(mp_handle* h, const std::string& fn, const KP* kp_yx, const int* kp_count, const int* match_idx,
                 const int* groups, int P, int K, int G, float* pts, int* query_index, long long capacity, int* pair_offsets,
                 int* group_offsets, void* workspace, long long workspace_bytes, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!kp_yx || !kp_count || !match_idx || !pair_offsets || !group_offsets)
        return fail(h, MP_EINVAL, fn + ": NULL tensor");
    if (P <= 0 || K <= 0 || (long long)P * K > 0x7fffffffLL) return fail(h, MP_EINVAL, fn + ": need P > 0, K > 0 and P * K < 2^31");
    if (!count_ok(G)) return fail(h, MP_EINVAL, fn + ": need 0 < G <= 65535 groups");
    if (!groups && G != 1) return fail(h, MP_EINVAL, fn + ": without group ids there is one group (G = 1)");
    if (capacity < 0 || (capacity > 0 && (!pts || !query_index))) return fail(h, MP_EINVAL, fn + ": NULL tensor");
    if ((reinterpret_cast<uintptr_t>(pts) & 15) != 0) return fail(h, MP_EINVAL, fn + ": pts must be 16-byte aligned");
    if (!workspace || workspace_bytes < (long long)pooled_pool_bytes(P))
        return fail(h, MP_EINVAL, fn + ": workspace smaller than mp_pooled_workspace_bytes");
    hipStream_t s = static_cast<hipStream_t>(stream);
    MP_HIP(hipSetDevice(h->device));
    launch_pool_matches(kp_yx, kp_count, match_idx, groups, P, K, G, pts, query_index, capacity, pair_offsets, group_offsets,
                        static_cast<int*>(workspace), s);
    return launch_status(h);
}

}  // namespace

extern "C" {

int mp_find_homography(mp_handle* h, const int* kp_yx, const int* kp_count, const int* match_idx, int P, int K,
                       double reproj_threshold, int max_iters, unsigned long long seed, double* homography,
                       unsigned char* inlier_mask, int* n_inliers, void* stream)
{
    return pair_find(h, "mp_find_homography", MP_MODEL_HOMOGRAPHY, kp_yx, kp_count, match_idx, P, K, reproj_threshold, max_iters,
                     seed, homography, inlier_mask, n_inliers, stream);
}

int mp_find_homography_f(mp_handle* h, const float* kp_sub_yx, const int* kp_count, const int* match_idx, int P, int K,
                         double reproj_threshold, int max_iters, unsigned long long seed, double* homography,
                         unsigned char* inlier_mask, int* n_inliers, void* stream)
{
    return pair_find(h, "mp_find_homography_f", MP_MODEL_HOMOGRAPHY, kp_sub_yx, kp_count, match_idx, P, K, reproj_threshold,
                     max_iters, seed, homography, inlier_mask, n_inliers, stream);
}

int mp_find_transform(mp_handle* h, const int* kp_yx, const int* kp_count, const int* match_idx, int P, int K, int model,
                      double reproj_threshold, int max_iters, unsigned long long seed, double* transform,
                      unsigned char* inlier_mask, int* n_inliers, void* stream)
{
    return pair_find(h, "mp_find_transform", model, kp_yx, kp_count, match_idx, P, K, reproj_threshold, max_iters, seed, transform,
                     inlier_mask, n_inliers, stream);
}

int mp_find_transform_f(mp_handle* h, const float* kp_sub_yx, const int* kp_count, const int* match_idx, int P, int K, int model,
                        double reproj_threshold, int max_iters, unsigned long long seed, double* transform,
                        unsigned char* inlier_mask, int* n_inliers, void* stream)
{
    return pair_find(h, "mp_find_transform_f", model, kp_sub_yx, kp_count, match_idx, P, K, reproj_threshold, max_iters, seed,
                     transform, inlier_mask, n_inliers, stream);
}

int mp_refine_homography(mp_handle* h, const int* kp_yx, const int* kp_count, const int* match_idx, int P, int K,
                         double reproj_threshold, int iters, double* homography, unsigned char* inlier_mask, int* n_inliers,
                         double* cost, void* stream)
{
    return pair_refine(h, "mp_refine_homography", MP_MODEL_HOMOGRAPHY, "iters", kp_yx, kp_count, match_idx, P, K, reproj_threshold,
                       iters, homography, inlier_mask, n_inliers, cost, stream);
}

int mp_refine_homography_f(mp_handle* h, const float* kp_sub_yx, const int* kp_count, const int* match_idx, int P, int K,
                           double reproj_threshold, int iters, double* homography, unsigned char* inlier_mask, int* n_inliers,
                           double* cost, void* stream)
{
    return pair_refine(h, "mp_refine_homography_f", MP_MODEL_HOMOGRAPHY, "iters", kp_sub_yx, kp_count, match_idx, P, K,
                       reproj_threshold, iters, homography, inlier_mask, n_inliers, cost, stream);
}

int mp_refine_transform(mp_handle* h, const int* kp_yx, const int* kp_count, const int* match_idx, int P, int K, int model,
                        double reproj_threshold, int rounds, double* transform, unsigned char* inlier_mask, int* n_inliers,
                        double* cost, void* stream)
{
    return pair_refine(h, "mp_refine_transform", model, "rounds", kp_yx, kp_count, match_idx, P, K, reproj_threshold, rounds,
                       transform, inlier_mask, n_inliers, cost, stream);
}

int mp_refine_transform_f(mp_handle* h, const float* kp_sub_yx, const int* kp_count, const int* match_idx, int P, int K, int model,
                          double reproj_threshold, int rounds, double* transform, unsigned char* inlier_mask, int* n_inliers,
                          double* cost, void* stream)
{
    return pair_refine(h, "mp_refine_transform_f", model, "rounds", kp_sub_yx, kp_count, match_idx, P, K, reproj_threshold, rounds,
                       transform, inlier_mask, n_inliers, cost, stream);
}

int mp_pooled_chunk(int* chunk_points, int* max_splits)
{
    if (!chunk_points || !max_splits) return MP_EINVAL;
    *chunk_points = MP_POOLED_CHUNK;
    *max_splits = MP_POOLED_MAX_SPLITS;
    return MP_OK;
}

int mp_pooled_workspace_bytes(int P, int G, int max_iters, long long* bytes)
{
    if (!bytes || P < 0 || !count_ok(G) || max_iters <= 0 || max_iters > (1 << 20)) return MP_EINVAL;
    *bytes = (long long)std::max(pooled_pool_bytes(P), pooled_find_workspace(nullptr, G, max_iters).bytes);
    return MP_OK;
}

int mp_pool_matches(mp_handle* h, const int* kp_yx, const int* kp_count, const int* match_idx, const int* groups, int P, int K,
                    int G, float* pts, int* query_index, long long capacity, int* pair_offsets, int* group_offsets,
                    void* workspace, long long workspace_bytes, void* stream)
{
    return pool_matches(h, "mp_pool_matches", kp_yx, kp_count, match_idx, groups, P, K, G, pts, query_index, capacity, pair_offsets,
                        group_offsets, workspace, workspace_bytes, stream);
}

int mp_pool_matches_f(mp_handle* h, const float* kp_sub_yx, const int* kp_count, const int* match_idx, const int* groups, int P, int K,
                      int G, float* pts, int* query_index, long long capacity, int* pair_offsets, int* group_offsets,
                      void* workspace, long long workspace_bytes, void* stream)
{
    return pool_matches(h, "mp_pool_matches_f", kp_sub_yx, kp_count, match_idx, groups, P, K, G, pts, query_index, capacity,
                        pair_offsets, group_offsets, workspace, workspace_bytes, stream);
}

int mp_find_homography_pooled(mp_handle* h, const float* pts, const int* group_offsets, long long N, int G,
                              double reproj_threshold, int max_iters, unsigned long long seed, double* homography,
                              unsigned char* inlier_mask, int* n_inliers, void* workspace, long long workspace_bytes, void* stream)
{
    return pooled_find(h, "mp_find_homography_pooled", MP_MODEL_HOMOGRAPHY, pts, group_offsets, N, G, reproj_threshold, max_iters,
                       seed, homography, inlier_mask, n_inliers, workspace, workspace_bytes, stream);
}

int mp_find_transform_pooled(mp_handle* h, const float* pts, const int* group_offsets, long long N, int G, int model,
                             double reproj_threshold, int max_iters, unsigned long long seed, double* transform,
                             unsigned char* inlier_mask, int* n_inliers, void* workspace, long long workspace_bytes, void* stream)
{
    return pooled_find(h, "mp_find_transform_pooled", model, pts, group_offsets, N, G, reproj_threshold, max_iters, seed, transform,
                       inlier_mask, n_inliers, workspace, workspace_bytes, stream);
}

int mp_refine_homography_pooled(mp_handle* h, const float* pts, const int* group_offsets, long long N, int G,
                                double reproj_threshold, int iters, double* homography, unsigned char* inlier_mask, int* n_inliers,
                                double* cost, void* stream)
{
    return pooled_refine(h, "mp_refine_homography_pooled", MP_MODEL_HOMOGRAPHY, "iters", pts, group_offsets, N, G, reproj_threshold,
                         iters, homography, inlier_mask, n_inliers, cost, stream);
}

int mp_refine_transform_pooled(mp_handle* h, const float* pts, const int* group_offsets, long long N, int G, int model,
                               double reproj_threshold, int rounds, double* transform, unsigned char* inlier_mask, int* n_inliers,
                               double* cost, void* stream)
{
    return pooled_refine(h, "mp_refine_transform_pooled", model, "rounds", pts, group_offsets, N, G, reproj_threshold, rounds,
                         transform, inlier_mask, n_inliers, cost, stream);
}

}  // extern "C"
