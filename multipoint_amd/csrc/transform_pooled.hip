// One similarity or affine model per GROUP of pairs from their pooled matches (mp_find_transform_pooled,
// mp_refine_transform_pooled): homography_pooled.hip's route with the models of mp_transform.h.  The pooled list is the one
// mp_pool_matches writes (model-free); a group is a contiguous range of it.  Scoring is pooled_score_kernel of mp_ransac.h, the
// homography route's kernel with a thread's 6 coefficients in the place of 9; the winner is selected by that route's kernel
// (launch_pooled_select); the refit and the refinement are the kernel templates of mp_transform.h.
#include "../../include/multipoint_hip.h"
#include "mp_common.h"
#include "mp_device.h"
#include "mp_transform.h"

namespace {

template <class Model>
void find(const float4* p4, const int* group_offsets, int N, int G, int T, double thr, unsigned long long seed, unsigned int* counts,
          unsigned long long* best, double* H_out, unsigned char* mask, int* n_inliers, hipStream_t s)
{
    hipLaunchKernelGGL(pooled_score_kernel<Model>, dim3((T + 255) / 256, pool_splits(N), G), dim3(256), 0, s, p4, group_offsets, N,
                       T, thr, seed, counts);
    launch_pooled_select(counts, T, G, best, s);
    hipLaunchKernelGGL((transform_refit_kernel<Model, PooledSource>), dim3(G), dim3(256), 0, s,
                       PooledSource{p4, group_offsets, N, mask}, thr, seed, best, H_out, n_inliers);
}

}  // namespace

void launch_find_transform_pooled(int model, const float* pts, const int* group_offsets, int N, int G, int T, double thr,
                                  unsigned long long seed, unsigned int* counts, unsigned long long* best, double* H_out,
                                  unsigned char* mask, int* n_inliers, hipStream_t s)
{
    const float4* p4 = reinterpret_cast<const float4*>(pts);
    if (model == MP_MODEL_SIMILARITY) find<Similarity>(p4, group_offsets, N, G, T, thr, seed, counts, best, H_out, mask, n_inliers, s);
    else find<Affine>(p4, group_offsets, N, G, T, thr, seed, counts, best, H_out, mask, n_inliers, s);
}

void launch_refine_transform_pooled(int model, const float* pts, const int* group_offsets, int N, int G, double thr, int rounds,
                                    double* H_io, unsigned char* mask, int* n_inliers, double* cost, hipStream_t s)
{
    const PooledSource src{reinterpret_cast<const float4*>(pts), group_offsets, N, mask};
    if (model == MP_MODEL_SIMILARITY)
        hipLaunchKernelGGL((transform_refine_kernel<Similarity, PooledSource>), dim3(G), dim3(256), 0, s, src, thr, rounds, H_io,
                           n_inliers, cost);
    else
        hipLaunchKernelGGL((transform_refine_kernel<Affine, PooledSource>), dim3(G), dim3(256), 0, s, src, thr, rounds, H_io,
                           n_inliers, cost);
}
