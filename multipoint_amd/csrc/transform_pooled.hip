// One similarity or affine model per GROUP of pairs from their pooled matches (mp_find_transform_pooled,
// mp_refine_transform_pooled): homography_pooled.hip's route with the models of mp_transform.h.  The pooled list is the one
// mp_pool_matches writes (model-free); a group is a contiguous range of it.  Scoring runs on a grid of hypothesis blocks x
// point splits x groups: a thread owns one hypothesis (its 6 coefficients in registers), the group's points pass through LDS
// in chunks of POOL_CHUNK that every lane reads at the same address (a broadcast), and the splits' partial counts are added
// with integer atomics -- order-independent, so every run gives the same bits.  The winner is selected by the homography
// route's kernel (launch_pooled_select); the refit and the refinement are the kernel templates of mp_transform.h.
#include "../../include/multipoint_hip.h"
#include "mp_common.h"
#include "mp_device.h"
#include "mp_transform.h"

namespace {

constexpr int POOL_CHUNK = MP_POOLED_CHUNK;            // points per staged chunk: 16 KB of LDS
constexpr int POOL_MAX_SPLITS = MP_POOLED_MAX_SPLITS;  // most blocks that share the points of one (hypothesis block, group)

// grid (hypothesis blocks, point splits, groups).  Block (bx, s, g) scores hypotheses bx * 256 .. + 255 of group g on the
// chunks s, s + splits, ... of its points and adds the counts to counts[g][t].  A thread without a hypothesis (t >= T, or a
// degenerate sample) still takes part in every staging barrier: the only early exits are the same for the whole workgroup.
template <class Model>
__global__ __launch_bounds__(256) void transform_pooled_score_kernel(const float4* __restrict__ pts,
                                                                     const int* __restrict__ group_offsets, int N, int T,
                                                                     double thr, unsigned long long seed,
                                                                     unsigned int* __restrict__ counts)
{
    __shared__ float4 chunk[POOL_CHUNK];
    const int g = blockIdx.z, tid = threadIdx.x;
    int start;
    const int n = group_range(group_offsets, g, N, start);
    if (n < Model::S) return;                                // (the sampling needs S points; the whole workgroup leaves)
    const int nchunks = (n + POOL_CHUNK - 1) / POOL_CHUNK;
    if ((int)blockIdx.y >= nchunks) return;                  // (no chunk for this split; the whole workgroup leaves)
    pts += start;
    const int t = blockIdx.x * 256 + tid;
    double m[6];
    bool ok = t < T;
    if (ok) ok = transform_hypothesis<Model>(PooledView{pts, nullptr, n}, seed, g, t, m);
    const double thr2 = thr * thr;
    int cnt = 0;
    for (int c = blockIdx.y; c < nchunks; c += gridDim.y) {
        const int base = c * POOL_CHUNK, len = min(POOL_CHUNK, n - base);
        __syncthreads();                                     // the previous chunk has been read by every thread
        for (int i = tid; i < len; i += 256) chunk[i] = pts[base + i];
        __syncthreads();
        if (ok)
            for (int i = 0; i < len; ++i) {
                const float4 q = chunk[i];
                cnt += error2(m, q.x, q.y, q.z, q.w) <= thr2;
            }
    }
    if (ok && cnt > 0) atomicAdd(&counts[(size_t)g * T + t], (unsigned int)cnt);
}

template <class Model>
void find(const float4* p4, const int* group_offsets, int N, int G, int T, double thr, unsigned long long seed, unsigned int* counts,
          unsigned long long* best, double* H_out, unsigned char* mask, int* n_inliers, hipStream_t s)
{
    const int splits = min(max((N + POOL_CHUNK - 1) / POOL_CHUNK, 1), POOL_MAX_SPLITS);
    hipLaunchKernelGGL(transform_pooled_score_kernel<Model>, dim3((T + 255) / 256, splits, G), dim3(256), 0, s, p4, group_offsets, N,
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
