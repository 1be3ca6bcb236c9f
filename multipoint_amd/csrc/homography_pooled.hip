// One homography per GROUP of pairs from their pooled matches (mp_pool_matches, mp_find_homography_pooled,
// mp_refine_homography_pooled): the estimator for a rig whose optical -> thermal transform is the same for a whole recording,
// where a single cross-spectral pair has too few good matches and many pairs together have thousands.
// The algorithm is the one homography.hip documents, with the group index in the place of the pair index: counter-based
// sampling sample_distinct<4>(seed, g, t, n_g), exact 4-point solve, forward reprojection test, most inliers wins (lowest
// hypothesis index on ties), normalised-DLT refit, Levenberg-Marquardt polish.  The refit and the polish are the kernel
// templates of mp_homography.h that the per-pair route launches too; what differs is the point view they are given.  The
// per-pair route keeps a pair's list in LDS (at most 3200, PairView); here the lists of all pairs are compacted once into
// global memory,
//   pts [N][4] fp32 (x, y, u, v), pair-major, query order inside a pair (compact_matches, as for the per-pair list),
// and a group is a contiguous range of it (group_offsets [G + 1], PooledView).  Scoring, the only step whose cost grows as
// T x N, runs on a grid of hypothesis blocks x point splits x groups (pooled_score_kernel, mp_ransac.h, which the similarity /
// affine route launches too): a thread owns one hypothesis (its 9 coefficients in registers), the group's points pass through
// LDS in chunks of POOL_CHUNK that every lane reads at the same address (a broadcast), and the splits' partial counts are added
// with integer atomics -- order-independent, so every run gives the same bits.
#include "mp_common.h"
#include "mp_device.h"
#include "mp_homography.h"

namespace {

// a pair's number of usable matches (usable_match: the filter of the ordered compaction)
__global__ __launch_bounds__(256) void pool_count_kernel(const int* __restrict__ kp_count, const int* __restrict__ match_idx, int K,
                                                         int* __restrict__ pair_cnt)
{
    __shared__ int wave_cnt[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int no = min(kp_count[2 * p], K), nt = min(kp_count[2 * p + 1], K);
    int c = 0;
    for (int i = tid; i < no; i += 256)
        c += usable_match(match_idx, p, K, i, no, nt) >= 0 ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((tid & 63) == 0) wave_cnt[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) pair_cnt[p] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// one workgroup: pair_offsets = exclusive prefix sum of pair_cnt (pair_offsets[P] = N), then group_offsets[g] = the offset of
// the first pair whose group id is >= g (ids non-decreasing: a binary search; groups == NULL: one group)
__global__ __launch_bounds__(256) void pool_scan_kernel(const int* __restrict__ pair_cnt, const int* __restrict__ groups, int P, int G,
                                                        int* __restrict__ pair_offsets, int* __restrict__ group_offsets)
{
    __shared__ int sh[256];
    __shared__ int carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int p0 = 0; p0 < P; p0 += 256) {
        const int p = p0 + tid;
        const int c = p < P ? pair_cnt[p] : 0;
        sh[tid] = c;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int v = tid >= off ? sh[tid - off] : 0;
            __syncthreads();
            sh[tid] += v;
            __syncthreads();
        }
        if (p < P) pair_offsets[p] = carry + sh[tid] - c;
        __syncthreads();
        if (tid == 255) carry += sh[255];
        __syncthreads();
    }
    if (tid == 0) pair_offsets[P] = carry;
    __syncthreads();                       // (the offsets above are read below by other threads of this workgroup)
    const int total = carry;
    for (int g = tid; g <= G; g += 256) {
        int first = P;                     // first pair with groups[pair] >= g
        if (!groups) first = g == 0 ? 0 : P;
        else {
            int lo = 0, hi = P;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (groups[mid] >= g) hi = mid; else lo = mid + 1;
            }
            first = lo;
        }
        group_offsets[g] = first < P ? pair_offsets[first] : total;
    }
}

// one workgroup per pair: its usable matches in query order to pts / query_index from row pair_offsets[p] on.  Rows at or
// beyond `capacity` are not written.
template <class KP>
__global__ __launch_bounds__(256) void pool_write_kernel(const KP* __restrict__ kp_yx, const int* __restrict__ kp_count,
                                                         const int* __restrict__ match_idx, int K,
                                                         const int* __restrict__ pair_offsets, long long capacity,
                                                         float4* __restrict__ pts, int* __restrict__ query_index)
{
    const int p = blockIdx.x;
    const long long base = pair_offsets[p];
    compact_matches(kp_count, match_idx, p, K, [&](int at, int i, int j) {
        const long long pos = base + at;
        if (pos < capacity) {
            pts[pos] = match_point(kp_yx, p, K, i, j);
            query_index[pos] = i;
        }
    });
}

// best[g] = max over t of (count << 32) | (0x7fffffff - t): most inliers, then the LOWEST hypothesis index
__global__ __launch_bounds__(256) void pooled_select_kernel(const unsigned int* __restrict__ counts, int T,
                                                            unsigned long long* __restrict__ best)
{
    __shared__ unsigned long long wave_best[4];
    const int g = blockIdx.x, tid = threadIdx.x;
    unsigned long long b = 0;
    for (int t = tid; t < T; t += 256) {
        const unsigned long long key = ((unsigned long long)counts[(size_t)g * T + t] << 32) | (unsigned long long)(0x7fffffff - t);
        b = key > b ? key : b;
    }
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(b, off); b = o > b ? o : b; }
    if ((tid & 63) == 0) wave_best[tid >> 6] = b;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) b = wave_best[w] > b ? wave_best[w] : b;
        best[g] = b;
    }
}

}  // namespace

template <class KP>
void launch_pool_matches(const KP* kp_yx, const int* kp_count, const int* match_idx, const int* groups, int P, int K, int G,
                         float* pts, int* query_index, long long capacity, int* pair_offsets, int* group_offsets, int* pair_cnt,
                         hipStream_t s)
{
    hipLaunchKernelGGL(pool_count_kernel, dim3(P), dim3(256), 0, s, kp_count, match_idx, K, pair_cnt);
    hipLaunchKernelGGL(pool_scan_kernel, dim3(1), dim3(256), 0, s, pair_cnt, groups, P, G, pair_offsets, group_offsets);
    hipLaunchKernelGGL(pool_write_kernel<KP>, dim3(P), dim3(256), 0, s, kp_yx, kp_count, match_idx, K, pair_offsets, capacity,
                       reinterpret_cast<float4*>(pts), query_index);
}

template void launch_pool_matches<int>(const int*, const int*, const int*, const int*, int, int, int, float*, int*, long long, int*, int*,
                                       int*, hipStream_t);
template void launch_pool_matches<float>(const float*, const int*, const int*, const int*, int, int, int, float*, int*, long long, int*,
                                         int*, int*, hipStream_t);

void launch_find_homography_pooled(const float* pts, const int* group_offsets, int N, int G, int T, double thr,
                                   unsigned long long seed, unsigned int* counts, unsigned long long* best, double* H_out,
                                   unsigned char* mask, int* n_inliers, hipStream_t s)
{
    const float4* p4 = reinterpret_cast<const float4*>(pts);
    hipLaunchKernelGGL(pooled_score_kernel<Homography>, dim3((T + 255) / 256, pool_splits(N), G), dim3(256), 0, s, p4, group_offsets, N, T, thr, seed,
                       counts);
    hipLaunchKernelGGL(pooled_select_kernel, dim3(G), dim3(256), 0, s, counts, T, best);
    hipLaunchKernelGGL(refit_kernel<PooledSource>, dim3(G), dim3(256), 0, s, PooledSource{p4, group_offsets, N, mask}, thr, seed, best,
                       H_out, n_inliers);
}

// the winner selection on its own, for the other motion models' pooled route (transform_pooled.hip): counts is model-free
void launch_pooled_select(const unsigned int* counts, int T, int G, unsigned long long* best, hipStream_t s)
{
    hipLaunchKernelGGL(pooled_select_kernel, dim3(G), dim3(256), 0, s, counts, T, best);
}

void launch_refine_homography_pooled(const float* pts, const int* group_offsets, int N, int G, double thr, int iters, double* H_io,
                                     unsigned char* mask, int* n_inliers, double* cost, hipStream_t s)
{
    hipLaunchKernelGGL(refine_kernel<PooledSource>, dim3(G), dim3(256), 0, s,
                       PooledSource{reinterpret_cast<const float4*>(pts), group_offsets, N, mask}, thr, iters, H_io, n_inliers, cost);
}
