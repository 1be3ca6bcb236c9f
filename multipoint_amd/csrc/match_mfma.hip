// Matching of unit descriptors on MFMA distance tiles, P pairs per launch: mutual nearest neighbours and the one-directional
// modes.  The tile walk both share is mp_match.h.
//
// mutual   : NNMatcher.match (reference multipoint/utils/matching.py:41-72), which is also how
//     cv2.BFMatcher(NORM_L2, crossCheck=True) (matching.py:7,31) is restated for unit descriptors:
//         dmat = sqrt(2 - 2 * clip(d1 . d2^T, -1, 1)); idx = argmin(axis=1); idx2 = argmin(axis=0)
//         keep (i, idx[i]) iff idx2[idx[i]] == i [and dmat < threshold]; lowest index wins ties.
//     The N x M similarity tiles are computed on v_mfma_f32_32x32x2_f32 (exact fp32); the distance
//     and a packed (distance bits << 32 | index) running arg-min are fused behind the MFMAs, so
//     the matrix never exists in memory.  Each direction (rows of A against B, rows of B against A)
//     is one pass; a*b is commutative and both passes add the products in the same k order, so the
//     two passes see bit-identical distances and the mutual test is exact.
// nearest  : the nearest train row of every query row (cv2.BFMatcher(cv2.NORM_L2).match() without crossCheck,
//     matching.py:7,31) and the two nearest plus Lowe's ratio test (knnMatch(d1, d2, 2), matching.py:20-27): ONE
//     direction of the same walk with TWO running keys per lane (OpenCV inserts a candidate only if it is strictly
//     closer: exact distance ties go to the lower train index first).
#include "mp_match.h"

namespace {

// best2[x] = the two smallest (dist(x,y) bits << 32 | y) over the share's rows y of B, for every row x of A.
// grid: (row-block groups, pairs, column shares)
template <int D>
__global__ __launch_bounds__(256) void near2_rows_kernel(const float* __restrict__ dA, const int* __restrict__ nA,
                                                        const float* __restrict__ dB, const int* __restrict__ nB,
                                                        long long pair_stride, int count_stride, int K,
                                                        unsigned long long* __restrict__ best2,
                                                        int* __restrict__ match_count, int nsplit)
{
    // (the pair's match counter, which nearest_kernel adds to behind this launch, is zeroed here)
    if (blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x == 0) match_count[blockIdx.y] = 0;
    const int p = blockIdx.y, share = blockIdx.z;
    const float* X = dA + (long long)p * pair_stride;
    const float* Y = dB + (long long)p * pair_stride;
    const int nx = min(nA[p * count_stride], K);
    const int ny = min(nB[p * count_stride], K);
    unsigned long long* best = best2 + (((long long)share * gridDim.y + p) * K) * 2;
    const ColumnShare cs = column_share(ny, share, nsplit);
    if ((int)blockIdx.x * 128 >= nx) return;             // (the whole workgroup)
    const int lane = threadIdx.x & 63, li = lane & 31, half = lane >> 5;
    const int r0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    KeepTwoNearest keep;
    if (!walk_tiles<D>(X, Y, nx, ny, cs.c_begin, cs.c_end, r0, li, half, keep)) return;
    // the two half-waves hold the two halves of the row's columns
    merge2(keep.k1, keep.k2, __shfl_xor(keep.k1, 32), __shfl_xor(keep.k2, 32));
    const int row = r0 + li;
    if (half == 0 && row < nx) {
        best[(long long)row * 2] = keep.k1;
        best[(long long)row * 2 + 1] = keep.k2;
    }
}

__global__ __launch_bounds__(256) void mutual_kernel(const unsigned long long* __restrict__ bestA,
                                                    const unsigned long long* __restrict__ bestB,
                                                    const int* __restrict__ nA, const int* __restrict__ nB,
                                                    int count_stride, int K, float thr,
                                                    int* __restrict__ match_idx, float* __restrict__ match_dist,
                                                    int* __restrict__ match_count, int nsplit)
{
    const int na = min(nA[blockIdx.y * count_stride], K), nb = min(nB[blockIdx.y * count_stride], K);
    write_matches(K, match_idx, match_dist, match_count, nullptr, nullptr, [&](int p, int i) {
        RowMatch m;
        if (i < na && nb > 0) {
            unsigned long long v, w, unused;
            merge_shares<1>(bestA, (long long)p * K + i, K, nsplit, v, unused);
            if (v != NO_KEY) {                                                         // (a gated row may have no candidate)
                const int jj = (int)(v & 0xffffffffu);
                m.d = __uint_as_float((unsigned)(v >> 32));
                merge_shares<1>(bestB, (long long)p * K + jj, K, nsplit, w, unused);
                const bool mutual = (int)(w & 0xffffffffu) == i;                  // matching.py:58-59 (i is in j's gate: w is a key)
                const bool close = (thr < 0.f) || (m.d < thr);                     // matching.py:56
                if (mutual && close) m.j = jj;
            }
        }
        return m;
    });
}

// ratio <= 0: every query row with a train row is matched to its nearest.  ratio > 0: kept iff d1 < ratio * d2, in double
// like Python's `m.distance < 0.9 * n.distance` (matching.py:25); a query without a second neighbour is not matched.
__global__ __launch_bounds__(256) void nearest_kernel(const unsigned long long* __restrict__ best2,
                                                     const int* __restrict__ nA, const int* __restrict__ nB,
                                                     int count_stride, int K, double ratio, int* __restrict__ match_idx,
                                                     float* __restrict__ match_dist, int* __restrict__ match_count,
                                                     int* __restrict__ second_idx, float* __restrict__ second_dist,
                                                     int nsplit)
{
    const int na = min(nA[blockIdx.y * count_stride], K), nb = min(nB[blockIdx.y * count_stride], K);
    write_matches(K, match_idx, match_dist, match_count, second_idx, second_dist, [&](int p, int i) {
        RowMatch m;
        if (i < na && nb > 0) {
            unsigned long long k1, k2;
            merge_shares<2>(best2, (long long)p * K + i, K, nsplit, k1, k2);
            m.d = __uint_as_float((unsigned)(k1 >> 32));
            if (k2 != NO_KEY) { m.j2 = (int)(k2 & 0xffffffffu); m.d2 = __uint_as_float((unsigned)(k2 >> 32)); }
            // (written as selects: hipcc 7 lost the kept index when this was `if (keep) j = ...` behind the nested condition)
            const bool lowe = (m.j2 >= 0) & ((double)m.d < ratio * (double)m.d2);
            const bool keep = (k1 != NO_KEY) & ((ratio > 0.0) ? lowe : true);
            m.j = keep ? (int)(k1 & 0xffffffffu) : -1;
        }
        return m;
    });
}

}  // namespace

// rowbest/colbest: [MATCH_SHARES][P][K] packed each; match_count is zeroed by the first launch
void launch_match_impl(const float* dA, const int* nA, const float* dB, const int* nB,
                       long long pair_stride, int count_stride, int P, int K, int D, float thr,
                       unsigned long long* rowbest, unsigned long long* colbest, int* match_idx,
                       float* match_dist, int* match_count, hipStream_t s)
{
    if (P <= 0 || K <= 0) return;
    for_width(D, [&](auto d) {
        hipLaunchKernelGGL((nn_rows_kernel<decltype(d)::value, NoGateArgs>), dim3((K + 127) / 128, P, 2 * MATCH_SHARES), dim3(256),
                           0, s, dA, nA, dB, nB, pair_stride, count_stride, K, rowbest, colbest, match_count, MATCH_SHARES,
                           NoGateArgs{});
    });
    launch_match_mutual_rows(rowbest, colbest, nA, nB, count_stride, P, K, thr, match_idx, match_dist, match_count, s);
}

// the mutual test on the two directions' best keys, with or without a gate
void launch_match_mutual_rows(const unsigned long long* rowbest, const unsigned long long* colbest, const int* nA, const int* nB,
                              int count_stride, int P, int K, float thr, int* match_idx, float* match_dist, int* match_count,
                              hipStream_t s)
{
    hipLaunchKernelGGL(mutual_kernel, dim3((K + 255) / 256, P), dim3(256), 0, s, rowbest, colbest, nA, nB, count_stride, K, thr,
                       match_idx, match_dist, match_count, MATCH_SHARES);
}

// best2: [MATCH_SHARES][P][K][2] packed keys; match_count is zeroed by the first launch
void launch_match_nearest(const float* dA, const int* nA, const float* dB, const int* nB, long long pair_stride,
                          int count_stride, int P, int K, int D, double ratio, unsigned long long* best2, int* match_idx,
                          float* match_dist, int* match_count, int* second_idx, float* second_dist, hipStream_t s)
{
    if (P <= 0 || K <= 0) return;
    for_width(D, [&](auto d) {
        hipLaunchKernelGGL(near2_rows_kernel<decltype(d)::value>, dim3((K + 127) / 128, P, MATCH_SHARES), dim3(256), 0, s, dA,
                           nA, dB, nB, pair_stride, count_stride, K, best2, match_count, MATCH_SHARES);
    });
    hipLaunchKernelGGL(nearest_kernel, dim3((K + 255) / 256, P), dim3(256), 0, s, best2, nA, nB, count_stride, K, ratio,
                       match_idx, match_dist, match_count, second_idx, second_dist, MATCH_SHARES);
}
