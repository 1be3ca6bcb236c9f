// One-directional matching on the MFMA distance tiles of sample_match.hip: the nearest train row of every query row
// (cv2.BFMatcher(cv2.NORM_L2).match() without crossCheck, reference multipoint/utils/matching.py:7,31) and the two
// nearest plus Lowe's ratio test (knnMatch(d1, d2, 2), matching.py:20-27), for P pairs per launch.
//
// near2_rows_kernel is nn_rows_kernel (sample_match.hip) with ONE direction and TWO running keys per lane: the same
// 32 x 32 tiles on v_mfma_f32_32x32x2_f32 with the products formed transposed (lane li owns query row r0 + li), the same
// double-buffered train tile in LDS, the same column shares, the same metric d = sqrt(2 - 2 clip(x.y, -1, 1)) -- the L2
// distance of UNIT rows -- and the same packed key (distance bits << 32 | train index).  Keys are distinct (the index is
// part of the key), so "the two smallest keys of a row" is a pure function of the inputs whatever the order in which
// lanes, half-waves and shares are merged, and exact distance ties go to the lower train index first (OpenCV inserts a
// candidate only if it is strictly closer).  nearest_kernel merges the shares and applies the mode.
#include "mp_common.h"

namespace {

constexpr unsigned long long NO_KEY = ~0ull;             // (distance bits 0xffffffff are a NaN: never a real key)

// the two smallest of the union of two ascending key pairs
__device__ __forceinline__ void merge2(unsigned long long& k1, unsigned long long& k2, unsigned long long o1,
                                       unsigned long long o2)
{
    const unsigned long long lo = k1 < o1 ? k1 : o1, hi = k1 < o1 ? o1 : k1, s = k2 < o2 ? k2 : o2;
    k1 = lo;
    k2 = hi < s ? hi : s;
}

// best2[x] = the two smallest (dist(x,y) bits << 32 | y) over the share's rows y of B, for every row x of A.
// grid: (row-block groups, pairs, column shares); tiling, staging and barriers exactly as nn_rows_kernel.
template <int D>
__global__ __launch_bounds__(256) void near2_rows_kernel(const float* __restrict__ dA, const int* __restrict__ nA,
                                                        const float* __restrict__ dB, const int* __restrict__ nB,
                                                        long long pair_stride, int count_stride, int K,
                                                        unsigned long long* __restrict__ best2,
                                                        int* __restrict__ match_count, int nsplit)
{
    // (the pair's match counter, which nearest_kernel adds to behind this launch, is zeroed here)
    if (blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x == 0) match_count[blockIdx.y] = 0;
    constexpr int RS = D + 4;                            // LDS row stride in floats
    __shared__ __attribute__((aligned(16))) float ytile[2][32 * RS];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, half = lane >> 5;
    const int p = blockIdx.y, share = blockIdx.z;
    const float* X = dA + (long long)p * pair_stride;
    const float* Y = dB + (long long)p * pair_stride;
    const int nx = min(nA[p * count_stride], K);
    const int ny = min(nB[p * count_stride], K);
    unsigned long long* best = best2 + (((long long)share * gridDim.y + p) * K) * 2;
    const int ntile = (ny + 31) >> 5, per = (ntile + nsplit - 1) / nsplit;
    const int c_begin = min(share * per, ntile) * 32, c_end = min(min((share + 1) * per, ntile) * 32, ny);
    if ((int)blockIdx.x * 128 >= nx) return;             // (the whole workgroup)
    const int r0 = (blockIdx.x * 4 + wave) * 32;
    const bool active = r0 < nx;                         // a wave without rows still stages tiles and meets the barriers

    constexpr int NG = D / 8;
    f32x4 a[NG];
    {
        const int row = min(r0 + li, nx - 1);
#pragma unroll
        for (int g = 0; g < NG; ++g)
            a[g] = *reinterpret_cast<const f32x4*>(X + (long long)row * D + g * 8 + half * 4);
    }
    // Two running keys per lane, k1 < k2, and the u = 2 - 2 clip(x.y) each of them came from.  Columns reach a lane in
    // ascending order and d = sqrt(u) is monotone in u, so a column whose u is not below ub2 has d >= the second distance
    // and a larger index: its key cannot enter.  "u < ub2" (strict) is the one compare every element pays; the correctly
    // rounded sqrt and the 64-bit updates run only behind it.
    unsigned long long k1 = NO_KEY, k2 = NO_KEY;
    float ub1 = __builtin_inff(), ub2 = __builtin_inff();

    // staging: the tile's 32 * D / 4 granules of 16 bytes, D / 32 per thread (rows beyond ny repeat row ny - 1; never selected)
    constexpr int GPT = D / 32, GPR = D / 4;
    f32x4 stage[GPT];
    auto gload = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < GPT; ++k) {
            const int gran = tid + k * 256;
            const int row = gran / GPR, q = gran - row * GPR;
            stage[k] = *reinterpret_cast<const f32x4*>(Y + (long long)min(c0 + row, ny - 1) * D + q * 4);
        }
    };
    auto lstore = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < GPT; ++k) {
            const int gran = tid + k * 256;
            const int row = gran / GPR, q = gran - row * GPR;
            *reinterpret_cast<f32x4*>(&ytile[buf][row * RS + q * 4]) = stage[k];
        }
    };
    if (c_begin < c_end) { gload(c_begin); lstore(0); }
    __syncthreads();
    for (int c0 = c_begin, buf = 0; c0 < c_end; c0 += 32, buf ^= 1) {
        const bool more = c0 + 32 < c_end;
        if (more) gload(c0 + 32);                        // in flight across this tile's MFMAs
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(&ytile[buf][li * RS + g * 8 + half * 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[e], a[g][e], acc, 0, 0, 0);      // acc[r]: column i(r) of the tile, row li
        }
        if (active) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int col = c0 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const float t = fminf(fmaxf(acc[r], -1.f), 1.f);               // np.clip, matching.py:51
                const float u = 2.f - 2.f * t;
                if (col < ny && u < ub2) {
                    const float d = sqrtf(u);
                    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)col;
                    if (key < k1) { k2 = k1; ub2 = ub1; k1 = key; ub1 = u; }
                    else if (key < k2) { k2 = key; ub2 = u; }                 // (equal d, larger index: neither)
                }
            }
        }
        if (more) lstore(buf ^ 1);                       // last read one barrier ago
        __syncthreads();
    }
    if (!active) return;
    // the two half-waves hold the two halves of the row's columns
    merge2(k1, k2, __shfl_xor(k1, 32), __shfl_xor(k2, 32));
    const int row = r0 + li;
    if (half == 0 && row < nx) {
        best[(long long)row * 2] = k1;
        best[(long long)row * 2 + 1] = k2;
    }
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
    const int p = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const long long share_stride = (long long)gridDim.y * K * 2;    // the column shares' arrays lie [share][pair][K][2]
    const int na = min(nA[p * count_stride], K), nb = min(nB[p * count_stride], K);
    int hit = 0;
    if (i < K) {
        int j = -1, j2 = -1;
        float d = 0.f, d2 = 0.f;
        if (i < na && nb > 0) {
            const long long at = ((long long)p * K + i) * 2;
            unsigned long long k1 = best2[at], k2 = best2[at + 1];
            for (int sh = 1; sh < nsplit; ++sh) merge2(k1, k2, best2[at + sh * share_stride], best2[at + sh * share_stride + 1]);
            d = __uint_as_float((unsigned)(k1 >> 32));
            if (k2 != NO_KEY) { j2 = (int)(k2 & 0xffffffffu); d2 = __uint_as_float((unsigned)(k2 >> 32)); }
            // (written as selects: hipcc 7 lost the kept index when this was `if (keep) j = ...` behind the nested condition)
            const bool lowe = (j2 >= 0) & ((double)d < ratio * (double)d2);
            const bool keep = (k1 != NO_KEY) & ((ratio > 0.0) ? lowe : true);
            j = keep ? (int)(k1 & 0xffffffffu) : -1;
        }
        const long long o = (long long)p * K + i;
        match_idx[o] = j;
        match_dist[o] = j >= 0 ? d : 0.f;
        if (second_idx) second_idx[o] = j2;
        if (second_dist) second_dist[o] = j2 >= 0 ? d2 : 0.f;
        hit = j >= 0;
    }
    const int c = __syncthreads_count(hit);
    if (threadIdx.x == 0 && c) atomicAdd(&match_count[p], c);
}

}  // namespace

// best2: [MATCH_SHARES][P][K][2] packed keys; match_count is zeroed by the first launch
void launch_match_nearest(const float* dA, const int* nA, const float* dB, const int* nB, long long pair_stride,
                          int count_stride, int P, int K, int D, double ratio, unsigned long long* best2, int* match_idx,
                          float* match_dist, int* match_count, int* second_idx, float* second_dist, hipStream_t s)
{
    if (P <= 0 || K <= 0) return;
    const dim3 grid((K + 127) / 128, P, MATCH_SHARES);
    if (D == 64)
        hipLaunchKernelGGL(near2_rows_kernel<64>, grid, dim3(256), 0, s, dA, nA, dB, nB, pair_stride, count_stride, K,
                           best2, match_count, MATCH_SHARES);
    else if (D == 128)
        hipLaunchKernelGGL(near2_rows_kernel<128>, grid, dim3(256), 0, s, dA, nA, dB, nB, pair_stride, count_stride, K,
                           best2, match_count, MATCH_SHARES);
    else
        hipLaunchKernelGGL(near2_rows_kernel<256>, grid, dim3(256), 0, s, dA, nA, dB, nB, pair_stride, count_stride, K,
                           best2, match_count, MATCH_SHARES);
    hipLaunchKernelGGL(nearest_kernel, dim3((K + 255) / 256, P), dim3(256), 0, s, best2, nA, nB, count_stride, K, ratio,
                       match_idx, match_dist, match_count, second_idx, second_dist, MATCH_SHARES);
}
