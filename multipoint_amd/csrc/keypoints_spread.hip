// Spatially uniform top-k: adaptive non-maximal suppression (ANMS; Brown, Szeliski and Winder 2005) on a keypoint list.
//
// No reference counterpart: the reference keeps the k highest scores (multipoint/utils/utils.py:109-116, keypoints.hip).  Here every
// candidate i of an image's list gets its suppression radius
//     R_i = min over { j : s_i < c (x) s_j } of (y_i - y_j)^2 + (x_i - x_j)^2        (uint32; 0xFFFFFFFF when nothing dominates i)
// with (x) ONE fp32 multiply, and the k candidates first in the order (R descending, score bits descending, row-major index
// ascending) are kept and written in row-major order -- the output contract of select_keypoints_kernel.  Everything is integer or
// single-rounding fp32 arithmetic and every R_i is a minimum over the whole list, so the result is a function of the list alone:
// not of the grid, of the batch, or of which workgroup took which chunk.
//   suppression_radius_kernel   all pairs of a list, the other candidates staged through LDS in tiles
//   select_spread_kernel        one workgroup per image: radix cut on R, radix cut on the score bits inside the R tie, row-major
//                               admission inside the exact (R, s) tie, ordered output (mp_select.h, as keypoints.hip)
#include "mp_common.h"
#include "mp_select.h"

namespace {

constexpr int RT = 256;            // threads per workgroup = candidates per chunk (one candidate per thread)
constexpr int RTILE = 1024;        // candidates staged per LDS tile: 8 bytes each, 8 KiB
constexpr int RGRID = 64;          // workgroups per image (fixed: the list length is only known on the device); they stride over chunks
constexpr int BTS = 1024;          // threads of the per-image selection workgroup
constexpr unsigned R_NONE = 0xFFFFFFFFu;

// packed (y, x): 16 bits each (frames up to 4096 x 4096; coordinates below 32768 keep d^2 inside 31 bits)
// LIST: row-major pixel index of a work map of width W (compact_segments_kernel<0>'s list); otherwise (y, x) int pairs
template <bool LIST>
__device__ __forceinline__ unsigned load_yx(const int* __restrict__ pos, int i, int W)
{
    if (LIST) { const int idx = pos[i]; return ((unsigned)(idx / W) << 16) | (unsigned)(idx % W); }
    return ((unsigned)pos[2 * i] << 16) | ((unsigned)pos[2 * i + 1] & 0xffffu);
}

template <bool LIST>
__global__ __launch_bounds__(RT) void suppression_radius_kernel(const int* __restrict__ pos, const float* __restrict__ score,
                                                                const int* __restrict__ count, long long stride, int cap, int W,
                                                                float c, unsigned* __restrict__ radius2)
{
    __shared__ uint2 s_tile[RTILE];          // .x packed (y, x), .y bits of c (x) s_j
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = min(max(count[b], 0), cap);
    pos += (long long)b * stride * (LIST ? 1 : 2);
    score += (long long)b * stride;
    radius2 += (long long)b * stride;
    for (int chunk = blockIdx.x * RT; chunk < n; chunk += gridDim.x * RT) {          // (uniform over the workgroup)
        const int i = chunk + tid;
        const bool own = i < n;
        float si = 0.f;
        int yi = 0, xi = 0;
        if (own) {
            const unsigned p = load_yx<LIST>(pos, i, W);
            si = score[i]; yi = (int)(p >> 16); xi = (int)(p & 0xffffu);
        }
        unsigned r = R_NONE;
        for (int t0 = 0; t0 < n; t0 += RTILE) {
            __syncthreads();                 // the previous tile's readers are done
            for (int e = tid; e < RTILE; e += RT) {
                const int j = t0 + e;
                uint2 v = make_uint2(0u, __float_as_uint(-__builtin_inff()));          // beyond the list: dominates nothing
                if (j < n) v = make_uint2(load_yx<LIST>(pos, j, W), __float_as_uint(__fmul_rn(c, score[j])));
                s_tile[e] = v;
            }
            __syncthreads();
            const int m = (min(RTILE, n - t0) + 3) & ~3;
            for (int e = 0; e < m; e += 4) {          // every lane reads the same entry: an LDS broadcast, no bank conflicts
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint2 v = s_tile[e + u];
                    const int dy = (int)(v.x >> 16) - yi, dx = (int)(v.x & 0xffffu) - xi;
                    const unsigned d2 = (unsigned)(dy * dy + dx * dx);
                    if (si < __uint_as_float(v.y)) r = min(r, d2);
                }
            }
        }
        if (own) radius2[i] = r;
    }
}

__global__ __launch_bounds__(BTS) void select_spread_kernel(int H, int W, int topk, int K, const int* __restrict__ list_idx,
                                                            const float* __restrict__ list_score,
                                                            const unsigned* __restrict__ list_r2, int list_cap,
                                                            const int* __restrict__ list_count, int* __restrict__ kp_yx,
                                                            float* __restrict__ kp_score, unsigned* __restrict__ kp_radius2,
                                                            int* __restrict__ kp_count, float* __restrict__ prob_nms, int Wout)
{
    __shared__ int s_wave[BTS / 64];
    __shared__ unsigned s_hist[256];
    __shared__ unsigned s_sel[2];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int* lidx = list_idx + (long long)b * list_cap;
    const float* lsc = list_score + (long long)b * list_cap;
    const unsigned* lr = list_r2 + (long long)b * list_cap;
    const int nk = min(list_count[b], list_cap);

    // admit R > TR; of R == TR the score bits > TS; of (R, s) == (TR, TS) the first `need` in row-major order
    unsigned TR = 0, TS = 0;
    int need = 0;
    const bool select = nk > topk;
    if (select) {
        int need_r;
        radix_select_cut<BTS>([&](int i) { return lr[i]; }, nk, topk, s_hist, s_wave, s_sel, &TR, &need_r);
        // the need_r best scores among the entries AT the radius cut (there are at least need_r of them): scores are positive, so
        // every other entry's key 0 sorts below all of theirs
        radix_select_cut<BTS>([&](int i) { return lr[i] == TR ? __float_as_uint(lsc[i]) : 0u; }, nk, need_r, s_hist, s_wave, s_sel,
                              &TS, &need);
    }

    // ordered output (row-major)
    int out_base = 0, tie_base = 0;
    for (int start = 0; start < nk; start += BTS) {
        const int i = start + tid;
        unsigned key = 0, r = 0;
        int idx = 0;
        float sc = 0.f;
        if (i < nk) { sc = lsc[i]; key = __float_as_uint(sc); idx = lidx[i]; r = lr[i]; }
        bool sel = i < nk;
        if (select) {
            const int eq = (i < nk) && (r == TR) && (key == TS);
            int tie_rank = 0;
            if (__syncthreads_or(eq)) {
                int tot_eq;
                tie_rank = tie_base + block_excl_scan<BTS>(eq, s_wave, &tot_eq);
                tie_base += tot_eq;
            }
            sel = (i < nk) && ((r > TR) || (r == TR && key > TS) || (eq && tie_rank < need));
        }
        int tot;
        const int pos = out_base + block_excl_scan<BTS>(sel ? 1 : 0, s_wave, &tot);
        out_base += tot;
        if (sel && pos < K) {
            if (kp_yx) {
                kp_yx[((long long)b * K + pos) * 2] = idx / W;
                kp_yx[((long long)b * K + pos) * 2 + 1] = idx % W;
            }
            if (kp_score) kp_score[(long long)b * K + pos] = sc;
            if (kp_radius2) kp_radius2[(long long)b * K + pos] = r;
        }
        // (Wout: the dense output's row stride -- the caller's width; W is that rounded up to a multiple of 4)
        if (sel && prob_nms) prob_nms[(long long)b * H * Wout + (long long)(idx / W) * Wout + idx % W] = sc;
    }
    if (tid == 0 && kp_count) kp_count[b] = out_base;
}

}  // namespace

void launch_suppression_radii(const int* kp_yx, const float* kp_score, const int* kp_count, int B, int K, float robust,
                              unsigned* radius2, hipStream_t s)
{
    if (B <= 0 || K <= 0) return;
    hipLaunchKernelGGL(suppression_radius_kernel<false>, dim3(RGRID, B), dim3(RT), 0, s, kp_yx, kp_score, kp_count, (long long)K, K, 0,
                       robust, radius2);
}

void launch_select_spread(int B, int H, int W, int topk, int K, const int* list_idx, const float* list_score, unsigned* list_r2,
                          int list_cap, const int* list_count, float robust, int* kp_yx, float* kp_score, unsigned* kp_radius2,
                          int* kp_count, float* prob_nms, int Wout, hipStream_t s)
{
    if (B <= 0) return;
    hipLaunchKernelGGL(suppression_radius_kernel<true>, dim3(RGRID, B), dim3(RT), 0, s, list_idx, list_score, list_count,
                       (long long)list_cap, list_cap, W, robust, list_r2);
    hipLaunchKernelGGL(select_spread_kernel, dim3(B), dim3(BTS), 0, s, H, W, topk, K, list_idx, list_score, list_r2, list_cap,
                       list_count, kp_yx, kp_score, kp_radius2, kp_count, prob_nms, Wout);
}
