// RIFT baseline (Li, Hu, Ai, IEEE TIP 2020, restated): what stands between the FFT's row passes (fft.hip) and the
// FAST and patch-histogram kernels it shares with LGHD (lghd.hip): the noise thresholds from the exact medians of the six scale-0
// amplitude planes, and the 8-bit image of the maximum-moment map M that FAST runs on.
#include "mp_common.h"
#include "mp_select.h"

namespace {

struct NoiseConsts {
    double sqrt_ln4;       // sqrt(ln 4)
    double c1, c2;         // 1 - q^4 and 1 - q, q = 1 / 1.6
    double s1, s2;         // sqrt(pi / 2), sqrt((4 - pi) / 2)
    double k;
};

// T = tot s1 + (k tot) s2, tot = tau c1 / c2, tau = median / sqrt(ln 4): float64, every operation rounded on its own, the result
// rounded once to fp32.  One workgroup per plane of n amplitudes (non-negative, so their bit patterns order like the floats):
// an 8-bit radix select finds the lower middle element and how many of its equals lie above the cut; the upper middle element
// of an even n is the same value, or the smallest key above it.
__global__ __launch_bounds__(1024) void noise_threshold_kernel(const float* __restrict__ amp, int n, const NoiseConsts c,
                                                              float* __restrict__ T)
{
    __shared__ unsigned s_hist[256], s_sel[2], s_min[16];
    __shared__ int s_wave[16];
    const int tid = threadIdx.x;
    const float* a = amp + (long long)blockIdx.x * n;
    const int k = n - (n - 1) / 2;          // the k-th largest is element (n - 1) / 2 in ascending order
    unsigned lo;
    int need;
    radix_select_cut<1024>([a](int i) { return __float_as_uint(a[i]); }, n, k, s_hist, s_wave, s_sel, &lo, &need);
    unsigned hi = lo;
    if (!(n & 1) && need == 1) {            // (uniform over the workgroup)
        unsigned mn = 0xffffffffu;
        for (int i = tid; i < n; i += 1024) {
            const unsigned key = __float_as_uint(a[i]);
            if (key > lo) mn = min(mn, key);
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) mn = min(mn, (unsigned)__shfl_xor((int)mn, off));
        if ((tid & 63) == 0) s_min[tid >> 6] = mn;
        __syncthreads();
        hi = s_min[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) hi = min(hi, s_min[i]);
    }
    if (tid == 0) {
        const double median = __dmul_rn(__dadd_rn((double)__uint_as_float(lo), (double)__uint_as_float(hi)), 0.5);
        const double tau = __ddiv_rn(median, c.sqrt_ln4);
        const double tot = __ddiv_rn(__dmul_rn(tau, c.c1), c.c2);
        T[blockIdx.x] = (float)__dadd_rn(__dmul_rn(tot, c.s1), __dmul_rn(__dmul_rn(c.k, tot), c.s2));
    }
}

// range[b] = (min, max) of M[b]: one workgroup per image (minimum and maximum do not depend on the order)
__global__ __launch_bounds__(1024) void moment_range_kernel(const float* __restrict__ M, long long HW, float* __restrict__ range)
{
    __shared__ float s_mn[16], s_mx[16];
    const int tid = threadIdx.x;
    const float* a = M + blockIdx.x * HW;
    float mn = a[0], mx = a[0];
    for (long long i = tid; i < HW; i += 1024) { mn = fminf(mn, a[i]); mx = fmaxf(mx, a[i]); }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { mn = fminf(mn, __shfl_xor(mn, off)); mx = fmaxf(mx, __shfl_xor(mx, off)); }
    if ((tid & 63) == 0) { s_mn[tid >> 6] = mn; s_mx[tid >> 6] = mx; }
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < 16; ++i) { mn = fminf(mn, s_mn[i]); mx = fmaxf(mx, s_mx[i]); }
        range[blockIdx.x * 2] = mn; range[blockIdx.x * 2 + 1] = mx;
    }
}

// u8m = (uint8) floor(255 ((M - min) / (max - min))): one subtraction, one correctly rounded division, one multiplication, each
// rounded to fp32 on its own; all zero where max == min
__global__ __launch_bounds__(256) void moment_u8_kernel(const float* __restrict__ M, long long HW, const float* __restrict__ range,
                                                       unsigned char* __restrict__ u8m)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= HW) return;
    const float mn = range[blockIdx.y * 2], span = __fsub_rn(range[blockIdx.y * 2 + 1], mn);
    const long long at = blockIdx.y * HW + i;
    u8m[at] = span > 0.f ? (unsigned char)(int)__fmul_rn(255.f, __fdiv_rn(__fsub_rn(M[at], mn), span)) : 0;
}

}  // namespace

void launch_rift_noise_threshold(const float* amp, int planes, long long HW, float k, float* T, hipStream_t s)
{
    const double q = 1.0 / 1.6, pi = 3.14159265358979323846;
    NoiseConsts c;
    c.sqrt_ln4 = sqrt(log(4.0));
    c.c1 = 1.0 - q * q * q * q; c.c2 = 1.0 - q;
    c.s1 = sqrt(pi / 2.0); c.s2 = sqrt((4.0 - pi) / 2.0);
    c.k = (double)k;
    hipLaunchKernelGGL(noise_threshold_kernel, dim3(planes), dim3(1024), 0, s, amp, (int)HW, c, T);
}

void launch_rift_detect(const float* M, int B, int H, int W, int threshold, int patch, unsigned char* u8m, float* range,
                        unsigned char* score, unsigned char* corners, float* prob, hipStream_t s)
{
    const long long HW = (long long)H * W;
    hipLaunchKernelGGL(moment_range_kernel, dim3(B), dim3(1024), 0, s, M, HW, range);
    hipLaunchKernelGGL(moment_u8_kernel, dim3((unsigned)((HW + 255) / 256), B), dim3(256), 0, s, M, HW, range, u8m);
    launch_fast_detect(u8m, B, H, W, threshold, patch / 2, 1, score, corners, prob, s);
}
