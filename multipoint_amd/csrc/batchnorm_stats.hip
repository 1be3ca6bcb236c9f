// BatchNorm2d with the statistics of the current batch (training-mode forward, forward only): the reference's train.py never
// calls net.eval(), so its validation loop normalises every BatchNorm with the mean and biased variance of the batch
// (torch.nn.functional.batch_norm(training=True), eps 1e-5) and blends the batch mean / unbiased variance into the running
// statistics.  The convolutions run with an identity epilogue (forward.hip: run_forward_batch_stats); these kernels do the rest.
//
// bn_gather_kernel      the images routed to one encoder of a multispectral model, gathered into a contiguous batch (its
//                       statistics cover those images only, MultiPoint.py:117-122)
// bn_stats_kernel       per-channel shifted sums of an NHWC fp32 activation [npx][cstride] over all npx pixels: a lane owns
//                       4 consecutive channels (one 16-byte load; a row of lanes reads a pixel's channels contiguously), a
//                       workgroup a fixed contiguous range of pixels.  The sums are of d = x - K, K = the channel's value at
//                       pixel 0, in fp64: a near-constant channel does not cancel.  Each workgroup writes its partial into
//                       slot blockIdx, summed over its lanes in a fixed order.
// bn_finalize_kernel    one thread per channel sums the partials in slot order (fp64) and writes scale = gamma invstd,
//                       shift = beta - mean scale (invstd = 1 / sqrt(var_biased + 1e-5)) and the batch mean / unbiased
//                       variance; padding channels get scale = shift = 0 and no statistics
// bn_apply_kernel       y = x scale + shift (one fma), then ReLU (bn_first models), then 2x2 max-pool where MaxPool2d(2,2)
//                       follows the block (after the affine: gamma can be negative); optional scatter of the images back to
//                       their places in the batch
// No atomics anywhere: the results are bit-identical from run to run.
#include "mp_common.h"

#include <algorithm>

namespace {

constexpr int BN_THREADS = 256;

__global__ __launch_bounds__(BN_THREADS) void bn_gather_kernel(const float* __restrict__ img, const int* __restrict__ list,
                                                               long long hw4, float* __restrict__ out)
{
    const int b = blockIdx.y;
    const f32x4* src = reinterpret_cast<const f32x4*>(img) + (long long)list[b] * hw4;
    f32x4* dst = reinterpret_cast<f32x4*>(out) + (long long)b * hw4;
    for (long long i = (long long)blockIdx.x * BN_THREADS + threadIdx.x; i < hw4; i += (long long)gridDim.x * BN_THREADS)
        dst[i] = src[i];
}

__global__ __launch_bounds__(BN_THREADS) void bn_stats_kernel(const float* __restrict__ x, long long npx, int C, int cstride,
                                                              long long chunk, double* __restrict__ part)
{
    __shared__ double red[2][4][BN_THREADS];
    const int tid = threadIdx.x;
    const int c4n = C >> 2;                    // lanes per pixel
    const int rows = BN_THREADS / c4n;         // pixels per pass
    const int q = tid % c4n, r = tid / c4n;
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    if (r < rows) {
        const f32x4 k4 = *reinterpret_cast<const f32x4*>(x + 4 * q);
        const long long p0 = (long long)blockIdx.x * chunk;
        const long long p1 = min(p0 + chunk, npx);
        const float* base = x + 4 * q;
        long long p = p0 + r;
        // four loads in flight per lane
        for (; p + 3 * rows < p1; p += 4 * rows) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(base + (p + (long long)u * rows) * cstride);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double d = (double)v[u][e] - (double)k4[e];
                    s1[e] += d;
                    s2[e] = fma(d, d, s2[e]);
                }
        }
        for (; p < p1; p += rows) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(base + p * cstride);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double d = (double)v[e] - (double)k4[e];
                s1[e] += d;
                s2[e] = fma(d, d, s2[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[0][e][tid] = s1[e]; red[1][e][tid] = s2[e]; }
    __syncthreads();
    if (tid < c4n) {
        double t1[4] = {0.0, 0.0, 0.0, 0.0}, t2[4] = {0.0, 0.0, 0.0, 0.0};
        for (int rr = 0; rr < rows; ++rr)          // fixed order: row 0, 1, ...
#pragma unroll
            for (int e = 0; e < 4; ++e) { t1[e] += red[0][e][rr * c4n + tid]; t2[e] += red[1][e][rr * c4n + tid]; }
        double* o = part + (long long)blockIdx.x * 2 * C + 4 * tid;
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[e] = t1[e]; o[C + e] = t2[e]; }
    }
}

__global__ __launch_bounds__(BN_THREADS) void bn_finalize_kernel(const double* __restrict__ part, int nparts, int C,
                                                                 const float* __restrict__ x, long long n, int c0, int nc,
                                                                 int c_real, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float* __restrict__ scale,
                                                                 float* __restrict__ shift, float* __restrict__ mean_out,
                                                                 float* __restrict__ var_out)
{
    const int c = blockIdx.x * BN_THREADS + threadIdx.x;      // channel of this range
    if (c >= nc) return;
    const int cc = c0 + c;                                    // ... of the tensor
    if (c >= c_real) { scale[cc] = 0.f; shift[cc] = 0.f; return; }
    double t1 = 0.0, t2 = 0.0;
    for (int g = 0; g < nparts; ++g) {
        t1 += part[(long long)g * 2 * C + cc];
        t2 += part[(long long)g * 2 * C + C + cc];
    }
    const double dn = (double)n;
    const double m1 = t1 / dn;                                // mean of d = x - K
    const double var = fmax(t2 / dn - m1 * m1, 0.0);          // biased
    const double mean = (double)x[cc] + m1;
    const double invstd = 1.0 / sqrt(var + 1e-5);
    const double sc = (double)gamma[c] * invstd;
    scale[cc] = (float)sc;
    shift[cc] = (float)((double)beta[c] - mean * sc);
    if (mean_out) {
        mean_out[c] = (float)mean;
        var_out[c] = (float)(var * dn / (dn - 1.0));
    }
}

template <bool POOL, bool RELU>
__global__ __launch_bounds__(BN_THREADS) void bn_apply_kernel(const float* x, float* y, int nrows, int H, int W, int C,
                                                              const float* __restrict__ scale, const float* __restrict__ shift,
                                                              const int* __restrict__ out_list)
{
    // one output row (image, oy) per blockIdx.y step; lanes over (ox, channel quad) of the row
    const int c4n = C >> 2;
    const int Ho = POOL ? H / 2 : H, Wo = POOL ? W / 2 : W;
    const int per_row = Wo * c4n;
    const int i = blockIdx.x * BN_THREADS + threadIdx.x;
    if (i >= per_row) return;
    const int q = i % c4n, ox = i / c4n;
    const f32x4 s4 = *reinterpret_cast<const f32x4*>(scale + 4 * q);
    const f32x4 t4 = *reinterpret_cast<const f32x4*>(shift + 4 * q);
    auto act = [&](f32x4 v) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a = fmaf(v[e], s4[e], t4[e]);
            if (RELU) a = fmaxf(a, 0.f);
            o[e] = a;
        }
        return o;
    };
    for (int row = blockIdx.y; row < nrows; row += gridDim.y) {
        const int b = row / Ho, oy = row - b * Ho;
        f32x4 o;
        if constexpr (POOL) {
            const float* src = x + (((long long)b * H + 2 * oy) * W + 2 * ox) * C + 4 * q;
            const f32x4 a0 = act(*reinterpret_cast<const f32x4*>(src));
            const f32x4 a1 = act(*reinterpret_cast<const f32x4*>(src + C));
            const f32x4 a2 = act(*reinterpret_cast<const f32x4*>(src + (long long)W * C));
            const f32x4 a3 = act(*reinterpret_cast<const f32x4*>(src + (long long)W * C + C));
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = fmaxf(fmaxf(a0[e], a1[e]), fmaxf(a2[e], a3[e]));
        } else {
            o = act(*reinterpret_cast<const f32x4*>(x + (((long long)b * H + oy) * W + ox) * C + 4 * q));
        }
        const int ob = out_list ? out_list[b] : b;
        *reinterpret_cast<f32x4*>(y + (((long long)ob * Ho + oy) * Wo + ox) * C + 4 * q) = o;
    }
}

}  // namespace

void launch_bn_gather(const float* img, const int* list, int nb, int H, int W, float* out, hipStream_t s)
{
    const long long hw4 = (long long)H * W / 4;
    const unsigned gx = (unsigned)std::min<long long>((hw4 + BN_THREADS - 1) / BN_THREADS, 1024);
    if (nb <= 0 || hw4 <= 0) return;
    hipLaunchKernelGGL(bn_gather_kernel, dim3(gx, (unsigned)nb), dim3(BN_THREADS), 0, s, img, list, hw4, out);
}

int bn_stats_parts(long long npx, int C)
{
    const long long rows = BN_THREADS / (C / 4);
    const long long want = (npx + rows * 16 - 1) / (rows * 16);          // at least 16 pixels per lane
    return (int)std::max<long long>(1, std::min<long long>(want, MP_BN_MAX_PARTS));
}

void launch_bn_stats(const float* x, long long npx, int C, int cstride, double* part, hipStream_t s)
{
    const int g = bn_stats_parts(npx, C);
    const long long chunk = (npx + g - 1) / g;
    hipLaunchKernelGGL(bn_stats_kernel, dim3((unsigned)g), dim3(BN_THREADS), 0, s, x, npx, C, cstride, chunk, part);
}

void launch_bn_finalize(const double* part, long long npx, int C, const float* x, int c0, int nc, int c_real, const float* gamma,
                        const float* beta, float* scale, float* shift, float* mean_out, float* var_out, hipStream_t s)
{
    const int g = bn_stats_parts(npx, C);
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((unsigned)((nc + BN_THREADS - 1) / BN_THREADS)), dim3(BN_THREADS), 0, s, part, g,
                       C, x, npx, c0, nc, c_real, gamma, beta, scale, shift, mean_out, var_out);
}

void launch_bn_apply(const float* x, float* y, int B, int H, int W, int C, const float* scale, const float* shift, bool relu,
                     bool pool, const int* out_list, hipStream_t s)
{
    const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
    const int nrows = B * Ho, per_row = Wo * (C / 4);
    if (nrows <= 0 || per_row <= 0) return;
    const dim3 grid((unsigned)((per_row + BN_THREADS - 1) / BN_THREADS), (unsigned)std::min(nrows, 65535));
    if (pool) {
        if (relu) hipLaunchKernelGGL((bn_apply_kernel<true, true>), grid, dim3(BN_THREADS), 0, s, x, y, nrows, H, W, C, scale, shift, out_list);
        else hipLaunchKernelGGL((bn_apply_kernel<true, false>), grid, dim3(BN_THREADS), 0, s, x, y, nrows, H, W, C, scale, shift, out_list);
    } else {
        if (relu) hipLaunchKernelGGL((bn_apply_kernel<false, true>), grid, dim3(BN_THREADS), 0, s, x, y, nrows, H, W, C, scale, shift, out_list);
        else hipLaunchKernelGGL((bn_apply_kernel<false, false>), grid, dim3(BN_THREADS), 0, s, x, y, nrows, H, W, C, scale, shift, out_list);
    }
}
