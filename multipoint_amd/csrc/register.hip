// Fourier-Mellin registration: the four stages around the 2-D FFT of fft.hip.  All are memory-bound: one lane
// owns one output value, consecutive lanes own consecutive values (a wave writes 512 contiguous bytes of a complex plane or
// reads 256 of a real one), gathers go through the caches, and nothing is accumulated with atomics -- every result is bit for
// bit the same from run to run.
//
//   register_prepare_kernel       one lane per complex value of the N x N plane.  Inside the H x W window the four taps
//                                 (x +- 1, y), (x, y +- 1) are mapped through the frame's similarity about its centre with
//                                 explicit fused multiply-adds (the float64 restatement repeats exactly these, so both sides
//                                 agree on which pixels are zero), sampled bilinearly, and the windowed magnitude of the central
//                                 differences is stored; everything else is zero.
//   register_logpolar_kernel      one lane per (angle, radius): log1p|F| at the four spectrum bins around the sample -- the
//                                 fftshift is index arithmetic, modulo N -- interpolated and windowed.
//   register_cross_power_kernel   one lane per bin of one group: the unit cross-power of the group's pairs added in pair order.
//   register_peak_kernel          two stages, twice: per chunk of MP_REGISTER_PEAK_CHUNK values the maximum and its first index,
//                                 then per plane the reduction of the chunks' results (same tie rule: the larger value, then the
//                                 smaller index) and the parabola fit; the second round repeats both with the wrapped 3 x 3 block
//                                 around the maximum left out.
#include "mp_common.h"
#include "mp_device.h"
#include "mp_workspace.h"

#include <climits>

namespace {

constexpr int THREADS = 256;

// bilinear sample of f [H][W] at (sx, sy); false when one of the four samples lies outside the frame (or sx, sy is NaN)
__device__ __forceinline__ bool bilinear_inside(const float* __restrict__ f, int H, int W, float sx, float sy, float& v)
{
    const float x0f = floorf(sx), y0f = floorf(sy);
    if (!(x0f >= 0.f && y0f >= 0.f && x0f <= (float)(W - 2) && y0f <= (float)(H - 2))) return false;
    const float fx = sx - x0f, fy = sy - y0f;                   // exact
    const float* p = f + (size_t)(int)y0f * W + (int)x0f;
    const float top = fmaf(fx, p[1] - p[0], p[0]);
    const float bot = fmaf(fx, p[W + 1] - p[W], p[W]);
    v = fmaf(fy, bot - top, top);
    return true;
}

__global__ __launch_bounds__(THREADS) void register_prepare_kernel(const float* __restrict__ frames, const float* __restrict__ cs,
                                                                   const float* __restrict__ wy, const float* __restrict__ wx,
                                                                   int H, int W, int N, float2* __restrict__ out)
{
    const int img = blockIdx.y;
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= N * N) return;
    const int Y = idx / N, X = idx - Y * N;
    const int y = Y - (N - H) / 2, x = X - (N - W) / 2;
    float val = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
        const float c = cs ? cs[2 * img] : 1.f, s = cs ? cs[2 * img + 1] : 0.f;
        const float cx = (float)(W - 1) * 0.5f, cy = (float)(H - 1) * 0.5f;
        const float* f = frames + (size_t)img * H * W;
        float t[4];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int dx = k == 0 ? 1 : k == 1 ? -1 : 0, dy = k == 2 ? 1 : k == 3 ? -1 : 0;
            const float px = (float)(x + dx) - cx, py = (float)(y + dy) - cy;     // exact: half-integers
            const float sx = fmaf(c, px, fmaf(-s, py, cx));
            const float sy = fmaf(s, px, fmaf(c, py, cy));
            t[k] = 0.f;
            ok = bilinear_inside(f, H, W, sx, sy, t[k]) && ok;
        }
        if (ok) {
            const float gx = 0.5f * (t[0] - t[1]), gy = 0.5f * (t[2] - t[3]);
            val = sqrtf(gx * gx + gy * gy) * (wy[y] * wx[x]);
        }
    }
    out[(size_t)img * N * N + idx] = make_float2(val, 0.f);
}

// index of the spectrum that holds value i of its fftshifted form, any int i: (i - N / 2) mod N
__device__ __forceinline__ int unshift(int i, int N)
{
    int m = i % N - N / 2;            // in (-1.5 N, N)
    m %= N;
    return m < 0 ? m + N : m;
}

__global__ __launch_bounds__(THREADS) void register_logpolar_kernel(const float2* __restrict__ spectrum, int N,
                                                                    const float* __restrict__ ca, const float* __restrict__ sa,
                                                                    const float* __restrict__ rho, const float* __restrict__ wr,
                                                                    int A, int R, float2* __restrict__ out)
{
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= A * R) return;
    const int a = idx / R, r = idx - a * R;
    const float half = (float)(N / 2);
    const float x = fmaf(rho[r], ca[a], half), y = fmaf(rho[r], sa[a], half);
    const float x0f = floorf(x), y0f = floorf(y);
    float val = 0.f;
    if (fabsf(x0f) < 1e9f && fabsf(y0f) < 1e9f) {       // (tables are finite: a NaN or huge coordinate gives 0, never an index)
        const float fx = x - x0f, fy = y - y0f;
        const int xa = unshift((int)x0f, N), ya = unshift((int)y0f, N);
        const int xb = xa + 1 == N ? 0 : xa + 1, yb = ya + 1 == N ? 0 : ya + 1;
        const float2* F = spectrum + (size_t)blockIdx.y * N * N;
        const float2 v00 = F[(size_t)ya * N + xa], v01 = F[(size_t)ya * N + xb];
        const float2 v10 = F[(size_t)yb * N + xa], v11 = F[(size_t)yb * N + xb];
        const float m00 = log1pf(hypotf(v00.x, v00.y)), m01 = log1pf(hypotf(v01.x, v01.y));
        const float m10 = log1pf(hypotf(v10.x, v10.y)), m11 = log1pf(hypotf(v11.x, v11.y));
        const float top = fmaf(fx, m01 - m00, m00), bot = fmaf(fx, m11 - m10, m10);
        val = fmaf(fy, bot - top, top) * wr[r];
    }
    out[(size_t)blockIdx.y * A * R + idx] = make_float2(val, 0.f);
}

__global__ __launch_bounds__(THREADS) void register_cross_power_kernel(const float2* __restrict__ a, const float2* __restrict__ b,
                                                                       const int* __restrict__ group_offsets, int P, int hw,
                                                                       int accumulate, float2* __restrict__ out)
{
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= hw) return;
    const int g = blockIdx.y;
    const int p0 = max(group_offsets[g], 0), p1 = min(group_offsets[g + 1], P);
    float2* o = out + (size_t)g * hw + idx;
    float2 sum = make_float2(0.f, 0.f);
    if (idx != 0) {                                       // bin (0, 0) is 0: the mean is removed here
        if (accumulate) sum = *o;
        for (int p = p0; p < p1; ++p) {
            const float2 u = a[(size_t)p * hw + idx], v = b[(size_t)p * hw + idx];
            const float xr = fmaf(u.x, v.x, u.y * v.y), xi = fmaf(u.y, v.x, -(u.x * v.y));      // u conj(v)
            const float m = hypotf(xr, xi);
            if (m > 0.f) {
                sum.x += xr / m;
                sum.y += xi / m;
            }
        }
    }
    *o = sum;
}

struct Best { float v; int i; };
// the larger value; on a tie the smaller index (the first in row-major order)
__device__ __forceinline__ Best better(Best p, Best q) { return (q.v > p.v || (q.v == p.v && q.i < p.i)) ? q : p; }

__device__ __forceinline__ Best block_best(Best mine, Best* lds)
{
    const int tid = threadIdx.x;
    lds[tid] = mine;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) lds[tid] = better(lds[tid], lds[tid + s]);
        __syncthreads();
    }
    return lds[0];
}

__device__ __forceinline__ bool in_wrapped_block(int i, int w, int h, int py, int px)
{
    const int y = i / w, x = i - y * w;
    int dy = y - py, dx = x - px;
    dy = dy < 0 ? dy + h : dy;
    dx = dx < 0 ? dx + w : dx;
    return (dy <= 1 || dy == h - 1) && (dx <= 1 || dx == w - 1);
}

// stage 1: the best of one chunk of one plane.  EXCLUDE: without the wrapped 3 x 3 block around the plane's peak (out_i).
template <bool EXCLUDE>
__global__ __launch_bounds__(THREADS) void register_peak_chunk_kernel(const float* __restrict__ planes, int h, int w, int stride,
                                                                      const int* __restrict__ out_i, float* __restrict__ part_v,
                                                                      int* __restrict__ part_i)
{
    __shared__ Best lds[THREADS];
    const int g = blockIdx.y, hw = h * w;
    const float* src = planes + (size_t)g * hw * stride;
    const int begin = blockIdx.x * MP_REGISTER_PEAK_CHUNK, end = min(begin + MP_REGISTER_PEAK_CHUNK, hw);
    int py = 0, px = 0;
    if (EXCLUDE) { py = out_i[2 * g]; px = out_i[2 * g + 1]; }
    Best mine{-INFINITY, INT_MAX};
    for (int i = begin + threadIdx.x; i < end; i += THREADS) {
        if (EXCLUDE && in_wrapped_block(i, w, h, py, px)) continue;
        const float v = src[(size_t)i * stride];
        // ascending i: a later equal value never replaces; the first non-NaN value is taken even when it is -inf
        if (v > mine.v || (mine.i == INT_MAX && v == v)) mine = Best{v, i};
    }
    const Best r = block_best(mine, lds);
    if (threadIdx.x == 0) {
        part_v[g * gridDim.x + blockIdx.x] = r.v;
        part_i[g * gridDim.x + blockIdx.x] = r.i;
    }
}

__device__ __forceinline__ float parabola(float l, float c, float r)
{
    const float d = l - 2.f * c + r;
    return d == 0.f ? 0.f : 0.5f * (l - r) / d;
}

// stage 2: the best of a plane's chunks.  Round one writes the peak and its fit, round two (EXCLUDE) the second value.
template <bool EXCLUDE>
__global__ __launch_bounds__(THREADS) void register_peak_final_kernel(const float* __restrict__ planes, int h, int w, int stride,
                                                                      int chunks, const float* __restrict__ part_v,
                                                                      const int* __restrict__ part_i, int* __restrict__ out_i,
                                                                      float* __restrict__ out_f)
{
    __shared__ Best lds[THREADS];
    const int g = blockIdx.x;
    Best mine{-INFINITY, INT_MAX};
    for (int c = threadIdx.x; c < chunks; c += THREADS) mine = better(mine, Best{part_v[g * chunks + c], part_i[g * chunks + c]});
    const Best r = block_best(mine, lds);
    if (threadIdx.x != 0) return;
    if (EXCLUDE) {
        out_f[6 * g + 5] = r.i == INT_MAX ? -INFINITY : r.v;         // nothing outside the block (h, w <= 3): -inf
        return;
    }
    const int i = (r.i == INT_MAX || r.i < 0 || r.i >= h * w) ? 0 : r.i;      // (a plane of NaNs: position 0)
    const int py = i / w, px = i - py * w;
    const float* src = planes + (size_t)g * h * w * stride;
    auto at = [&](int y, int x) { return src[((size_t)y * w + x) * stride]; };
    const float c = at(py, px);
    const float oy = parabola(at(py == 0 ? h - 1 : py - 1, px), c, at(py == h - 1 ? 0 : py + 1, px));
    const float ox = parabola(at(py, px == 0 ? w - 1 : px - 1), c, at(py, px == w - 1 ? 0 : px + 1));
    out_i[2 * g] = py;
    out_i[2 * g + 1] = px;
    out_f[6 * g + 0] = oy;
    out_f[6 * g + 1] = ox;
    out_f[6 * g + 2] = (float)(py > h / 2 ? py - h : py) + oy;
    out_f[6 * g + 3] = (float)(px > w / 2 ? px - w : px) + ox;
    out_f[6 * g + 4] = c;
}

}  // namespace

void launch_register_prepare(const float* frames, const float* cs, const float* wy, const float* wx, int n, int H, int W, int N,
                             float* out, hipStream_t s)
{
    const dim3 grid((unsigned)(((long long)N * N + THREADS - 1) / THREADS), (unsigned)n);
    hipLaunchKernelGGL(register_prepare_kernel, grid, dim3(THREADS), 0, s, frames, cs, wy, wx, H, W, N,
                       reinterpret_cast<float2*>(out));
}

void launch_register_logpolar(const float* spectrum, int n, int N, const float* ca, const float* sa, const float* rho,
                              const float* wr, int A, int R, float* out, hipStream_t s)
{
    const dim3 grid((unsigned)(((long long)A * R + THREADS - 1) / THREADS), (unsigned)n);
    hipLaunchKernelGGL(register_logpolar_kernel, grid, dim3(THREADS), 0, s, reinterpret_cast<const float2*>(spectrum), N, ca, sa,
                       rho, wr, A, R, reinterpret_cast<float2*>(out));
}

void launch_register_cross_power(const float* a, const float* b, const int* group_offsets, int P, int G, int h, int w,
                                 int accumulate, float* out, hipStream_t s)
{
    const int hw = h * w;
    const dim3 grid((unsigned)((hw + THREADS - 1) / THREADS), (unsigned)G);
    hipLaunchKernelGGL(register_cross_power_kernel, grid, dim3(THREADS), 0, s, reinterpret_cast<const float2*>(a),
                       reinterpret_cast<const float2*>(b), group_offsets, P, hw, accumulate, reinterpret_cast<float2*>(out));
}

RegisterPeakWorkspace register_peak_workspace(void* partial, int G, int h, int w)
{
    Carver c(partial, alignof(float));
    RegisterPeakWorkspace ws{};
    ws.chunks = (h * w + MP_REGISTER_PEAK_CHUNK - 1) / MP_REGISTER_PEAK_CHUNK;
    ws.part_v = c.take<float>((size_t)G * ws.chunks);
    ws.part_i = c.take<int>((size_t)G * ws.chunks);
    ws.bytes = c.bytes();
    return ws;
}

void launch_register_peak(const float* planes, int G, int h, int w, int stride, int* out_i, float* out_f, void* partial,
                          hipStream_t s)
{
    const RegisterPeakWorkspace ws = register_peak_workspace(partial, G, h, w);
    const int chunks = ws.chunks;
    float* part_v = ws.part_v;
    int* part_i = ws.part_i;
    const dim3 grid((unsigned)chunks, (unsigned)G);
    hipLaunchKernelGGL(register_peak_chunk_kernel<false>, grid, dim3(THREADS), 0, s, planes, h, w, stride, out_i, part_v, part_i);
    hipLaunchKernelGGL(register_peak_final_kernel<false>, dim3(G), dim3(THREADS), 0, s, planes, h, w, stride, chunks, part_v, part_i,
                       out_i, out_f);
    hipLaunchKernelGGL(register_peak_chunk_kernel<true>, grid, dim3(THREADS), 0, s, planes, h, w, stride, out_i, part_v, part_i);
    hipLaunchKernelGGL(register_peak_final_kernel<true>, dim3(G), dim3(THREADS), 0, s, planes, h, w, stride, chunks, part_v, part_i,
                       out_i, out_f);
}
