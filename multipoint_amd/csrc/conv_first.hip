// First encoder block: ReflectionPad2d(1) -> Conv2d(1, 64, 3) -> ReLU -> BatchNorm2d(64)
// (reference multipoint/models/MultiPoint.py:143-148 with N_in = 1, encoder modules 0-3).
// K = 9 only: arithmetic intensity 4.4 FLOP/B, i.e. bound by the 64-channel NHWC output write
// (78.6 MB per 480x640 image).  Direct VALU convolution: 16 lanes share one pixel, each lane owns
// 4 consecutive output channels whose 36 weights + bias/scale/shift live in registers; a wave
// writes 4 adjacent pixels = 1 KiB contiguous per store instruction.
// Two kernels: conv_first_kernel<C1, LINEAR, POOL> (NHWC; conv + bias only; with the 2x2 max-pool) and the planar one.  They
// share the tile decode and patch load of mp_tile.h (as do conv_f16.hip's first block and conv_mfma.hip's fused one), the
// window gather and ONE tap chain + activation (tap_chain_act).
#include "mp_common.h"
#include "mp_device.h"
#include "mp_tile.h"

namespace {

constexpr int TH = 8, TW = 32;              // output tile per workgroup
constexpr int LW = TW + 2, LH = TH + 2;

// the tile's image patch with its one-pixel halo (first_tile_decode / patch_load: mp_tile.h)
__device__ __forceinline__ FirstTile stage_patch(const Conv1Params& p, float* tile, int tid)
{
    const FirstTile t = first_tile_decode<TH, TW>(p, blockIdx.x);
    patch_load<TH, TW, 1>(tile, p.in + (long long)t.img * p.H * p.W, t.y0, t.x0, p.H, p.W, p.pad_zero, tid, [](float v) { return v; });
    return t;
}

// the 3x3 window of tile pixel (py, px)
__device__ __forceinline__ void window(const float* tile, int py, int px, float (&x)[9])
{
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) x[kh * 3 + kw] = tile[(py + kh) * LW + px + kw];
}

// one output channel of a pixel: the nine taps (weight of tap k: wk(k)) as one k-ordered fmaf chain, bias, then ReLU -> BatchNorm
// (bn_first: BatchNorm -> ReLU).  LINEAR: conv + bias only
template <bool LINEAR = false, typename WK>
__device__ __forceinline__ float tap_chain_act(const float (&x)[9], WK wk, float bias, float scale, float shift, int bn_first)
{
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) a = fmaf(x[k], wk(k), a);
    a += bias;
    if constexpr (!LINEAR) {
        if (bn_first) a = fmaxf(a * scale + shift, 0.f);
        else a = fmaxf(a, 0.f) * scale + shift;
    }
    return a;
}

// C1 = output channels (64, or 32 for channel_version 1 / 2): C1/4 lanes share a pixel.  LINEAR: conv + bias only (the
// batch-statistics forward of bn_first models: their BatchNorm needs the pre-ReLU output; scale / shift are not read).
// POOL: double_convolution: false (MultiPoint.py:147-148; generate_encoder :168-172): the block is followed directly by
// MaxPool2d(2,2) -- a lane evaluates the four pixels of one pooling window and stores their maximum: out [B][H/2][W/2][C1].
template <int C1, bool LINEAR, bool POOL>
__global__ __launch_bounds__(256) void conv_first_kernel(const Conv1Params p)
{
    __shared__ float tile[LH * LW];
    const int tid = threadIdx.x;
    const FirstTile t = stage_patch(p, tile, tid);
    const int img = t.img, y0 = t.y0, x0 = t.x0;

    // this lane's 4 output channels
    constexpr int LPP = C1 / 4;                   // lanes per pixel
    const int c4 = (tid % LPP) * 4;
    float w[9][4], bia[4], scl[4], sft[4];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p.w + k * C1 + c4);
#pragma unroll
        for (int e = 0; e < 4; ++e) w[k][e] = v[e];
    }
    {
        const f32x4 b = *reinterpret_cast<const f32x4*>(p.bias + c4);
        const f32x4 s = *reinterpret_cast<const f32x4*>(p.scale + c4);
        const f32x4 h = *reinterpret_cast<const f32x4*>(p.shift + c4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { bia[e] = b[e]; scl[e] = s[e]; sft[e] = h[e]; }
    }
    __syncthreads();

    auto pixel = [&](int py, int px) __attribute__((always_inline)) -> f32x4 {
        float x[9];
        window(tile, py, px, x);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            o[e] = tap_chain_act<LINEAR>(x, [&](int k) { return w[k][e]; }, bia[e], scl[e], sft[e], p.bn_first);
        return o;
    };
    constexpr int PPP = 256 / LPP;                // (pooled) pixels per pass
    const int psub = tid / LPP;
    if constexpr (POOL) {
        const int Ho = p.H >> 1, Wo = p.W >> 1;
        float* out = p.out + (long long)img * Ho * Wo * C1;
        for (int it = 0; it < (TH * TW / 4) / PPP; ++it) {
            const int pix = it * PPP + psub;
            const int qy = pix / (TW / 2), qx = pix % (TW / 2);
            f32x4 o = pixel(2 * qy, 2 * qx);
#pragma unroll
            for (int sub = 1; sub < 4; ++sub) {
                const f32x4 a = pixel(2 * qy + (sub >> 1), 2 * qx + (sub & 1));
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = fmaxf(o[e], a[e]);
            }
            const int oy = (y0 >> 1) + qy, ox = (x0 >> 1) + qx;
            if (oy < Ho && ox < Wo)
                *reinterpret_cast<f32x4*>(out + ((long long)oy * Wo + ox) * C1 + c4) = o;
        }
    } else {
        float* out = p.out + (long long)img * p.H * p.W * C1;
#pragma unroll 4
        for (int it = 0; it < (TH * TW) / PPP; ++it) {
            const int pix = it * PPP + psub;
            const int py = pix / TW, px = pix % TW;
            const f32x4 o = pixel(py, px);
            const int oy = y0 + py, ox = x0 + px;
            if (oy < p.H && ox < p.W)
                // streaming store: the 5 GB this layer writes per 64 images are read back once by the next layer, long after
                // they have left the caches (measured 0.91 vs 0.93 ms, and the next layer runs 0.5 % faster)
                __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(out + ((long long)oy * p.W + ox) * C1 + c4));
        }
    }
}

// The same block writing the channel-quad-planar layout [B][C1/4][H][W][4] that conv_wino43.hip consumes: a thread owns ONE pixel
// and walks the C1/4 channel quads (weights and bias / scale / shift of a quad are wave-uniform: LDS broadcast reads), so a
// store instruction writes two 512-byte row segments of one plane.  The multiply-add order is the NHWC kernel's.
template <int C1>
__global__ __launch_bounds__(256) void conv_first_planar_kernel(const Conv1Params p)
{
    __shared__ float tile[LH * LW];
    __shared__ __attribute__((aligned(16))) float wl[9 * C1], pl[3 * C1];
    const int tid = threadIdx.x;
    const FirstTile t = stage_patch(p, tile, tid);
    const int img = t.img, y0 = t.y0, x0 = t.x0;
    for (int f = tid; f < 9 * C1; f += 256) wl[f] = p.w[f];
    for (int f = tid; f < C1; f += 256) { pl[f] = p.bias[f]; pl[C1 + f] = p.scale[f]; pl[2 * C1 + f] = p.shift[f]; }
    __syncthreads();

    const int py = tid / TW, px = tid % TW;
    float x[9];
    window(tile, py, px, x);
    const int oy = y0 + py, ox = x0 + px;
    const bool ok = oy < p.H && ox < p.W;
    const long long plane = (long long)p.H * p.W * 4;
    float* out = p.out + (long long)img * (C1 / 4) * plane + ((long long)oy * p.W + ox) * 4;
#pragma unroll 4
    for (int q = 0; q < C1 / 4; ++q) {
        f32x4 wv[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) wv[k] = *reinterpret_cast<const f32x4*>(&wl[k * C1 + 4 * q]);
        const f32x4 b = *reinterpret_cast<const f32x4*>(&pl[4 * q]);
        const f32x4 sc = *reinterpret_cast<const f32x4*>(&pl[C1 + 4 * q]);
        const f32x4 sh = *reinterpret_cast<const f32x4*>(&pl[2 * C1 + 4 * q]);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            o[e] = tap_chain_act(x, [&](int k) { return wv[k][e]; }, b[e], sc[e], sh[e], p.bn_first);
        if (ok) __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(out + q * plane));
    }
}

// grid of both launchers: one workgroup per tile
long long first_blocks(const Conv1Params& p)
{
    return (long long)p.B * ((p.W + TW - 1) / TW) * ((p.H + TH - 1) / TH);
}

}  // namespace

void launch_conv_first(const Conv1Params& p, hipStream_t s)
{
    const long long nblk = first_blocks(p);
    if (nblk <= 0) return;
    if (p.pool) {
        if (p.channels == 32) hipLaunchKernelGGL((conv_first_kernel<32, false, true>), dim3((unsigned)nblk), dim3(256), 0, s, p);
        else hipLaunchKernelGGL((conv_first_kernel<64, false, true>), dim3((unsigned)nblk), dim3(256), 0, s, p);
        return;
    }
    if (p.out_planar) {
        if (p.channels == 32) hipLaunchKernelGGL(conv_first_planar_kernel<32>, dim3((unsigned)nblk), dim3(256), 0, s, p);
        else hipLaunchKernelGGL(conv_first_planar_kernel<64>, dim3((unsigned)nblk), dim3(256), 0, s, p);
        return;
    }
    if (p.channels == 32) hipLaunchKernelGGL((conv_first_kernel<32, false, false>), dim3((unsigned)nblk), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((conv_first_kernel<64, false, false>), dim3((unsigned)nblk), dim3(256), 0, s, p);
}

void launch_conv_first_linear(const Conv1Params& p, hipStream_t s)
{
    const long long nblk = first_blocks(p);
    if (nblk <= 0) return;
    if (p.channels == 32) hipLaunchKernelGGL((conv_first_kernel<32, true, false>), dim3((unsigned)nblk), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((conv_first_kernel<64, true, false>), dim3((unsigned)nblk), dim3(256), 0, s, p);
}
