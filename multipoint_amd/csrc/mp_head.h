// The stages that the two fused head-tail kernels share (head_tail.hip: fp32, head_tail_f16.hip: fp16): parameter staging, tile
// placement, the detector tail behind the BatchNorm, the descriptor tail behind the BatchNorm, the launcher.  The kernels keep
// their main loops (double buffer / ring, MFMA type) and the step from an accumulator to a value.  Internal header.
//
// Lane mapping of both kernels: a lane owns ONE pixel (pl = lane & 31) and half (hf = lane >> 5) of every 32-channel block:
// register r of a block is channel (r&3) + 8*(r>>2) + 4*hf, so a register quad is 4 consecutive channels.
#pragma once
#include "mp_common.h"
#include "mp_device.h"

// bias | scale | shift of the NP = 96 + D output channels into prm[3][NP]: detector channels 0..95, the descriptor's behind
template <int NP, typename P>
__device__ __forceinline__ void head_stage_params(const P& p, float* prm, int tid)
{
    for (int i = tid; i < NP; i += 256) {
        const bool det = i < 96;
        const int c = det ? i : i - 96;
        prm[i] = det ? p.bdet[c] : p.bdesc[c];
        prm[NP + i] = det ? p.sdet[c] : p.sdesc[c];
        prm[2 * NP + i] = det ? p.tdet[c] : p.tdesc[c];
    }
}

// Where this lane's 16 bytes of tile t (128 consecutive pixels, 32 per wave) start: `base` is the tile's first pixel
// (wave-uniform), `off` the lane's byte offset from it.  Waves and lanes beyond the end re-read the last pixel.
template <typename T, typename P>
__device__ __forceinline__ void head_place(const P& p, long long t, int wave, int pl, int hf, unsigned& off, const T*& base)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    const long long q = (t * 4 + wave) * 32 + pl;
    off = (unsigned)(((q < p.npx ? q : p.npx - 1) - t * 128) * p.xstride + hf * VEC) * (unsigned)sizeof(T);
    base = p.x + t * 128 * p.xstride;
}

// the cell of pixel px: image b, cell index, cell row and column.  (Taken before the accumulators are read: the 64-bit
// divisions need registers of their own)
struct HeadCell { int b, cell, hc, wc; };
template <typename P>
__device__ __forceinline__ HeadCell head_cell(const P& p, long long px)
{
    const int cell = (int)(px % ((long long)p.Hc * p.Wc));
    const int b = (int)(px / ((long long)p.Hc * p.Wc));
    const int hc = cell / p.Wc;
    return {b, cell, hc, cell - hc * p.Wc};
}

// Detector tail of the pixel at `at`: v[16 t + r] = channel 32 t + (r&3) + 8*(r>>2) + 4*hf (t = 0, 1) behind bias and BatchNorm, d = the
// dustbin (channel 64) as the lower half-wave holds it.  Stores the logits and / or softmax over 65 channels -> drop the
// dustbin -> PixelShuffle(8).
template <typename P>
__device__ __forceinline__ void head_detector_tail(const P& p, const HeadCell& at, float (&v)[32], float d, bool valid, int pl, int hf)
{
    const int cell = at.cell, b = at.b, hc = at.hc, wc = at.wc;
    d = __shfl(d, pl);                                            // from lane pl (hf = 0): both halves need it
    if (p.logits_nchw && valid) {
        const long long plane = (long long)p.Hc * p.Wc;
        float* o = p.logits_nchw + (long long)b * 65 * plane + cell;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[(long long)(32 * t + (r & 3) + 8 * (r >> 2) + 4 * hf) * plane] = v[16 * t + r];
        if (hf == 0) o[64 * plane] = d;
    }
    if (p.prob) {
        // mode 0: nn.Softmax2d (max-subtracted); mode 1: SuperPointMagicLeap.generate_heatmap: exp(x) / (sum + 1e-5)
        float m = 0.f;
        if (p.softmax_mode == 0) {
            m = d;
#pragma unroll
            for (int i = 0; i < 32; ++i) m = fmaxf(m, v[i]);
            m = fmaxf(m, __shfl_xor(m, 32));
        }
        float s = 0.f;
#pragma unroll
        // __expf(x) = v_exp_f32(x * log2(e)): the rounded product costs a relative ln(2) * ulp(|x| * log2(e)) / 2, about 6.6e-7
        // (~6 ulp) at x = ln(1e-6); prob is measured within 1.3e-6 relative of float64 where it is >= 1e-6 (tests/test_gpu_exact.py)
        for (int i = 0; i < 32; ++i) { v[i] = __expf(v[i] - m); s += v[i]; }
        s += __shfl_xor(s, 32);
        s += __expf(d - m);
        if (p.softmax_mode == 1) s += 0.00001f;
        // one IEEE division per pixel instead of 32 (a division is a ten-instruction sequence): v * (1/s) is within
        // one ulp of v / s
        const float rs = 1.0f / s;
        if (valid) {
            const int H = p.Hc * 8, W = p.Wc * 8;
            float* o = p.prob + ((long long)b * H + hc * 8) * W + wc * 8 + 4 * hf;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    // channels 32t + 8q + 4hf + (0..3) = row dy = 4t + q of the 8x8 block, columns 4hf .. 4hf+3
                    const f32x4 o4 = {v[16 * t + 4 * q] * rs, v[16 * t + 4 * q + 1] * rs, v[16 * t + 4 * q + 2] * rs,
                                      v[16 * t + 4 * q + 3] * rs};
                    *reinterpret_cast<f32x4*>(o + (long long)(4 * t + q) * W) = o4;
                }
        }
    }
}

// Descriptor tail of pixel px: dv[4 t + q] = channels 32 t + 8 q + 4 hf + (0..3) behind bias and BatchNorm, ss = this lane's
// sum of their squares.  L2 normalisation (F.normalize) and the 16-byte stores of the row.
template <int ND, typename P>
__device__ __forceinline__ void head_descriptor_tail(const P& p, f32x4 (&dv)[ND * 4], float ss, long long px, bool valid, int hf)
{
    if (p.normalize) {
        ss += __shfl_xor(ss, 32);
        const float rd = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
        for (int i = 0; i < ND * 4; ++i) dv[i] = dv[i] * rd;
    }
    if (valid) {
        float* o = p.desc + px * (32 * ND) + 4 * hf;
#pragma unroll
        for (int t = 0; t < ND; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4*>(o + 32 * t + 8 * q) = dv[4 * t + q];
    }
}

// Host side: one persistent workgroup per CU walks the tiles; k0 / k2 / k4 / k8 are the kernel's instantiations for
// D = 0 (no descriptor head), 64, 128, 256.  Returns 1 when D is none of them (nothing is launched).
template <typename P>
inline int head_tail_launch(const P& p, hipStream_t s, void (*k0)(P), void (*k2)(P), void (*k4)(P), void (*k8)(P))
{
    const int D = p.desc ? p.D : 0;
    void (*const k)(P) = D == 0 ? k0 : D == 64 ? k2 : D == 128 ? k4 : D == 256 ? k8 : nullptr;
    if (!k) return 1;
    const long long tiles = (p.npx + 127) / 128;
    hipLaunchKernelGGL(k, dim3((unsigned)(tiles < p.ncu ? tiles : p.ncu)), dim3(256), 0, s, p);
    return 0;
}
