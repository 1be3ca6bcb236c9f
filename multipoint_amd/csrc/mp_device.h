// Device primitives shared by the kernel sources of libmultipoint_hip.so (gfx950).  Internal header.
#pragma once
#include <hip/hip_runtime.h>

// ReflectionPad2d(1) index of row / column v of an n-pixel frame
__device__ __forceinline__ int reflect_clamp(int v, int n)
{
    v = v < 0 ? -v : v;                     // ReflectionPad2d(1): -1 -> 1
    v = v >= n ? 2 * (n - 1) - v : v;       //                      n -> n-2
    v = v < 0 ? 0 : v;
    return v >= n ? n - 1 : v;              // (only reachable for pixels outside the image tile)
}

// The padding rule of the 3x3 convolutions: the frame pixel that feeds position (gy, gx) of a halo, and whether that
// position is a zero instead (ZeroPad2d(1); the coordinates are then clamped into the frame, so a dummy load stays legal).
struct PadSource { int y, x; bool zero; };
__device__ __forceinline__ PadSource pad_source(int gy, int gx, int H, int W, int pad_zero)
{
    if (pad_zero) return {min(max(gy, 0), H - 1), min(max(gx, 0), W - 1), (bool)((gy < 0) | (gy >= H) | (gx < 0) | (gx >= W))};
    return {reflect_clamp(gy, H), reflect_clamp(gx, W), false};
}

// borderInterpolate(p, n, BORDER_REFLECT_101) with the reflection repeated while p stays outside (period 2n - 2): the modulo
// also keeps the rows and columns that a partial tile loads but never uses inside the frame
__device__ __forceinline__ int reflect101(int p, int n)
{
    if (n == 1) return 0;
    const int period = 2 * n - 2;
    int q = p % period;
    if (q < 0) q += period;
    return q < n ? q : period - q;
}

// The source position of cv2.warpPerspective(INTER_LINEAR) for destination pixel (x, y) under the inverted homography m[9], as
// OpenCV's WarpPerspectiveInvoker + remapBilinear<float> compute it: per row of a block of bw0 columns X0 = m0 xb + m1 y + m2
// (likewise Y0, W0) in float64, per pixel 32 / (W0 + m6 x1) and the coordinates rounded half-to-even to 1/32 pixel; the source
// pixel is that >> 5 saturated to int16, the fraction that & 31, and the four taps (sy, sx), (sy, sx + 1), (sy + 1, sx),
// (sy + 1, sx + 1) weigh w0..w3 from the float32 table.  Every product and sum is rounded separately, as OpenCV's scalar code
// does (hipcc's __dmul_rn / __fadd_rn wrappers are inline operators that carry their own `contract` flag, hence the pragma).
__device__ __forceinline__ int cv_fixed(double num, double w)
{
#pragma clang fp contract(off)
    double f = num * w;
    f = fmax(-2147483648.0, fmin(2147483647.0, f));
    return (int)rint(f);
}
struct CvWarpSource { int sx, sy; float w0, w1, w2, w3; };
__device__ __forceinline__ CvWarpSource cv_warp_source(const double* m, int x, int y, int bw0)
{
#pragma clang fp contract(off)
    const int xb = (x / bw0) * bw0;
    const double dxb = (double)xb, dx1 = (double)(x - xb), dy = (double)y;
    const double X0 = (m[0] * dxb + m[1] * dy) + m[2];
    const double Y0 = (m[3] * dxb + m[4] * dy) + m[5];
    const double W0 = (m[6] * dxb + m[7] * dy) + m[8];
    double w = W0 + m[6] * dx1;
    w = w != 0.0 ? 32.0 / w : 0.0;
    const int X = cv_fixed(X0 + m[0] * dx1, w);
    const int Y = cv_fixed(Y0 + m[3] * dx1, w);
    const int sx = max(-32768, min(32767, X >> 5)), sy = max(-32768, min(32767, Y >> 5));
    const float fx = (float)(X & 31) * (1.f / 32.f), fy = (float)(Y & 31) * (1.f / 32.f);
    const float ax = 1.f - fx, ay = 1.f - fy;
    return {sx, sy, ay * ax, ay * fx, fy * ax, fy * fx};
}

// the sum of v over the wave's 64 lanes, in every lane (a fixed butterfly: the same bits on every run)
__device__ __forceinline__ double wave_add(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// ReLU as an integer max (finite inputs): one v_max_i32, no NaN-canonicalising v_max_f32 in front of it
__device__ __forceinline__ float relu_bits(float v) { return __int_as_float(max(__float_as_int(v), 0)); }

// splitmix64 finaliser: the counter-based hash behind RANSAC sampling (homography.hip), label noise (losses.hip) and
// photometric noise (photometric.hip)
__device__ __forceinline__ unsigned long long mix64(unsigned long long z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// a double in [0, 1) with 53 random bits per (key, counter), counter-based (photometric.hip, shapes.hip)
__device__ __forceinline__ double hash_uniform(unsigned long long key, unsigned long long ctr)
{
    return (double)(mix64(key ^ mix64(ctr)) >> 11) * 0x1p-53;
}

// LDS-DMA: 64 lanes x DWORDS dwords from (uniform base + per-lane byte offset [+ OFF]) to LDS [lds_byte [+ M0ADD] [+ OFF] +
// 4 DWORDS lane, ...).  The immediate OFF moves the source AND the LDS destination, M0ADD the destination only.  M0 is
// compiler-reserved and not preserved around an asm statement: the statement sets it and restores it.
// hipcc pads no hazard inside an asm statement, and an SGPR base needs five wait states behind a VALU write: NOP is the s_nop
// in front of the load, LEAD > 0 opens the statement with s_nop LEAD (behind a wave-uniform branch the wait states must lie
// inside the branch's own block).  multipoint_amd/build.py checks the generated code of the sources that use this (DMA_SOURCES).
constexpr int LDS_DMA_NO_OFFSET = 1 << 13;      // OFF: the instruction without an offset field (13-bit signed: never a real one)
template <int DWORDS, int LEAD, int NOP, int OFF = LDS_DMA_NO_OFFSET, int M0ADD = 0, typename T>
__device__ __forceinline__ void lds_dma(const T* sbase, unsigned voff_bytes, unsigned lds_byte)
{
    static_assert(DWORDS == 1 || DWORDS == 4, "global_load_lds_dword or global_load_lds_dwordx4");
    unsigned keep;
    // an asm template is a string literal: one statement per variant of its text, all with the same operands
#define MP_LDS_DMA(LEAD_S, M0_S, LOAD_S, ...)                                                                                  \
    asm volatile(LEAD_S "s_mov_b32 %0, m0\n\t" M0_S "\n\ts_nop %4\n\t" LOAD_S "\n\ts_mov_b32 m0, %0"                          \
                 : "=&s"(keep) : "v"(voff_bytes), "s"(sbase), "s"(lds_byte), "n"(NOP), "n"(OFF), "n"(M0ADD), "n"(LEAD)       \
                 : __VA_ARGS__)
#define MP_LDS_DMA_M0(LEAD_S, LOAD_S)                                                                                          \
    if constexpr (M0ADD == 0 && OFF == LDS_DMA_NO_OFFSET) MP_LDS_DMA(LEAD_S, "s_mov_b32 m0, %3", LOAD_S " %1, %2", "memory"); \
    else if constexpr (M0ADD == 0) MP_LDS_DMA(LEAD_S, "s_mov_b32 m0, %3", LOAD_S " %1, %2 offset:%5", "memory");             \
    else if constexpr (OFF == LDS_DMA_NO_OFFSET) MP_LDS_DMA(LEAD_S, "s_add_u32 m0, %3, %6", LOAD_S " %1, %2", "memory", "scc"); \
    else MP_LDS_DMA(LEAD_S, "s_add_u32 m0, %3, %6", LOAD_S " %1, %2 offset:%5", "memory", "scc")
    if constexpr (LEAD == 0 && DWORDS == 4) { MP_LDS_DMA_M0("", "global_load_lds_dwordx4"); }
    else if constexpr (LEAD == 0) { MP_LDS_DMA_M0("", "global_load_lds_dword"); }
    else if constexpr (DWORDS == 4) { MP_LDS_DMA_M0("s_nop %7\n\t", "global_load_lds_dwordx4"); }
    else { MP_LDS_DMA_M0("s_nop %7\n\t", "global_load_lds_dword"); }
#undef MP_LDS_DMA_M0
#undef MP_LDS_DMA
}
// wait for every LDS-DMA (and every other vector-memory load) of the wave: hipcc counts none of the asm statements above
__device__ __forceinline__ void dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// byte address of an LDS array (the M0 / ds_* operand)
__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(size_t)p; }

// Phase timers of the -DMP_TIMING developer build (tools/conv_timing.py): a kernel keeps wave-uniform cycle sums in a local
// `unsigned long long tsum[]` and writes them to its table once per workgroup.  MP_CLOCK(var) reads the clock into a const,
// MP_CLOCK_ADD(slot, a, b) adds b - a to tsum[slot]; MP_TIMING_TABLE declares a kernel's table and its extern "C" reader,
// MP_TIMING_HEIGHT the input height whose launches are recorded and its setter.  All empty without MP_TIMING.
#ifdef MP_TIMING
#define MP_CLOCK(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#define MP_CLOCK_ADD(slot, a, b) do { tsum[slot] += (b) - (a); } while (0)
#define MP_TIMING_TABLE(table, n, reader)                                                                                      \
    __device__ unsigned long long table[n];                                                                                    \
    extern "C" int reader(unsigned long long* host, int cnt)                                                                   \
    {                                                                                                                          \
        return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(table), sizeof(unsigned long long) * cnt);                            \
    }
#define MP_TIMING_HEIGHT(sel, init, setter)                                                                                    \
    __device__ int sel = init;                                                                                                 \
    extern "C" int setter(int h) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(sel), &h, sizeof(int)); }
#else
#define MP_CLOCK(var) do { } while (0)
#define MP_CLOCK_ADD(slot, a, b) do { } while (0)
#define MP_TIMING_TABLE(table, n, reader)
#define MP_TIMING_HEIGHT(sel, init, setter)
#endif
