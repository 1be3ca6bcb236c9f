// Frame preparation (reference create_dataset/extract_images.py:167-242, ImageExtractorRos.preprocess_images):
// lens undistortion of 8-bit colour and 16-bit frames with the 180-degree rotation fused into the store, the 8-bit bilinear
// down-scale, and the percentile clip + min-max normalisation of the 16-bit thermal frame.  Every kernel works on a batch.
//
//   undistort_bgr8_kernel   one thread per destination pixel of the flat [n H W] range: the radial-tangential model in float64
//   undistort_u16_kernel    (+ - * / only, nothing contracted into FMA), the source position in 1/32 pixel, four taps with border
//                           0.  8 bit: 15-bit integer weights; a block's 256 pixels (768 bytes) are staged in LDS and stored as
//                           192 aligned dwords.  16 bit: float weights, round half even; a thread makes two neighbouring pixels
//                           and stores one dword.  rotate180 mirrors the DESTINATION index, so the stores stay in order.
//   resize_bgr8_kernel      cv2.resize's 11-bit fixed-point bilinear path, one thread per output pixel, the same staged store
//   tr_hist_hi_kernel       thermal rescale, pass 1: per image the histogram of the high byte (LDS histogram per block, runs of
//                           equal bytes among a thread's 8 pixels added at once, then one global atomic per non-empty bin)
//   tr_hist_lo_kernel       pass 2: every block scans the 256 counts, finds the high byte each of the four ranks falls in and
//                           histograms the low byte of the pixels that carry it -- four 256-bin histograms, one per rank
//   tr_bounds_kernel        one block per image: the four order statistics, numpy's interpolation between them in float64, the
//                           truncated bounds, cv2.normalize's scale and shift
//   tr_apply_kernel         clip, normalise (a separate fp32 multiply and add), the saved 16-bit form; 8 pixels per thread
//
// The order statistics are exact: integer counts, integer atomics.  After the clip the frame's minimum is trunc(lower) and its
// maximum trunc(upper) -- the order statistic below the lower bound exists in the frame and is moved onto trunc(lower), every
// pixel that stays is >= lower; likewise above -- so no further reduction pass is needed.  Without outlier rejection the ranks
// are 0 and N - 1: the bounds are the frame's minimum and maximum and the clip changes nothing.
#include "mp_common.h"

#include <climits>

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;

// ---------------------------------------------------------------------------------------------------------------- undistort
// rint(t), half to even, saturated to int32; NaN gives INT_MIN
__device__ __forceinline__ int round_fixed(double t)
{
    const double r = __builtin_rint(t);
    if (!(r >= -2147483648.0)) return INT_MIN;
    if (r > 2147483647.0) return INT_MAX;
    return (int)r;
}

// destination pixel (u, v) -> first tap (sx, sy) and the 1/32-pixel fractions
__device__ __forceinline__ void source_taps(const FramesCamera& c, int u, int v, int& sx, int& sy, int& ax, int& ay)
{
    const double x = ((double)u - c.ncx) / c.nfx;
    const double y = ((double)v - c.ncy) / c.nfy;
    const double r2 = x * x + y * y;
    const double kr = 1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2;
    const double xy2 = (2.0 * x) * y;
    const double xd = (x * kr + c.p1 * xy2) + c.p2 * (r2 + (2.0 * x) * x);
    const double yd = (y * kr + c.p1 * (r2 + (2.0 * y) * y)) + c.p2 * xy2;
    const int iu = round_fixed((c.fx * xd + c.cx) * 32.0);
    const int iv = round_fixed((c.fy * yd + c.cy) * 32.0);
    sx = iu >> 5, sy = iv >> 5, ax = iu & 31, ay = iv & 31;
}

// Pixel p0 + off of the flat [n][HW] range -> image and offset inside it.  p0 is the block's first pixel, so its division is
// one per wave on uniform values; off < span.  With HW >= span the lane's pixel lies in that image or the next one.
__device__ __forceinline__ void flat_pixel(long long p0, int off, int span, int HW, long long& img, int& rem)
{
    img = p0 / HW;
    long long r = p0 - img * HW + off;
    if (HW >= span) {
        if (r >= HW) r -= HW, ++img;
    } else {
        const long long k = r / HW;
        img += k, r -= k * HW;
    }
    rem = (int)r;
}

// offset `rem` inside a destination frame -> the (u, v) whose undistorted value it holds
__device__ __forceinline__ void dest_pixel(int rem, int H, int W, int rotate180, int& u, int& v)
{
    const int y = rem / W, x = rem - y * W;
    u = rotate180 ? W - 1 - x : x;
    v = rotate180 ? H - 1 - y : y;
}

// the block's 768 staged bytes as aligned dwords; the range's last bytes, where it is no multiple of four, one by one
__device__ __forceinline__ void store_staged(const unsigned* stage, unsigned char* dst, long long total_bytes)
{
    const int t = threadIdx.x;
    if (t >= THREADS * 3 / 4) return;
    const long long o = (long long)blockIdx.x * (THREADS * 3) + 4 * t;
    if (o + 4 <= total_bytes) {
        reinterpret_cast<unsigned*>(dst)[o >> 2] = stage[t];
    } else {
        const unsigned char* b = reinterpret_cast<const unsigned char*>(stage) + 4 * t;
        for (int j = 0; o + j < total_bytes; ++j) dst[o + j] = b[j];
    }
}

__global__ __launch_bounds__(THREADS) void undistort_bgr8_kernel(const unsigned char* __restrict__ src, long long total, int H, int W,
                                                                 FramesCamera cam, int rotate180, unsigned char* __restrict__ dst)
{
    __shared__ unsigned stage[THREADS * 3 / 4];
    const long long p = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (p < total) {
        long long img;
        int rem, u, v, sx, sy, ax, ay;
        flat_pixel((long long)blockIdx.x * THREADS, threadIdx.x, THREADS, H * W, img, rem);
        dest_pixel(rem, H, W, rotate180, u, v);
        source_taps(cam, u, v, sx, sy, ax, ay);
        const int w[4] = {(32 - ax) * (32 - ay) * 32, ax * (32 - ay) * 32, (32 - ax) * ay * 32, ax * ay * 32};
        int acc[3] = {0, 0, 0};
        const unsigned char* base = src + img * H * W * 3;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ty = sy + (k >> 1), tx = sx + (k & 1);
            if (ty >= 0 && ty < H && tx >= 0 && tx < W) {
                const unsigned char* px = base + ((long long)ty * W + tx) * 3;
                acc[0] += w[k] * px[0], acc[1] += w[k] * px[1], acc[2] += w[k] * px[2];
            }
        }
        unsigned char* o = reinterpret_cast<unsigned char*>(stage) + 3 * threadIdx.x;
        o[0] = (unsigned char)((acc[0] + 16384) >> 15);
        o[1] = (unsigned char)((acc[1] + 16384) >> 15);
        o[2] = (unsigned char)((acc[2] + 16384) >> 15);
    }
    __syncthreads();
    store_staged(stage, dst, total * 3);
}

__device__ __forceinline__ unsigned undistort_u16_pixel(const unsigned short* __restrict__ src, int off, int H, int W,
                                                        const FramesCamera& cam, int rotate180)
{
    long long img;
    int rem, u, v, sx, sy, ax, ay;
    flat_pixel(2 * (long long)blockIdx.x * THREADS, off, 2 * THREADS, H * W, img, rem);
    dest_pixel(rem, H, W, rotate180, u, v);
    source_taps(cam, u, v, sx, sy, ax, ay);
    const int w[4] = {(32 - ax) * (32 - ay), ax * (32 - ay), (32 - ax) * ay, ax * ay};
    const unsigned short* base = src + img * H * W;
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ty = sy + (k >> 1), tx = sx + (k & 1);
        const float val = (ty >= 0 && ty < H && tx >= 0 && tx < W) ? (float)base[(long long)ty * W + tx] : 0.0f;
        const float prod = ((float)w[k] / 1024.0f) * val;
        s = k == 0 ? prod : s + prod;
    }
    const float r = __builtin_rintf(s);
    return r <= 0.0f ? 0u : r >= 65535.0f ? 65535u : (unsigned)r;
}

__global__ __launch_bounds__(THREADS) void undistort_u16_kernel(const unsigned short* __restrict__ src, long long total, int H, int W,
                                                                FramesCamera cam, int rotate180, unsigned short* __restrict__ dst)
{
    const long long p = 2 * ((long long)blockIdx.x * THREADS + threadIdx.x);
    if (p >= total) return;
    const unsigned a = undistort_u16_pixel(src, 2 * threadIdx.x, H, W, cam, rotate180);
    if (p + 1 < total) {
        const unsigned b = undistort_u16_pixel(src, 2 * threadIdx.x + 1, H, W, cam, rotate180);
        reinterpret_cast<unsigned*>(dst)[p >> 1] = a | (b << 16);
    } else {
        dst[p] = (unsigned short)a;
    }
}

// ------------------------------------------------------------------------------------------------------------------- resize
__device__ __forceinline__ int sat16(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

// destination index d of an axis of n_in source pixels, scale = n_in / n_out: first source index, the two 11-bit weights
__device__ __forceinline__ void resize_coef(int d, int n_in, double scale, int& i, int& a0, int& a1)
{
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    i = (int)__builtin_floorf(f);
    f = f - (float)i;
    if (i < 0) i = 0, f = 0.0f;
    if (i >= n_in - 1) i = n_in - 1, f = 0.0f;
    a1 = sat16((int)__builtin_rintf(f * 2048.0f));
    a0 = sat16((int)__builtin_rintf((1.0f - f) * 2048.0f));
}

__global__ __launch_bounds__(THREADS) void resize_bgr8_kernel(const unsigned char* __restrict__ src, long long total, int H, int W,
                                                              int oh, int ow, double sy, double sx, unsigned char* __restrict__ dst)
{
    __shared__ unsigned stage[THREADS * 3 / 4];
    const long long p = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (p < total) {
        long long img;
        int rem;
        flat_pixel((long long)blockIdx.x * THREADS, threadIdx.x, THREADS, oh * ow, img, rem);
        const int y = rem / ow, x = rem - y * ow;
        int xi, a0, a1, yi, b0, b1;
        resize_coef(x, W, sx, xi, a0, a1);
        resize_coef(y, H, sy, yi, b0, b1);
        const int xj = xi + 1 < W ? xi + 1 : W - 1, yj = yi + 1 < H ? yi + 1 : H - 1;
        const unsigned char* base = src + img * H * W * 3;
        const unsigned char* r0 = base + (long long)yi * W * 3;
        const unsigned char* r1 = base + (long long)yj * W * 3;
        unsigned char* o = reinterpret_cast<unsigned char*>(stage) + 3 * threadIdx.x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int S0 = r0[xi * 3 + c] * a0 + r0[xj * 3 + c] * a1;
            const int S1 = r1[xi * 3 + c] * a0 + r1[xj * 3 + c] * a1;
            const int r = (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2;
            o[c] = (unsigned char)(r < 0 ? 0 : r > 255 ? 255 : r);
        }
    }
    __syncthreads();
    store_staged(stage, dst, total * 3);
}

// ----------------------------------------------------------------------------------------------------------- thermal rescale
constexpr int TR_PER = 8;           // pixels per thread and step of the vector paths (one 16-byte load)
constexpr int TR_MAX_BLOCKS = 1024; // blocks per image; the rest is a grid-stride loop

// per-image state in the caller's workspace (zeroed by the caller in front of every launch_thermal_rescale)
struct TrImage {
    unsigned hi[256];        // histogram of the high byte
    unsigned lo[4][256];     // histogram of the low byte among the pixels with high byte sel[k]
    int sel[4];              // the high byte rank k falls in
    unsigned resid[4];       // rank k minus the pixels below that high byte
    double lower, upper;     // np.percentile(x, 1), np.percentile(x, 99)
    unsigned tl, tu;         // the bounds as they land in the uint16 array
    float a, b;              // cv2.normalize: out = v a + b
};

__device__ __forceinline__ void unpack8(const uint4& q, unsigned v[TR_PER])
{
    v[0] = q.x & 0xffffu, v[1] = q.x >> 16, v[2] = q.y & 0xffffu, v[3] = q.y >> 16;
    v[4] = q.z & 0xffffu, v[5] = q.z >> 16, v[6] = q.w & 0xffffu, v[7] = q.w >> 16;
}

template <int VEC>
__global__ __launch_bounds__(THREADS) void tr_hist_hi_kernel(const unsigned short* __restrict__ in, int HW, TrImage* __restrict__ ws)
{
    __shared__ unsigned h[256];
    const int tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    const unsigned short* img = in + (long long)blockIdx.y * HW;
    if (VEC) {
        for (int c = blockIdx.x * THREADS + tid; c < HW / TR_PER; c += gridDim.x * THREADS) {
            unsigned v[TR_PER];
            unpack8(reinterpret_cast<const uint4*>(img)[c], v);
            unsigned cur = v[0] >> 8, cnt = 1;
#pragma unroll
            for (int j = 1; j < TR_PER; ++j) {
                const unsigned b = v[j] >> 8;
                if (b == cur) {
                    ++cnt;
                } else {
                    atomicAdd(&h[cur], cnt);
                    cur = b, cnt = 1;
                }
            }
            atomicAdd(&h[cur], cnt);
        }
    } else {
        for (int i = blockIdx.x * THREADS + tid; i < HW; i += gridDim.x * THREADS) atomicAdd(&h[img[i] >> 8], 1u);
    }
    __syncthreads();
    if (h[tid]) atomicAdd(&ws[blockIdx.y].hi[tid], h[tid]);
}

// inclusive scan of 256 counts held one per thread; returns this thread's inclusive sum
__device__ __forceinline__ unsigned scan256(unsigned* cum, unsigned v)
{
    const int tid = threadIdx.x;
    cum[tid] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const unsigned add = tid >= off ? cum[tid - off] : 0u;
        __syncthreads();
        cum[tid] += add;
        __syncthreads();
    }
    return cum[tid];
}

template <int VEC>
__global__ __launch_bounds__(THREADS) void tr_hist_lo_kernel(const unsigned short* __restrict__ in, int HW, FramesRanks rk,
                                                             TrImage* __restrict__ ws)
{
    __shared__ unsigned cum[256];
    __shared__ unsigned lo[4][256];
    __shared__ int sel[4];
    __shared__ unsigned resid[4];
    const int tid = threadIdx.x;
    TrImage& w = ws[blockIdx.y];
    if (tid < 4) sel[tid] = 0, resid[tid] = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) lo[k][tid] = 0;
    const unsigned count = w.hi[tid];
    const unsigned incl = scan256(cum, count), excl = incl - count;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (rk.rank[k] >= (long long)excl && rk.rank[k] < (long long)incl) sel[k] = tid, resid[k] = (unsigned)(rk.rank[k] - excl);
    __syncthreads();
    const unsigned s0 = sel[0], s1 = sel[1], s2 = sel[2], s3 = sel[3];
    const unsigned short* img = in + (long long)blockIdx.y * HW;
    auto take = [&](unsigned v) {
        const unsigned b = v >> 8, l = v & 255u;
        if (b == s0) atomicAdd(&lo[0][l], 1u);
        if (b == s1) atomicAdd(&lo[1][l], 1u);
        if (b == s2) atomicAdd(&lo[2][l], 1u);
        if (b == s3) atomicAdd(&lo[3][l], 1u);
    };
    if (VEC) {
        for (int c = blockIdx.x * THREADS + tid; c < HW / TR_PER; c += gridDim.x * THREADS) {
            unsigned v[TR_PER];
            unpack8(reinterpret_cast<const uint4*>(img)[c], v);
#pragma unroll
            for (int j = 0; j < TR_PER; ++j) take(v[j]);
        }
    } else {
        for (int i = blockIdx.x * THREADS + tid; i < HW; i += gridDim.x * THREADS) take(img[i]);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (lo[k][tid]) atomicAdd(&w.lo[k][tid], lo[k][tid]);
    if (blockIdx.x == 0 && tid < 4) w.sel[tid] = sel[tid], w.resid[tid] = resid[tid];
}

// numpy's _lerp on two order statistics a <= b
__device__ __forceinline__ double lerp_np(double a, double b, double t)
{
    const double diff = b - a;
    return t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;
}

__global__ __launch_bounds__(THREADS) void tr_bounds_kernel(FramesRanks rk, TrImage* __restrict__ ws)
{
    __shared__ unsigned cum[256];
    __shared__ unsigned val[4];
    const int tid = threadIdx.x;
    TrImage& w = ws[blockIdx.x];
    if (tid < 4) val[tid] = (unsigned)w.sel[tid] << 8;
    __syncthreads();
    for (int k = 0; k < 4; ++k) {
        const unsigned count = w.lo[k][tid];
        const unsigned incl = scan256(cum, count), excl = incl - count;
        const unsigned r = w.resid[k];
        if (r >= excl && r < incl) val[k] = ((unsigned)w.sel[k] << 8) | (unsigned)tid;
        __syncthreads();
    }
    if (tid == 0) {
        const double lower = lerp_np((double)val[0], (double)val[1], rk.gamma[0]);
        const double upper = lerp_np((double)val[2], (double)val[3], rk.gamma[1]);
        const unsigned tl = (unsigned)lower, tu = (unsigned)upper;
        const double smin = (double)tl, smax = (double)tu;
        const double scale = smax - smin > 2.220446049250313e-16 ? 1.0 / (smax - smin) : 0.0;
        const double shift = -smin * scale;
        w.lower = lower, w.upper = upper, w.tl = tl, w.tu = tu;
        w.a = (float)scale, w.b = (float)shift;
    }
}

struct TrOut {
    unsigned clipped, saved;
    float rescaled;
};

__device__ __forceinline__ TrOut tr_pixel(unsigned v, double lower, double upper, unsigned tl, unsigned tu, float a, float b)
{
    TrOut o;
    unsigned c = (double)v < lower ? tl : v;
    c = (double)c > upper ? tu : c;
    float r = (float)c * a;
    r = r + b;
    o.clipped = c, o.rescaled = r;
    o.saved = (unsigned)((int)(r * 65535.0f)) & 0xffffu;
    return o;
}

template <int VEC>
__global__ __launch_bounds__(THREADS) void tr_apply_kernel(const unsigned short* in, int HW, const TrImage* __restrict__ ws,
                                                           unsigned short* clipped, float* __restrict__ rescaled,
                                                           unsigned short* __restrict__ saved)
{
    const TrImage& w = ws[blockIdx.y];
    const double lower = w.lower, upper = w.upper;
    const unsigned tl = w.tl, tu = w.tu;
    const float a = w.a, b = w.b;
    const long long base = (long long)blockIdx.y * HW;
    if (VEC) {
        for (int c = blockIdx.x * THREADS + threadIdx.x; c < HW / TR_PER; c += gridDim.x * THREADS) {
            unsigned v[TR_PER];
            unpack8(reinterpret_cast<const uint4*>(in + base)[c], v);
            unsigned cl[TR_PER], sv[TR_PER];
            float rs[TR_PER];
#pragma unroll
            for (int j = 0; j < TR_PER; ++j) {
                const TrOut o = tr_pixel(v[j], lower, upper, tl, tu, a, b);
                cl[j] = o.clipped, sv[j] = o.saved, rs[j] = o.rescaled;
            }
            if (clipped)
                reinterpret_cast<uint4*>(clipped + base)[c] =
                    make_uint4(cl[0] | cl[1] << 16, cl[2] | cl[3] << 16, cl[4] | cl[5] << 16, cl[6] | cl[7] << 16);
            float4* ro = reinterpret_cast<float4*>(rescaled + base) + 2 * (long long)c;
            ro[0] = make_float4(rs[0], rs[1], rs[2], rs[3]);
            ro[1] = make_float4(rs[4], rs[5], rs[6], rs[7]);
            if (saved)
                reinterpret_cast<uint4*>(saved + base)[c] =
                    make_uint4(sv[0] | sv[1] << 16, sv[2] | sv[3] << 16, sv[4] | sv[5] << 16, sv[6] | sv[7] << 16);
        }
    } else {
        for (int i = blockIdx.x * THREADS + threadIdx.x; i < HW; i += gridDim.x * THREADS) {
            const TrOut o = tr_pixel(in[base + i], lower, upper, tl, tu, a, b);
            if (clipped) clipped[base + i] = (unsigned short)o.clipped;
            rescaled[base + i] = o.rescaled;
            if (saved) saved[base + i] = (unsigned short)o.saved;
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

void launch_undistort(const void* src, int u16, int n, int H, int W, const FramesCamera& cam, int rotate180, void* dst, hipStream_t s)
{
    const long long total = (long long)n * H * W;
    if (u16) {
        const long long threads = (total + 1) / 2;
        undistort_u16_kernel<<<(unsigned)((threads + THREADS - 1) / THREADS), THREADS, 0, s>>>(
            static_cast<const unsigned short*>(src), total, H, W, cam, rotate180, static_cast<unsigned short*>(dst));
    } else {
        undistort_bgr8_kernel<<<(unsigned)((total + THREADS - 1) / THREADS), THREADS, 0, s>>>(
            static_cast<const unsigned char*>(src), total, H, W, cam, rotate180, static_cast<unsigned char*>(dst));
    }
}

void launch_resize_bgr8(const unsigned char* src, int n, int H, int W, int oh, int ow, unsigned char* dst, hipStream_t s)
{
    const long long total = (long long)n * oh * ow;
    resize_bgr8_kernel<<<(unsigned)((total + THREADS - 1) / THREADS), THREADS, 0, s>>>(src, total, H, W, oh, ow, (double)H / (double)oh,
                                                                                      (double)W / (double)ow, dst);
}

size_t thermal_rescale_workspace_bytes(int n) { return (size_t)n * sizeof(TrImage); }

void launch_thermal_rescale(const unsigned short* in, int n, int H, int W, const FramesRanks& rk, unsigned short* clipped,
                            float* rescaled, unsigned short* saved, void* workspace, hipStream_t s)
{
    const int HW = H * W;
    TrImage* ws = static_cast<TrImage*>(workspace);
    const bool vec = HW % TR_PER == 0 && aligned16(in) && aligned16(rescaled) && (!clipped || aligned16(clipped)) &&
                     (!saved || aligned16(saved));
    const int per_block = THREADS * (vec ? TR_PER : 1);
    int bx = (HW + per_block - 1) / per_block;
    if (bx > TR_MAX_BLOCKS) bx = TR_MAX_BLOCKS;
    const dim3 grid(bx, n);
    if (vec) {
        tr_hist_hi_kernel<1><<<grid, THREADS, 0, s>>>(in, HW, ws);
        tr_hist_lo_kernel<1><<<grid, THREADS, 0, s>>>(in, HW, rk, ws);
        tr_bounds_kernel<<<n, THREADS, 0, s>>>(rk, ws);
        tr_apply_kernel<1><<<grid, THREADS, 0, s>>>(in, HW, ws, clipped, rescaled, saved);
    } else {
        tr_hist_hi_kernel<0><<<grid, THREADS, 0, s>>>(in, HW, ws);
        tr_hist_lo_kernel<0><<<grid, THREADS, 0, s>>>(in, HW, rk, ws);
        tr_bounds_kernel<<<n, THREADS, 0, s>>>(rk, ws);
        tr_apply_kernel<0><<<grid, THREADS, 0, s>>>(in, HW, ws, clipped, rescaled, saved);
    }
}
