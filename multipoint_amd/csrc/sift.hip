// SIFT baseline: Lowe (IJCV 2004) with the constants and conventions of opencv-contrib 4.2's sift.cpp, float
// build.  Gaussian scale space, 3-D extrema with ordered compaction, refinement + orientation and the 4 x 4 x 8 descriptor,
// batched over B images, wave64.  Nothing here uses a floating-point atomic: every sum has a fixed order, so results are
// bit-identical from run to run.
//
// Summation orders (the tests' error bounds and the run-to-run identity rest on them):
//   blur          row pass then column pass; each output acc = fma(w[k], x[k], acc) for k = 0 .. n-1 from acc = 0 (left to right,
//                 top to bottom); the row pass's result is rounded to fp32 in between
//   histograms    lane l of the keypoint's wave adds its samples l, l + 64, l + 128, .. (row-major over the window) into bins of
//                 its own in LDS; bin t is then the sum of the 64 lane copies in the order t, t + 1, .. 63, 0, .. t - 1 (mod 64)
//   norms         two values per lane squared and added, then a butterfly over the lanes (xor 1, 2, 4, .. 32)
#include "mp_common.h"
#include "mp_device.h"
#include "mp_select.h"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace {

constexpr int BT = 256;
constexpr int BTS = 1024;
constexpr int RMAX = MP_SIFT_MAX_TAPS / 2;      // 13
constexpr int POS_PER_BLOCK = BT * 4;           // candidate positions per workgroup
constexpr float PI_F = 3.14159265358979323846f;

// ---- scale space ------------------------------------------------------------------------------------------------------------

// SRC 0: a plane of the pyramid; 1: the 2x bilinear up-scale of the u8 frame (cv2.resize INTER_LINEAR: source coordinate
// (dst + 0.5) / 2 - 0.5, clamped -- weights 1/4 and 3/4, exact in fp32 on 8-bit values whatever the order); 2: the even rows and
// columns of a plane (sw: its width)
template <int SRC>
__device__ __forceinline__ float sift_src(const void* src, int y, int x, int sh, int sw)
{
    if constexpr (SRC == 0) return static_cast<const float*>(src)[(long long)y * sw + x];
    else if constexpr (SRC == 2) return static_cast<const float*>(src)[(long long)(2 * y) * sw + 2 * x];
    else {
        const unsigned char* im = static_cast<const unsigned char*>(src);
        // dst even: source floor = dst / 2 - 1, weight of the next pixel 3/4; odd: (dst - 1) / 2, weight 1/4
        int y0 = (y >> 1) - ((y & 1) ? 0 : 1), x0 = (x >> 1) - ((x & 1) ? 0 : 1);
        float wy = (y & 1) ? 0.25f : 0.75f, wx = (x & 1) ? 0.25f : 0.75f;
        if (y0 < 0) { y0 = 0; wy = 0.f; }
        if (y0 >= sh - 1) { y0 = sh - 1; wy = 0.f; }
        if (x0 < 0) { x0 = 0; wx = 0.f; }
        if (x0 >= sw - 1) { x0 = sw - 1; wx = 0.f; }
        const int y1 = min(y0 + 1, sh - 1), x1 = min(x0 + 1, sw - 1);
        const float a = (float)im[(long long)y0 * sw + x0] * (1.f - wx) + (float)im[(long long)y0 * sw + x1] * wx;
        const float c = (float)im[(long long)y1 * sw + x0] * (1.f - wx) + (float)im[(long long)y1 * sw + x1] * wx;
        return a * (1.f - wy) + c * wy;
    }
}

// row pass: out [b][y][x] = sum_k w[k] src(y, reflect101(x - r + k)); a workgroup takes 4 rows x 64 columns
template <int SRC>
__global__ __launch_bounds__(BT) void sift_row_blur_kernel(const void* __restrict__ src, long long src_stride, int sh, int sw,
                                                           float* __restrict__ out, int h, int w, SiftTaps taps)
{
    __shared__ float tile[4][64 + 2 * RMAX];
    const int r = taps.n >> 1, span = 64 + 2 * r;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 4, b = blockIdx.z;
    const void* plane = SRC == 1 ? (const void*)(static_cast<const unsigned char*>(src) + (long long)b * src_stride)
                                 : (const void*)(static_cast<const float*>(src) + (long long)b * src_stride);
    for (int i = threadIdx.x; i < 4 * span; i += BT) {
        const int ty = i / span, tx = i - ty * span;
        const int gy = min(y0 + ty, h - 1), gx = reflect101(x0 - r + tx, w);
        tile[ty][tx] = sift_src<SRC>(plane, gy, gx, sh, sw);
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= w || y >= h) return;
    float acc = 0.f;
    for (int k = 0; k < taps.n; ++k) acc = fmaf(taps.w[k], tile[ty][tx + k], acc);
    out[((long long)b * h + y) * w + x] = acc;
}

// column pass: out [b][y][x] = sum_k w[k] in(reflect101(y - r + k), x), and dog = out - prev when asked; 16 rows x 64 columns
__global__ __launch_bounds__(BT) void sift_col_blur_kernel(const float* __restrict__ in, float* __restrict__ out, long long out_stride,
                                                           const float* __restrict__ prev, float* __restrict__ dog,
                                                           long long dog_stride, int h, int w, SiftTaps taps)
{
    __shared__ float tile[16 + 2 * RMAX][64];
    const int r = taps.n >> 1, rows = 16 + 2 * r;
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 16, b = blockIdx.z;
    const float* plane = in + (long long)b * h * w;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int x = min(x0 + tx, w - 1);
    for (int i = ty; i < rows; i += 4) tile[i][tx] = plane[(long long)reflect101(y0 - r + i, h) * w + x];
    __syncthreads();
    if (x0 + tx >= w) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int yy = ty * 4 + e, y = y0 + yy;
        if (y >= h) break;
        float acc = 0.f;
        for (int k = 0; k < taps.n; ++k) acc = fmaf(taps.w[k], tile[yy + k][tx], acc);
        const long long at = (long long)y * w + x;
        out[(long long)b * out_stride + at] = acc;
        if (dog) dog[(long long)b * dog_stride + at] = acc - prev[(long long)b * out_stride + at];
    }
}

// ---- candidates -------------------------------------------------------------------------------------------------------------

struct SiftPos { int o, layer, r, c; };
__device__ __forceinline__ SiftPos sift_decode(const SiftLayout& L, long long flat)
{
    int o = 0;
    while (o + 1 < L.noct && flat >= L.flat[o + 1]) ++o;
    const int rem = (int)(flat - L.flat[o]), hw = L.h[o] * L.w[o];
    const int l = rem / hw, px = rem - l * hw;
    return {o, l + 1, px / L.w[o], px % L.w[o]};
}

// |v| > 1 and v >= (v > 0) or <= (v < 0) all 26 neighbours; both comparisons non-strict
__device__ __forceinline__ bool sift_is_extremum(const float* __restrict__ d, int h, int w, int r, int c)
{
    const long long hw = (long long)h * w;
    const float* p = d + (long long)r * w + c;
    const float v = *p;
    if (!(fabsf(v) > 1.0f)) return false;
    bool ge = true, le = true;
#pragma unroll
    for (int dl = -1; dl <= 1; ++dl)
#pragma unroll
        for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
            for (int dc = -1; dc <= 1; ++dc) {
                const float n = p[dl * hw + dr * w + dc];
                ge = ge && v >= n;
                le = le && v <= n;
            }
    return v > 0.f ? ge : le;
}

// one thread per four consecutive positions of (octave, layer 1..3, row, column): a 4-bit mask per thread and a count per workgroup
__global__ __launch_bounds__(BT) void sift_candidates_kernel(SiftLayout L, const float* __restrict__ ws_f, unsigned char* __restrict__ cmask,
                                                             int* __restrict__ seg_count)
{
    __shared__ int s_wave[BT / 64];
    const int b = blockIdx.y;
    const long long total = L.flat[L.noct];
    const long long first = (long long)blockIdx.x * POS_PER_BLOCK + threadIdx.x * 4;
    unsigned m = 0;
    for (int e = 0; e < 4; ++e) {
        const long long flat = first + e;
        if (flat >= total) break;
        const SiftPos p = sift_decode(L, flat);
        const int h = L.h[p.o], w = L.w[p.o];
        if (p.r < MP_SIFT_BORDER || p.r >= h - MP_SIFT_BORDER || p.c < MP_SIFT_BORDER || p.c >= w - MP_SIFT_BORDER) continue;
        const float* d = ws_f + L.dog[p.o] + ((long long)b * 5 + p.layer) * h * w;
        if (sift_is_extremum(d, h, w, p.r, p.c)) m |= 1u << e;
    }
    cmask[(long long)b * L.nblk * BT + (long long)blockIdx.x * BT + threadIdx.x] = (unsigned char)m;
    int tot;
    block_excl_scan<BT>(__popc(m), s_wave, &tot);
    if (threadIdx.x == 0) seg_count[b * L.nblk + blockIdx.x] = tot;
}

// per image: exclusive prefix of `count` [n] -> base [n]; the total goes to total [b], and past the capacity sets the flag
__global__ __launch_bounds__(BT) void sift_prefix_kernel(const int* __restrict__ count, int* __restrict__ base, int n, int* __restrict__ total,
                                                         int cap, int* __restrict__ flags, int flag)
{
    __shared__ int s_wave[BT / 64];
    const int b = blockIdx.x;
    int run = 0;
    for (int start = 0; start < n; start += BT) {
        const int i = start + threadIdx.x;
        const int c = i < n ? count[(long long)b * n + i] : 0;
        int tot;
        const int pre = block_excl_scan<BT>(c, s_wave, &tot);
        if (i < n) base[(long long)b * n + i] = run + pre;
        run += tot;
    }
    if (threadIdx.x == 0) {
        total[b] = run;
        if (run > cap) atomicOr(&flags[b], flag);
    }
}

__global__ __launch_bounds__(BT) void sift_compact_kernel(SiftLayout L, const unsigned char* __restrict__ cmask, const int* __restrict__ seg_base,
                                                          int4* __restrict__ cand)
{
    __shared__ int s_wave[BT / 64];
    const int b = blockIdx.y;
    const unsigned m = cmask[(long long)b * L.nblk * BT + (long long)blockIdx.x * BT + threadIdx.x];
    int tot;
    int pos = seg_base[b * L.nblk + blockIdx.x] + block_excl_scan<BT>(__popc(m), s_wave, &tot);
    const long long first = (long long)blockIdx.x * POS_PER_BLOCK + threadIdx.x * 4;
    for (int e = 0; e < 4; ++e)
        if (m & (1u << e)) {
            if (pos < L.cap) {
                const SiftPos p = sift_decode(L, first + e);
                cand[(long long)b * L.cap + pos] = make_int4(p.o, p.layer, p.r, p.c);
            }
            ++pos;
        }
}

// ---- refinement + orientation -----------------------------------------------------------------------------------------------

// x = A^-1 g by Gaussian elimination with partial pivoting (first largest pivot); false for a singular system
__device__ __forceinline__ bool sift_solve3(float A[3][3], float g[3], float x[3])
{
#pragma unroll
    for (int col = 0; col < 3; ++col) {
        int piv = col;
        float best = fabsf(A[col][col]);
#pragma unroll
        for (int r = col + 1; r < 3; ++r) {
            const float v = fabsf(A[r][col]);
            if (v > best) { best = v; piv = r; }
        }
        if (best == 0.f) return false;
#pragma unroll
        for (int r = col + 1; r < 3; ++r)
            if (piv == r) {
#pragma unroll
                for (int k = 0; k < 3; ++k) { const float t = A[col][k]; A[col][k] = A[r][k]; A[r][k] = t; }
                const float t = g[col]; g[col] = g[r]; g[r] = t;
            }
#pragma unroll
        for (int r = col + 1; r < 3; ++r) {
            const float f = A[r][col] / A[col][col];
#pragma unroll
            for (int k = col + 1; k < 3; ++k) A[r][k] -= f * A[col][k];
            g[r] -= f * g[col];
        }
    }
    x[2] = g[2] / A[2][2];
    x[1] = (g[1] - A[1][2] * x[2]) / A[1][1];
    x[0] = (g[0] - A[0][1] * x[1] - A[0][2] * x[2]) / A[0][0];
    return true;
}

// angle of (dx, dy) in degrees, [0, 360)
__device__ __forceinline__ float sift_angle(float dy, float dx)
{
    float a = atan2f(dy, dx) * (180.f / PI_F);
    if (a < 0.f) a += 360.f;
    return a >= 360.f ? 0.f : a;
}

// sum of the 64 lane copies of bin t (t < nbins at lane t): copies t, t + 1, .. in turn
__device__ __forceinline__ float sift_bin_sum(const float* hist, int t, int lane)
{
    float s = 0.f;
    for (int j = 0; j < 64; ++j) s += hist[t * 64 + ((j + lane) & 63)];
    return s;
}

// one wave per candidate: localisation (every lane the same arithmetic), then the 36-bin orientation histogram
__global__ __launch_bounds__(BT) void sift_refine_kernel(SiftLayout L, const float* __restrict__ ws_f, const int4* __restrict__ cand,
                                                         const int* __restrict__ cand_count, float* __restrict__ crec, int* __restrict__ cn,
                                                         float* __restrict__ cang, int4* __restrict__ cinfo)
{
    __shared__ float s_hist[BT / 64][36 * 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, b = blockIdx.y;
    const int idx = blockIdx.x * (BT / 64) + wv;
    const int ncand = min(cand_count[b], L.cap);
    bool live = idx < ncand;
    int o = 0, layer = 1, r = MP_SIFT_BORDER, c = MP_SIFT_BORDER;
    if (live) { const int4 q = cand[(long long)b * L.cap + idx]; o = q.x; layer = q.y; r = q.z; c = q.w; }
    const int h = L.h[o], w = L.w[o];
    const long long hw = (long long)h * w;
    const float* dogb = ws_f + L.dog[o] + (long long)b * 5 * hw;
    const float img_scale = 1.f / 255.f, deriv_scale = img_scale * 0.5f, second_scale = img_scale, cross_scale = img_scale * 0.25f;
    float xi = 0.f, xr = 0.f, xc = 0.f;
    bool converged = false;
    for (int it = 0; live && it < 5; ++it) {
        const float* img = dogb + layer * hw + (long long)r * w + c;
        const float *prv = img - hw, *nxt = img + hw;
        float g[3] = {(img[1] - img[-1]) * deriv_scale, (img[w] - img[-w]) * deriv_scale, (nxt[0] - prv[0]) * deriv_scale};
        const float v2 = img[0] * 2.f;
        const float dxx = (img[1] + img[-1] - v2) * second_scale, dyy = (img[w] + img[-w] - v2) * second_scale;
        const float dss = (nxt[0] + prv[0] - v2) * second_scale;
        const float dxy = (img[w + 1] - img[w - 1] - img[-w + 1] + img[-w - 1]) * cross_scale;
        const float dxs = (nxt[1] - nxt[-1] - prv[1] + prv[-1]) * cross_scale;
        const float dys = (nxt[w] - nxt[-w] - prv[w] + prv[-w]) * cross_scale;
        float A[3][3] = {{dxx, dxy, dxs}, {dxy, dyy, dys}, {dxs, dys, dss}};
        float X[3];
        if (!sift_solve3(A, g, X)) { live = false; break; }
        xc = -X[0]; xr = -X[1]; xi = -X[2];
        if (fabsf(xi) < 0.5f && fabsf(xr) < 0.5f && fabsf(xc) < 0.5f) { converged = true; break; }
        if (!(fabsf(xi) < 1e6f && fabsf(xr) < 1e6f && fabsf(xc) < 1e6f)) { live = false; break; }
        c += (int)rintf(xc); r += (int)rintf(xr); layer += (int)rintf(xi);
        if (layer < 1 || layer > 3 || c < MP_SIFT_BORDER || c >= w - MP_SIFT_BORDER || r < MP_SIFT_BORDER || r >= h - MP_SIFT_BORDER) live = false;
    }
    live = live && converged;
    float contr = 0.f;
    if (live) {
        const float* img = dogb + layer * hw + (long long)r * w + c;
        const float *prv = img - hw, *nxt = img + hw;
        const float gx = (img[1] - img[-1]) * deriv_scale, gy = (img[w] - img[-w]) * deriv_scale, gs = (nxt[0] - prv[0]) * deriv_scale;
        const float t = gx * xc + gy * xr + gs * xi;
        contr = img[0] * img_scale + t * 0.5f;
        if (fabsf(contr) * 3.f < 0.04f) live = false;
        const float v2 = img[0] * 2.f;
        const float dxx = (img[1] + img[-1] - v2) * second_scale, dyy = (img[w] + img[-w] - v2) * second_scale;
        const float dxy = (img[w + 1] - img[w - 1] - img[-w + 1] + img[-w - 1]) * cross_scale;
        const float tr = dxx + dyy, det = dxx * dyy - dxy * dxy;
        if (det <= 0.f || tr * tr * 10.f >= 121.f * det) live = false;
    }
    // the record, in doubled-base coordinates
    const float oscale = (float)(1 << o);
    const float size = 1.6f * exp2f(((float)layer + xi) / 3.f) * oscale * 2.f;
    float* hist = s_hist[wv];
    for (int i = lane; i < 36 * 64; i += 64) hist[i] = 0.f;
    __syncthreads();
    if (live) {
        const float scl = size * 0.5f / oscale;
        const int radius = (int)rintf(4.5f * scl);
        const float sigma = 1.5f * scl, expf_scale = -1.f / (2.f * sigma * sigma);
        const float* G = ws_f + L.gauss[o] + ((long long)b * MP_SIFT_LAYERS + layer) * hw;
        const int side = 2 * radius + 1;
        for (int s = lane; s < side * side; s += 64) {
            const int i = s / side - radius, j = s % side - radius;
            const int y = r + i, x = c + j;
            if (y <= 0 || y >= h - 1 || x <= 0 || x >= w - 1) continue;
            const float* p = G + (long long)y * w + x;
            const float dx = p[1] - p[-1], dy = p[-w] - p[w];
            const float wgt = expf((float)(i * i + j * j) * expf_scale);
            int bin = (int)rintf(sift_angle(dy, dx) * (36.f / 360.f));
            if (bin >= 36) bin -= 36;
            hist[bin * 64 + lane] += wgt * sqrtf(dx * dx + dy * dy);
        }
    }
    __syncthreads();
    const int t = lane < 36 ? lane : 0;
    const float raw = sift_bin_sum(hist, t, lane);
    // circular smoothing [1 4 6 4 1] / 16 over the 36 bins held by lanes 0 .. 35
    const float m1 = __shfl(raw, (t + 35) % 36), p1 = __shfl(raw, (t + 1) % 36), m2 = __shfl(raw, (t + 34) % 36), p2 = __shfl(raw, (t + 2) % 36);
    const float sm = (m2 + p2) * (1.f / 16.f) + (m1 + p1) * (4.f / 16.f) + raw * (6.f / 16.f);
    float mx = lane < 36 ? sm : 0.f;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    const float left = __shfl(sm, (t + 35) % 36), right = __shfl(sm, (t + 1) % 36);
    const bool peak = live && lane < 36 && sm > left && sm > right && sm >= mx * 0.8f;
    const unsigned long long peaks = __ballot(peak);
    if (!(idx < ncand)) return;
    const long long slot = (long long)b * L.cap + idx;
    if (peak) {
        float bin = (float)lane + 0.5f * (left - right) / (left - 2.f * sm + right);
        bin = bin < 0.f ? 36.f + bin : (bin >= 36.f ? bin - 36.f : bin);
        float angle = 360.f - 10.f * bin;
        if (fabsf(angle - 360.f) < FLT_EPSILON) angle = 0.f;
        cang[slot * MP_SIFT_MAX_ORI + __popcll(peaks & ((1ull << lane) - 1))] = angle;
    }
    if (lane == 0) {
        cn[slot] = __popcll(peaks);
        float* rec = crec + slot * 5;
        rec[0] = ((float)c + xc) * oscale;
        rec[1] = ((float)r + xr) * oscale;
        rec[2] = size;
        rec[3] = fabsf(contr);
        rec[4] = (float)(o * 8 + layer);
        // for the tests: where the refinement ended and which bins are peaks
        cinfo[slot] = make_int4(r, c, (int)(peaks & 0x3ffffull), (int)(peaks >> 18));
    }
}

// per image: the candidates' 0 .. n records each, in candidate order then bin order -> list [b][cap][6]
__global__ __launch_bounds__(BT) void sift_expand_kernel(SiftLayout L, const int* __restrict__ cand_count, const float* __restrict__ crec,
                                                         const int* __restrict__ cn, const float* __restrict__ cang, float* __restrict__ list,
                                                         int* __restrict__ list_count, int* __restrict__ flags)
{
    __shared__ int s_wave[BT / 64];
    const int b = blockIdx.x;
    const int ncand = min(cand_count[b], L.cap);
    int run = 0;
    for (int start = 0; start < ncand; start += BT) {
        const int i = start + threadIdx.x;
        const long long slot = (long long)b * L.cap + i;
        const int n = i < ncand ? cn[slot] : 0;
        int tot;
        int pos = run + block_excl_scan<BT>(n, s_wave, &tot);
        run += tot;
        for (int e = 0; e < n; ++e, ++pos)
            if (pos < L.cap) {
                float* out = list + ((long long)b * L.cap + pos) * 6;
                const float* rec = crec + slot * 5;
                out[0] = rec[0]; out[1] = rec[1]; out[2] = rec[2]; out[3] = cang[slot * MP_SIFT_MAX_ORI + e]; out[4] = rec[3]; out[5] = rec[4];
            }
    }
    if (threadIdx.x == 0) {
        list_count[b] = run;
        if (run > L.cap) atomicOr(&flags[b], MP_SIFT_FLAG_KEYPOINTS);
    }
}

// ---- selection --------------------------------------------------------------------------------------------------------------

// dup [b][i] = 1 when an earlier record of the list has the same x, y, size and angle
__global__ __launch_bounds__(BT) void sift_duplicates_kernel(const float* __restrict__ records, const int* __restrict__ rec_count, int M,
                                                             unsigned char* __restrict__ dup)
{
    __shared__ float4 s_rec[BT];
    const int b = blockIdx.y, n = min(rec_count[b], M);
    const int i0 = blockIdx.x * BT, i = i0 + threadIdx.x;
    if (i0 >= n) return;
    const float* rec = records + (long long)b * M * 6;
    float4 me = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n) me = make_float4(rec[i * 6LL], rec[i * 6LL + 1], rec[i * 6LL + 2], rec[i * 6LL + 3]);
    bool found = false;
    for (int j0 = 0; j0 <= i0; j0 += BT) {
        const int j = j0 + threadIdx.x;
        if (j < n) s_rec[threadIdx.x] = make_float4(rec[j * 6LL], rec[j * 6LL + 1], rec[j * 6LL + 2], rec[j * 6LL + 3]);
        __syncthreads();
        const int lim = min(BT, i - j0);            // earlier entries only (<= 0: none of this tile)
        for (int jj = 0; jj < lim; ++jj) {
            const float4 q = s_rec[jj];
            found = found || (q.x == me.x && q.y == me.y && q.z == me.z && q.w == me.w);
        }
        __syncthreads();
    }
    if (i < n) dup[(long long)b * M + i] = found ? 1 : 0;
}

// per image: of the records that are no duplicates, the k largest responses (a tie at the cut: the earlier one), in list order;
// x, y and size halved into frame coordinates
__global__ __launch_bounds__(BTS) void sift_select_kernel(const float* __restrict__ records, const int* __restrict__ rec_count, int M,
                                                          const unsigned char* __restrict__ dup, int k, int N, float* __restrict__ keypoints,
                                                          int* __restrict__ count)
{
    __shared__ int s_wave[BTS / 64];
    __shared__ unsigned s_hist[256];
    __shared__ unsigned s_sel[2];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(rec_count[b], M);
    const float* rec = records + (long long)b * M * 6;
    const unsigned char* dp = dup + (long long)b * M;
    auto key_at = [&](int i) { return dp[i] ? 0u : __float_as_uint(rec[i * 6LL + 4]); };      // responses are > 0: 0 is below all
    int nvalid = 0;
    for (int start = 0; start < n; start += BTS) {
        const int i = start + tid;
        int tot;
        block_excl_scan<BTS>(i < n && !dp[i] ? 1 : 0, s_wave, &tot);
        nvalid += tot;
    }
    unsigned T = 0;
    int need = 0;
    const bool select = nvalid > k;
    if (select) radix_select_cut<BTS>(key_at, n, k, s_hist, s_wave, s_sel, &T, &need);
    int out_base = 0, tie_base = 0;
    for (int start = 0; start < n; start += BTS) {
        const int i = start + tid;
        const bool valid = i < n && !dp[i];
        bool sel = valid;
        if (select) {
            const unsigned key = valid ? key_at(i) : 0u;
            const int eq = valid && key == T;
            int tot_eq;
            const int tie_rank = tie_base + block_excl_scan<BTS>(eq, s_wave, &tot_eq);
            tie_base += tot_eq;
            sel = valid && (key > T || (eq && tie_rank < need));
        }
        int tot;
        const int pos = out_base + block_excl_scan<BTS>(sel ? 1 : 0, s_wave, &tot);
        out_base += tot;
        if (sel && pos < N) {
            float* out = keypoints + ((long long)b * N + pos) * 6;
            const float* in = rec + i * 6LL;
            out[0] = in[0] * 0.5f; out[1] = in[1] * 0.5f; out[2] = in[2] * 0.5f; out[3] = in[3]; out[4] = in[4]; out[5] = in[5];
        }
    }
    const int kept = min(out_base, N);
    for (int i = kept * 6 + tid; i < N * 6; i += BTS) keypoints[(long long)b * N * 6 + i] = 0.f;
    if (tid == 0) count[b] = kept;
}

// ---- descriptor -------------------------------------------------------------------------------------------------------------

// one wave per keypoint slot: 4 x 4 x 8 trilinear histogram of the rotated, Gaussian-weighted gradients of the keypoint's layer
__global__ __launch_bounds__(64) void sift_describe_kernel(SiftLayout L, const float* __restrict__ ws_f, const float* __restrict__ keypoints,
                                                           const int* __restrict__ count, int N, float* __restrict__ desc)
{
    __shared__ float hist[128 * 64];
    const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    float* out = desc + ((long long)b * N + k) * 128;
    if (k >= min(count[b], N)) { out[lane] = 0.f; out[lane + 64] = 0.f; return; }
    const float* kp = keypoints + ((long long)b * N + k) * 6;
    const int code = (int)kp[5], o = min(max(code >> 3, 0), L.noct - 1), layer = min(max(code & 7, 0), MP_SIFT_LAYERS - 1);
    const int h = L.h[o], w = L.w[o];
    const float inv = 2.f / (float)(1 << o);            // frame coordinates -> this octave's pixels
    const int px = (int)rintf(kp[0] * inv), py = (int)rintf(kp[1] * inv);
    const float scl = kp[2] * inv * 0.5f;
    float ori = 360.f - kp[3];
    if (fabsf(ori - 360.f) < FLT_EPSILON) ori = 0.f;
    const float hist_width = 3.f * scl;
    int radius = (int)rintf(hist_width * 1.4142135623730951f * 5.f * 0.5f);
    radius = min(radius, (int)sqrtf((float)h * (float)h + (float)w * (float)w));
    const float cos_t = cosf(ori * (PI_F / 180.f)) / hist_width, sin_t = sinf(ori * (PI_F / 180.f)) / hist_width;
    const float* G = ws_f + L.gauss[o] + ((long long)b * MP_SIFT_LAYERS + layer) * h * w;
    for (int i = lane; i < 128 * 64; i += 64) hist[i] = 0.f;
    __syncthreads();
    const int side = 2 * radius + 1;
    for (int s = lane; s < side * side; s += 64) {
        const int i = s / side - radius, j = s % side - radius;
        const float c_rot = (float)j * cos_t - (float)i * sin_t, r_rot = (float)j * sin_t + (float)i * cos_t;
        float rbin = r_rot + 1.5f, cbin = c_rot + 1.5f;
        const int y = py + i, x = px + j;
        if (!(rbin > -1.f && rbin < 4.f && cbin > -1.f && cbin < 4.f && y > 0 && y < h - 1 && x > 0 && x < w - 1)) continue;
        const float* p = G + (long long)y * w + x;
        const float dx = p[1] - p[-1], dy = p[-w] - p[w];
        float obin = (sift_angle(dy, dx) - ori) * (8.f / 360.f);
        const float mag = sqrtf(dx * dx + dy * dy) * expf((c_rot * c_rot + r_rot * r_rot) * (-1.f / 8.f));
        const float r0f = floorf(rbin), c0f = floorf(cbin), o0f = floorf(obin);
        rbin -= r0f; cbin -= c0f; obin -= o0f;
        const int r0 = (int)r0f, c0 = (int)c0f;
        int o0 = (int)o0f;
        if (o0 < 0) o0 += 8;
        if (o0 >= 8) o0 -= 8;
        const float v_r1 = mag * rbin, v_r0 = mag - v_r1;
        const float v_rc11 = v_r1 * cbin, v_rc10 = v_r1 - v_rc11, v_rc01 = v_r0 * cbin, v_rc00 = v_r0 - v_rc01;
        const float v[2][2][2] = {{{v_rc00 - v_rc00 * obin, v_rc00 * obin}, {v_rc01 - v_rc01 * obin, v_rc01 * obin}},
                                  {{v_rc10 - v_rc10 * obin, v_rc10 * obin}, {v_rc11 - v_rc11 * obin, v_rc11 * obin}}};
#pragma unroll
        for (int dr = 0; dr < 2; ++dr)
#pragma unroll
            for (int dc = 0; dc < 2; ++dc)
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    const int rr = r0 + dr, cc = c0 + dc;
                    if (rr >= 0 && rr < 4 && cc >= 0 && cc < 4) hist[(((rr * 4 + cc) * 8) + ((o0 + d) & 7)) * 64 + lane] += v[dr][dc][d];
                }
    }
    __syncthreads();
    float a = sift_bin_sum(hist, lane, lane), c = sift_bin_sum(hist, lane + 64, lane);
    float n2 = a * a + c * c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) n2 += __shfl_xor(n2, off);
    const float thr = sqrtf(n2) * 0.2f;
    a = fminf(a, thr); c = fminf(c, thr);
    n2 = a * a + c * c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) n2 += __shfl_xor(n2, off);
    const float scale = 512.f / fmaxf(sqrtf(n2), FLT_EPSILON);
    out[lane] = fminf(fmaxf(rintf(a * scale), 0.f), 255.f);
    out[lane + 64] = fminf(fmaxf(rintf(c * scale), 0.f), 255.f);
}

// ---- adapter ----------------------------------------------------------------------------------------------------------------

// prob = 1 and owner = max list index at (round(y), round(x)) of every kept keypoint (prob zeroed, owner -1 beforehand)
__global__ __launch_bounds__(BT) void sift_scatter_kernel(const float* __restrict__ keypoints, const int* __restrict__ count, int N, int H, int W,
                                                          float* __restrict__ prob, int* __restrict__ owner)
{
    const int k = blockIdx.x * BT + threadIdx.x, b = blockIdx.y;
    if (k >= min(count[b], N)) return;
    const float* kp = keypoints + ((long long)b * N + k) * 6;
    const int x = (int)rintf(kp[0]), y = (int)rintf(kp[1]);
    if (x < 0 || x >= W || y < 0 || y >= H) return;
    const long long at = ((long long)b * H + y) * W + x;
    prob[at] = 1.f;
    atomicMax(&owner[at], k);
}

// weights exp(-x^2 / 2 s^2) in double, normalised by the double sum, rounded once; width round(8 s + 1) | 1
SiftTaps sift_taps(double sigma)
{
    SiftTaps t;
    t.n = (int)std::lrint(8.0 * sigma + 1.0) | 1;
    if (t.n > MP_SIFT_MAX_TAPS) t.n = MP_SIFT_MAX_TAPS;
    double wd[MP_SIFT_MAX_TAPS], sum = 0.0;
    const int r = t.n / 2;
    for (int i = 0; i < t.n; ++i) { wd[i] = std::exp(-(double)((i - r) * (i - r)) / (2.0 * sigma * sigma)); sum += wd[i]; }
    for (int i = 0; i < MP_SIFT_MAX_TAPS; ++i) t.w[i] = i < t.n ? (float)(wd[i] / sum) : 0.f;
    return t;
}

template <int SRC>
void row_blur(const void* src, long long src_stride, int sh, int sw, float* out, int B, int h, int w, const SiftTaps& t, hipStream_t s)
{
    hipLaunchKernelGGL(sift_row_blur_kernel<SRC>, dim3((w + 63) / 64, (h + 3) / 4, B), dim3(BT), 0, s, src, src_stride, sh, sw, out, h, w, t);
}

}  // namespace

void launch_sift_scale_space(const unsigned char* u8, const SiftLayout& L, void* ws, hipStream_t s)
{
    float* f = static_cast<float*>(ws);
    float* tmp = f + L.tmp;
    const double sigma0 = 1.6, k = std::pow(2.0, 1.0 / 3.0);
    for (int o = 0; o < L.noct; ++o) {
        const int h = L.h[o], w = L.w[o];
        const long long hw = (long long)h * w;
        float* g = f + L.gauss[o];
        float* d = f + L.dog[o];
        const dim3 gc((w + 63) / 64, (h + 15) / 16, L.B);
        for (int i = 0; i < MP_SIFT_LAYERS; ++i) {
            if (o > 0 && i == 0) {
                // the even rows and columns of layer 3 of the octave before: a copy (one tap of weight 1 in both passes is exact)
                SiftTaps one = sift_taps(1.0);
                one.n = 1; one.w[0] = 1.f;
                const int hp = L.h[o - 1], wp = L.w[o - 1];
                row_blur<2>(f + L.gauss[o - 1] + 3LL * hp * wp, MP_SIFT_LAYERS * (long long)hp * wp, hp, wp, tmp, L.B, h, w, one, s);
                hipLaunchKernelGGL(sift_col_blur_kernel, gc, dim3(BT), 0, s, tmp, g, MP_SIFT_LAYERS * hw, (const float*)nullptr, (float*)nullptr, 0LL, h, w, one);
                continue;
            }
            SiftTaps t;
            if (i == 0) {
                t = sift_taps(std::sqrt(std::max(sigma0 * sigma0 - 4.0 * 0.5 * 0.5, 0.01)));
                row_blur<1>(u8, (long long)L.H * L.W, L.H, L.W, tmp, L.B, h, w, t, s);
            } else {
                const double prev = sigma0 * std::pow(k, (double)(i - 1)), total = prev * k;
                t = sift_taps(std::sqrt(total * total - prev * prev));
                row_blur<0>(g + (i - 1) * hw, MP_SIFT_LAYERS * hw, h, w, tmp, L.B, h, w, t, s);
            }
            hipLaunchKernelGGL(sift_col_blur_kernel, gc, dim3(BT), 0, s, tmp, g + i * hw, MP_SIFT_LAYERS * hw,
                               i > 0 ? g + (i - 1) * hw : (const float*)nullptr, i > 0 ? d + (i - 1) * hw : (float*)nullptr, 5 * hw, h, w, t);
        }
    }
}

void launch_sift_detect(const SiftLayout& L, void* ws, int* flags, hipStream_t s)
{
    char* base = static_cast<char*>(ws);
    const float* f = static_cast<const float*>(ws);
    unsigned char* cmask = reinterpret_cast<unsigned char*>(base + L.cmask);
    int* seg_count = reinterpret_cast<int*>(base + L.seg_count);
    int* seg_base = reinterpret_cast<int*>(base + L.seg_base);
    int4* cand = reinterpret_cast<int4*>(base + L.cand);
    int* cand_count = reinterpret_cast<int*>(base + L.cand_count);
    float* crec = reinterpret_cast<float*>(base + L.crec);
    int* cn = reinterpret_cast<int*>(base + L.cn);
    float* cang = reinterpret_cast<float*>(base + L.cang);
    int4* cinfo = reinterpret_cast<int4*>(base + L.cinfo);
    float* list = reinterpret_cast<float*>(base + L.list);
    int* list_count = reinterpret_cast<int*>(base + L.list_count);
    (void)hipMemsetAsync(flags, 0, sizeof(int) * L.B, s);
    const dim3 gp(L.nblk, L.B);
    hipLaunchKernelGGL(sift_candidates_kernel, gp, dim3(BT), 0, s, L, f, cmask, seg_count);
    hipLaunchKernelGGL(sift_prefix_kernel, dim3(L.B), dim3(BT), 0, s, seg_count, seg_base, L.nblk, cand_count, L.cap, flags, MP_SIFT_FLAG_CANDIDATES);
    hipLaunchKernelGGL(sift_compact_kernel, gp, dim3(BT), 0, s, L, cmask, seg_base, cand);
    hipLaunchKernelGGL(sift_refine_kernel, dim3((L.cap + BT / 64 - 1) / (BT / 64), L.B), dim3(BT), 0, s, L, f, cand, cand_count, crec, cn, cang, cinfo);
    hipLaunchKernelGGL(sift_expand_kernel, dim3(L.B), dim3(BT), 0, s, L, cand_count, crec, cn, cang, list, list_count, flags);
}

void launch_sift_select(const float* records, const int* rec_count, int B, int M, int nfeatures, int N, float* keypoints, int* count,
                        unsigned char* dup, hipStream_t s)
{
    hipLaunchKernelGGL(sift_duplicates_kernel, dim3((M + BT - 1) / BT, B), dim3(BT), 0, s, records, rec_count, M, dup);
    hipLaunchKernelGGL(sift_select_kernel, dim3(B), dim3(BTS), 0, s, records, rec_count, M, dup, nfeatures, N, keypoints, count);
}

void launch_sift_describe(const SiftLayout& L, const void* ws, const float* keypoints, const int* count, int N, float* desc, hipStream_t s)
{
    hipLaunchKernelGGL(sift_describe_kernel, dim3(N, L.B), dim3(64), 0, s, L, static_cast<const float*>(ws), keypoints, count, N, desc);
}

void launch_sift_scatter(const float* keypoints, const int* count, int B, int N, int H, int W, float* prob, int* owner, hipStream_t s)
{
    (void)hipMemsetAsync(prob, 0, sizeof(float) * (size_t)B * H * W, s);
    (void)hipMemsetAsync(owner, 0xff, sizeof(int) * (size_t)B * H * W, s);
    hipLaunchKernelGGL(sift_scatter_kernel, dim3((N + BT - 1) / BT, B), dim3(BT), 0, s, keypoints, count, N, H, W, prob, owner);
}
