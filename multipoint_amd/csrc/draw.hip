// Result views (include/multipoint_hip.h): fp32 frames as grey RGB pixels, keypoint marks, match pictures and
// alignment overlays on uint8 RGB canvases [B][Hc][Wc][3] the caller owns.  Kernels and their C ABI.
//
//   draw_gray_kernel / draw_compose_kernel   one thread per four pixels of a row; whole dwords where the twelve bytes are aligned
//   draw_marks_kernel      one workgroup per 16 x 16 canvas tile: the marks that touch the tile are listed in LDS in chunks of
//                          LIST_CAP, each pixel takes the colour of the highest-index mark covering it (shapes_blobs_kernel's
//                          rule) -- a gather, so the result does not depend on the launch
//   draw_matches_scatter_kernel   one workgroup per match: its two rings (the lanes share the rows) and its LINE_8 segment
//                          (lane 0 walks it) are written as atomicMax(index + 1) into the handle's owner map
//   draw_resolve_kernel    every canvas pixel with an owner takes that match's colour
//   draw_segments_scatter_kernel / draw_segments_resolve_kernel   the same two steps for a list of segments per canvas: the
//                          LineIterator walk, every pixel widened to a t x t box, each segment in the colour it names
// Every pixel write is checked against the canvas; centres and offsets are added in 64 bits.
#include "host.h"
#include "mp_raster.h"

#include <cstdint>

#pragma clang fp contract(off)

using namespace mp_host;
using namespace mp_raster;

namespace {

constexpr int TILE = 16;                // mark tile: 16 x 16 pixels, one per thread
constexpr int LIST_CAP = 1024;          // marks listed per pass over a tile
constexpr int HALF_N = MP_DRAW_MAX_RADIUS + 1;
constexpr int MAX_LIST = 1 << 20;       // longest keypoint list (K)
constexpr long long MAX_PIXELS = 1LL << 38;      // per call: the flat index of a launch stays below 2^31 blocks

// the 8-bit value of a fp32 one: NaN -> 0, clamped to [0, 1], (uint8)(c * 255.0f) truncated -- numpy's
// (np.clip(x, 0, 1) * 255.0).astype(np.uint8)
__device__ __forceinline__ int to_u8(float g)
{
    float c = g != g ? 0.f : g;
    c = c < 0.f ? 0.f : c > 1.f ? 1.f : c;
    return (int)(c * 255.0f);
}

// n <= 4 consecutive pixels of row y of canvas image b from column x on, each clipped to the canvas
__device__ __forceinline__ void store_pixels(unsigned char* canvas, int Hc, int Wc, int b, long long y, long long x, int n,
                                             const unsigned char (*rgb)[3])
{
    if (y < 0 || y >= Hc) return;
    unsigned char* row = canvas + ((long long)b * Hc + y) * Wc * 3;
    if (n == 4 && x >= 0 && x + 3 < Wc && (reinterpret_cast<uintptr_t>(row + 3 * x) & 3) == 0) {
        unsigned w[3];
        const unsigned char* f = &rgb[0][0];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            w[k] = (unsigned)f[4 * k] | (unsigned)f[4 * k + 1] << 8 | (unsigned)f[4 * k + 2] << 16 | (unsigned)f[4 * k + 3] << 24;
        unsigned* d = reinterpret_cast<unsigned*>(row + 3 * x);
        d[0] = w[0], d[1] = w[1], d[2] = w[2];
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {                            // (unrolled: rgb stays in registers)
        const long long xx = x + k;
        if (k >= n || xx < 0 || xx >= Wc) continue;
        row[3 * xx] = rgb[k][0], row[3 * xx + 1] = rgb[k][1], row[3 * xx + 2] = rgb[k][2];
    }
}

// four-pixel group g of a [B][H][W] frame: image, row, first column, pixels in it
__device__ __forceinline__ bool pixel_group(long long g, int B, int H, int W, int& b, int& y, int& x, int& n)
{
    const int groups = (W + 3) / 4;
    if (g >= (long long)B * H * groups) return false;
    x = (int)(g % groups) * 4;
    const long long r = g / groups;
    y = (int)(r % H), b = (int)(r / H);
    n = min(4, W - x);
    return true;
}

__global__ __launch_bounds__(256) void draw_gray_kernel(const float* in, const float* mask, int B, int H, int W, float gain,
                                                        unsigned char* canvas, int Hc, int Wc, int y0, int x0)
{
    int b, y, x, n;
    if (!pixel_group((long long)blockIdx.x * blockDim.x + threadIdx.x, B, H, W, b, y, x, n)) return;
    const long long at = ((long long)b * H + y) * W + x;
    unsigned char rgb[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k >= n) break;
        float v = in[at + k];
        if (mask) v = v * mask[at + k];
        const int u = to_u8(v * gain);
        rgb[k][0] = rgb[k][1] = rgb[k][2] = (unsigned char)u;
    }
    store_pixels(canvas, Hc, Wc, b, (long long)y + y0, (long long)x + x0, n, rgb);
}

__global__ __launch_bounds__(256) void draw_compose_kernel(const float* a, const float* t, int B, int H, int W, int mode, int alpha,
                                                           int cell, unsigned char* canvas, int Hc, int Wc, int y0, int x0)
{
    int b, y, x, n;
    if (!pixel_group((long long)blockIdx.x * blockDim.x + threadIdx.x, B, H, W, b, y, x, n)) return;
    const long long at = ((long long)b * H + y) * W + x;
    unsigned char rgb[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k >= n) break;
        const float av = a[at + k];
        const bool outside = av < 0.f;                       // the -1 border of the warp
        const int A = outside ? 0 : to_u8(av), T = to_u8(t[at + k]);
        int r, g, bl;
        if (mode == MP_DRAW_ANAGLYPH) {
            r = A, g = T, bl = T;
        } else {
            int v;
            if (outside) v = T;
            else if (mode == MP_DRAW_BLEND) v = (A * alpha + T * (256 - alpha) + 128) >> 8;
            else if (mode == MP_DRAW_CHECKER) v = (((x + k) / cell + y / cell) & 1) ? T : A;
            else v = abs(A - T);
            r = g = bl = v;
        }
        rgb[k][0] = (unsigned char)r, rgb[k][1] = (unsigned char)g, rgb[k][2] = (unsigned char)bl;
    }
    store_pixels(canvas, Hc, Wc, b, (long long)y + y0, (long long)x + x0, n, rgb);
}

// the half widths of the outer disc (radius ro) and of the inner one (ri, none when negative), by one lane
__device__ __forceinline__ void ring_tables(int ro, int ri, short* half_o, short* half_i)
{
    if (threadIdx.x == 0) {
        circle_halfwidths(ro, half_o);
        if (ri >= 0) circle_halfwidths(ri, half_i);
    }
}

// one workgroup per canvas tile; the image's marks are listed LIST_CAP at a time
__global__ __launch_bounds__(TILE * TILE) void draw_marks_kernel(const int* kp, const int* counts, int K, int kind, int ro, int ri,
                                                                 int y0, int x0, const unsigned char* palette, int npal,
                                                                 unsigned char* canvas, int Hc, int Wc)
{
    __shared__ int list[LIST_CAP];
    __shared__ int count;
    __shared__ short half_o[HALF_N], half_i[HALF_N];
    const int b = blockIdx.z, tid = threadIdx.x;
    const int n = min(max(counts[b], 0), K);
    if (kind != MP_DRAW_CROSS) ring_tables(ro, ri, half_o, half_i);
    const int tx = blockIdx.x * TILE, ty = blockIdx.y * TILE;
    const int px = tx + tid % TILE, py = ty + tid / TILE;
    const bool inside = px < Wc && py < Hc;
    const int* pts = kp + (long long)b * K * 2;
    int best = -1;
    for (int base = 0; base < n; base += LIST_CAP) {         // (n is the same in every lane of the workgroup)
        __syncthreads();                                     // the tables are written, the previous list is read
        if (tid == 0) count = 0;
        __syncthreads();
        const int end = min(base + LIST_CAP, n);
        for (int i = base + tid; i < end; i += blockDim.x) {
            const long long cy = (long long)pts[2 * i] + y0, cx = (long long)pts[2 * i + 1] + x0;
            if (cx + ro >= tx && cx - ro < tx + TILE && cy + ro >= ty && cy - ro < ty + TILE) list[atomicAdd(&count, 1)] = i;
        }
        __syncthreads();
        if (!inside) continue;
        for (int j = 0; j < count; ++j) {
            const int i = list[j];
            if (i < best) continue;
            const long long dy = llabs((long long)py - ((long long)pts[2 * i] + y0));
            const long long dx = llabs((long long)px - ((long long)pts[2 * i + 1] + x0));
            if (dy > ro || dx > ro) continue;
            bool covered;
            if (kind == MP_DRAW_CROSS) covered = dy == 0 || dx == 0;
            else covered = dx <= half_o[dy] && !(dy <= ri && dx <= half_i[dy]);
            if (covered) best = i;
        }
    }
    if (best < 0 || !inside) return;
    const unsigned char* c = palette + 3 * (best % npal);
    unsigned char* d = canvas + (((long long)b * Hc + py) * Wc + px) * 3;
    d[0] = c[0], d[1] = c[1], d[2] = c[2];
}

__global__ __launch_bounds__(64) void draw_matches_scatter_kernel(const int* kpA, const int* kpB, const int* countA,
                                                                  const int* countB, const int* match_idx,
                                                                  const unsigned char* mask, int K, int yA, int xA, int yB, int xB,
                                                                  int ro, int ri, unsigned* owner, int Hc, int Wc)
{
    const int p = blockIdx.y, q = blockIdx.x;
    if (q >= min(max(countA[p], 0), K)) return;              // (the whole workgroup leaves together)
    const int m = match_idx[(long long)p * K + q];
    if (m < 0 || m >= min(max(countB[p], 0), K)) return;
    if (mask && !mask[(long long)p * K + q]) return;
    __shared__ short half_o[HALF_N], half_i[HALF_N];
    ring_tables(ro, ri, half_o, half_i);
    __syncthreads();
    unsigned* map = owner + (long long)p * Hc * Wc;
    const unsigned tag = (unsigned)q + 1u;
    const int* a = kpA + ((long long)p * K + q) * 2;
    const int* b = kpB + ((long long)p * K + m) * 2;
    const long long ay = (long long)a[0] + yA, ax = (long long)a[1] + xA, by = (long long)b[0] + yB, bx = (long long)b[1] + xB;
    const auto span = [&](long long y, long long x1, long long x2) {
        x1 = max(x1, 0LL), x2 = min(x2, (long long)Wc - 1);
        for (long long x = x1; x <= x2; ++x) atomicMax(map + y * Wc + x, tag);
    };
    const auto ring = [&](long long cx, long long cy) {
        for (int k = (int)threadIdx.x - ro; k <= ro; k += blockDim.x) {
            const long long y = cy + k;
            if (y < 0 || y >= Hc) continue;
            const int d = abs(k), ho = half_o[d], hi = d <= ri ? (int)half_i[d] : -1;
            if (hi < 0) {
                span(y, cx - ho, cx + ho);
            } else {
                span(y, cx - ho, cx - hi - 1);
                span(y, cx + hi + 1, cx + ho);
            }
        }
    };
    ring(ax, ay);
    ring(bx, by);
    if (threadIdx.x == 0)
        thin_line(Hc, Wc, ax, ay, bx, by, [&](int x, int y) {
            if (0 <= x && x < Wc && 0 <= y && y < Hc) atomicMax(map + (long long)y * Wc + x, tag);
        });
}

__global__ __launch_bounds__(256) void draw_resolve_kernel(const unsigned* owner, long long pixels, const unsigned char* palette,
                                                           int npal, unsigned char* canvas)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixels) return;
    const unsigned o = owner[i];
    if (!o) return;
    const unsigned char* c = palette + 3 * ((o - 1u) % (unsigned)npal);
    unsigned char* d = canvas + 3 * i;
    d[0] = c[0], d[1] = c[1], d[2] = c[2];
}

// one workgroup per segment: lane 0 walks it and tags the t x t box of every pixel of the walk in the owner map
__global__ __launch_bounds__(64) void draw_segments_scatter_kernel(const int* seg, const int* counts, int N, int t, unsigned* owner,
                                                                   int Hc, int Wc)
{
    const int b = blockIdx.y, i = blockIdx.x;
    if (threadIdx.x != 0 || i >= min(max(counts[b], 0), N)) return;
    const int* e = seg + ((long long)b * N + i) * MP_DRAW_SEGMENT_INTS;
    unsigned* map = owner + (long long)b * Hc * Wc;
    const unsigned tag = (unsigned)i + 1u;
    const int lo = (t - 1) / 2, hi = t / 2;
    thin_line(Hc, Wc, e[1], e[0], e[3], e[2], [&](int x, int y) {
        for (int yy = max(y - lo, 0); yy <= min(y + hi, Hc - 1); ++yy)
            for (int xx = max(x - lo, 0); xx <= min(x + hi, Wc - 1); ++xx) atomicMax(map + (long long)yy * Wc + xx, tag);
    });
}

// every canvas pixel with an owner takes the colour that segment names
__global__ __launch_bounds__(256) void draw_segments_resolve_kernel(const unsigned* owner, const int* seg, int N, long long per_canvas,
                                                                    long long pixels, const unsigned char* palette, int npal,
                                                                    unsigned char* canvas)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pixels) return;
    const unsigned o = owner[i];
    if (!o) return;
    const int ci = seg[((i / per_canvas) * N + (o - 1u)) * MP_DRAW_SEGMENT_INTS + 4];
    const unsigned char* c = palette + 3 * (((ci % npal) + npal) % npal);
    unsigned char* d = canvas + 3 * i;
    d[0] = c[0], d[1] = c[1], d[2] = c[2];
}

unsigned blocks_of(long long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

// the outer and inner radius of a mark; false when the mark is refused
bool mark_radii(int kind, int radius, int thickness, int* ro, int* ri)
{
    if (radius < 0 || radius > MP_DRAW_MAX_RADIUS || thickness < 1 || kind < MP_DRAW_RING || kind > MP_DRAW_CROSS) return false;
    *ro = radius, *ri = -1;                                  // disc and cross: the thickness is not read
    if (kind != MP_DRAW_RING) return true;
    if (thickness / 2 > MP_DRAW_MAX_RADIUS - radius) return false;
    *ro = radius + thickness / 2;
    *ri = radius - (thickness + 1) / 2;
    return true;
}

// the handle's owner map holds `bytes`.  A buffer it outgrows is retired, not freed: a launch of an earlier call may still
// run on another stream
int owner_map(mp_handle* h, size_t bytes)
{
    if (h->draw_ws.bytes >= bytes) return MP_OK;
    const size_t grown = bytes > 2 * h->draw_ws.bytes ? bytes : 2 * h->draw_ws.bytes;
    if (h->draw_ws.p) h->draw_retired.emplace_back(std::move(h->draw_ws));
    int rc = ensure(h, h->draw_ws, grown);
    if (rc != MP_OK && grown > bytes) rc = ensure(h, h->draw_ws, bytes);
    return rc;
}

}  // namespace

extern "C" {

int mp_draw_gray_to_rgb(mp_handle* h, const float* images, const float* mask, int B, int H, int W, float gain,
                        unsigned char* canvas, int Hc, int Wc, int y0, int x0, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!images || !canvas) return fail(h, MP_EINVAL, "mp_draw_gray_to_rgb: NULL tensor");
    if (!frames_ok(B, H, W, 1, 32767) || !frames_ok(B, Hc, Wc, 1, 32767) || (long long)B * H * W > MAX_PIXELS)
        return fail(h, MP_EINVAL, "mp_draw_gray_to_rgb: 1 to 65535 frames, frame and canvas of 1 x 1 to 32767 x 32767 pixels");
    MP_HIP(hipSetDevice(h->device));
    const long long groups = (long long)B * H * ((W + 3) / 4);
    hipLaunchKernelGGL(draw_gray_kernel, dim3(blocks_of(groups, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), images, mask,
                       B, H, W, gain, canvas, Hc, Wc, y0, x0);
    return launch_status(h);
}

int mp_draw_marks(mp_handle* h, const int* kp_yx, const int* kp_count, int B, int K, int kind, int radius, int thickness,
                  const unsigned char* palette, int n_colors, unsigned char* canvas, int Hc, int Wc, int y0, int x0, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!kp_yx || !kp_count || !palette || !canvas) return fail(h, MP_EINVAL, "mp_draw_marks: NULL tensor");
    if (!frames_ok(B, Hc, Wc, 1, 32767) || K < 1 || K > MAX_LIST)
        return fail(h, MP_EINVAL, "mp_draw_marks: 1 to 65535 canvases of 1 x 1 to 32767 x 32767 pixels, K in [1, 2^20]");
    if (n_colors < 1) return fail(h, MP_EINVAL, "mp_draw_marks: empty palette");
    int ro, ri;
    if (!mark_radii(kind, radius, thickness, &ro, &ri))
        return fail(h, MP_EINVAL, "mp_draw_marks: kind MP_DRAW_RING / _DISC / _CROSS, radius >= 0, thickness >= 1, outer radius "
                                  "(radius + thickness / 2) at most " + std::to_string(MP_DRAW_MAX_RADIUS));
    MP_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(draw_marks_kernel, dim3((Wc + TILE - 1) / TILE, (Hc + TILE - 1) / TILE, B), dim3(TILE * TILE), 0,
                       static_cast<hipStream_t>(stream), kp_yx, kp_count, K, kind, ro, ri, y0, x0, palette, n_colors, canvas, Hc, Wc);
    return launch_status(h);
}

int mp_draw_matches(mp_handle* h, const int* kp_a, const int* kp_b, const int* count_a, const int* count_b, const int* match_idx,
                    const unsigned char* draw_mask, int P, int K, int ya, int xa, int yb, int xb, int radius, int thickness,
                    const unsigned char* palette, int n_colors, unsigned char* canvas, int Hc, int Wc, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!kp_a || !kp_b || !count_a || !count_b || !match_idx || !palette || !canvas)
        return fail(h, MP_EINVAL, "mp_draw_matches: NULL tensor");
    if (!frames_ok(P, Hc, Wc, 1, 32767) || K < 1 || K > MAX_LIST)
        return fail(h, MP_EINVAL, "mp_draw_matches: 1 to 65535 canvases of 1 x 1 to 32767 x 32767 pixels, K in [1, 2^20]");
    if (n_colors < 1) return fail(h, MP_EINVAL, "mp_draw_matches: empty palette");
    int ro, ri;
    if (!mark_radii(MP_DRAW_RING, radius, thickness, &ro, &ri))
        return fail(h, MP_EINVAL, "mp_draw_matches: radius >= 0, thickness >= 1, outer radius (radius + thickness / 2) at most " +
                                      std::to_string(MP_DRAW_MAX_RADIUS));
    MP_HIP(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long pixels = (long long)P * Hc * Wc;
    const int rc = owner_map(h, (size_t)pixels * sizeof(unsigned));
    if (rc != MP_OK) return rc;
    unsigned* owner = static_cast<unsigned*>(h->draw_ws.p);
    MP_HIP(hipMemsetAsync(owner, 0, (size_t)pixels * sizeof(unsigned), s));      // this call's map: nothing is left to a previous call
    hipLaunchKernelGGL(draw_matches_scatter_kernel, dim3(K, P), dim3(64), 0, s, kp_a, kp_b, count_a, count_b, match_idx, draw_mask,
                       K, ya, xa, yb, xb, ro, ri, owner, Hc, Wc);
    hipLaunchKernelGGL(draw_resolve_kernel, dim3(blocks_of(pixels, 256)), dim3(256), 0, s, owner, pixels, palette, n_colors, canvas);
    return launch_status(h);
}

int mp_segments_draw(mp_handle* h, const int* segments, const int* seg_count, int B, int N, int thickness,
                     const unsigned char* palette, int n_colors, unsigned char* canvas, int Hc, int Wc, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!segments || !seg_count || !palette || !canvas) return fail(h, MP_EINVAL, "mp_segments_draw: NULL tensor");
    if (!frames_ok(B, Hc, Wc, 1, 32767) || N < 1 || N > MAX_LIST)
        return fail(h, MP_EINVAL, "mp_segments_draw: 1 to 65535 canvases of 1 x 1 to 32767 x 32767 pixels, N in [1, 2^20]");
    if (n_colors < 1) return fail(h, MP_EINVAL, "mp_segments_draw: empty palette");
    if (thickness < 1 || thickness > MP_DRAW_MAX_THICKNESS)
        return fail(h, MP_EINVAL, "mp_segments_draw: thickness in [1, " + std::to_string(MP_DRAW_MAX_THICKNESS) + "]");
    MP_HIP(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const long long pixels = (long long)B * Hc * Wc;
    const int rc = owner_map(h, (size_t)pixels * sizeof(unsigned));
    if (rc != MP_OK) return rc;
    unsigned* owner = static_cast<unsigned*>(h->draw_ws.p);
    MP_HIP(hipMemsetAsync(owner, 0, (size_t)pixels * sizeof(unsigned), s));
    hipLaunchKernelGGL(draw_segments_scatter_kernel, dim3(N, B), dim3(64), 0, s, segments, seg_count, N, thickness, owner, Hc, Wc);
    hipLaunchKernelGGL(draw_segments_resolve_kernel, dim3(blocks_of(pixels, 256)), dim3(256), 0, s, owner, segments, N,
                       (long long)Hc * Wc, pixels, palette, n_colors, canvas);
    return launch_status(h);
}

int mp_draw_compose(mp_handle* h, const float* warped, const float* thermal, int B, int H, int W, int mode, int alpha, int cell,
                    unsigned char* canvas, int Hc, int Wc, int y0, int x0, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!warped || !thermal || !canvas) return fail(h, MP_EINVAL, "mp_draw_compose: NULL tensor");
    if (!frames_ok(B, H, W, 1, 32767) || !frames_ok(B, Hc, Wc, 1, 32767) || (long long)B * H * W > MAX_PIXELS)
        return fail(h, MP_EINVAL, "mp_draw_compose: 1 to 65535 frames, frame and canvas of 1 x 1 to 32767 x 32767 pixels");
    if (mode < MP_DRAW_BLEND || mode > MP_DRAW_DIFFERENCE)
        return fail(h, MP_EINVAL, "mp_draw_compose: mode MP_DRAW_BLEND, _CHECKER, _ANAGLYPH or _DIFFERENCE");
    if (alpha < 0 || alpha > 256) return fail(h, MP_EINVAL, "mp_draw_compose: alpha in [0, 256], got " + std::to_string(alpha));
    if (cell < 1) return fail(h, MP_EINVAL, "mp_draw_compose: cell >= 1, got " + std::to_string(cell));
    MP_HIP(hipSetDevice(h->device));
    const long long groups = (long long)B * H * ((W + 3) / 4);
    hipLaunchKernelGGL(draw_compose_kernel, dim3(blocks_of(groups, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), warped,
                       thermal, B, H, W, mode, alpha, cell, canvas, Hc, Wc, y0, x0);
    return launch_status(h);
}

}  // extern "C"
