// Synthetic shapes (reference multipoint/utils/draw_primitives.py and multipoint/datasets/SyntheticShapes.py) for a batch of
// n fp32 canvases [n][H][W] with one host-drawn command list per image (include/multipoint_hip.h).
//
// The launcher walks the steps s = 0 .. max(commands per image) - 1 and at each step launches, for the whole batch, the
// kernels of the command kinds that some image has at s; a workgroup whose image has another kind there exits:
//   shapes_pixel_kernel    threshold (host field or hashed uniform against t) and randu, one thread per pixel
//   shapes_mean_kernel     the canvas mean summed in double: 64 workgroups per image, their sums added in a fixed order
//   shapes_blobs_kernel    one workgroup per 16 x 16 tile: the command's circles that touch the tile are listed in LDS (the
//                          list holds every circle of the command), each pixel takes the highest-index circle covering it
//   shapes_box_rows_kernel / shapes_box_cols_kernel   cv2.blur, separable, sums in double
//   shapes_draw_kernel     line, convex polygon, polygon, ellipse: DRAW_SPLIT workgroups per image share the rows; the
//                          16.16 edge walks run redundantly in every lane (registers only) and the lanes share each span
// Every rasteriser is integer arithmetic after OpenCV's drawing.cpp: Circle (the midpoint walk, as a table of half widths
// per radius and row), ThickLine / LineIterator, FillConvexPoly, CollectPolyEdges + FillEdgeCollection, ellipse2Poly.
// mp_shapes_finish runs the Gaussian blurs (photometric.hip's sepFilter2D restatement) and the INTER_LINEAR resize.
#include "host.h"
#include "mp_device.h"
#include "mp_raster.h"

#pragma clang fp contract(off)

using namespace mp_host;
using namespace mp_raster;

static_assert(sizeof(mp_shapes_cmd) == 88, "mp_shapes_cmd layout: multipoint_amd/_lib.py binds it with ctypes");

namespace {

constexpr int TILE = 16;                // blob tile: 16 x 16 pixels, one per thread
constexpr int HALF_STRIDE = MP_SHAPES_MAX_RADIUS + 1;
constexpr int DRAW_SPLIT = 16;          // workgroups sharing the rows of one image's draw command
constexpr int ROW_BAND = 4;             // consecutive rows one of them owns
constexpr int MEAN_PARTS = 64;         // workgroups sharing one image's mean
constexpr int BOX_COLS = 64, BOX_ROWS = 32;   // column pass: 64 columns x 4 row groups of BOX_ROWS rows per workgroup

__device__ __forceinline__ const mp_shapes_cmd* command(const mp_shapes_cmd* cmds, const int* offset, int img, int step)
{
    const int i = offset[img] + step;
    return i < offset[img + 1] ? cmds + i : nullptr;
}

__device__ __forceinline__ float resolve_color(const mp_shapes_cmd& c, double mean)
{
    return (float)(c.resolve && fabs(c.u - mean) < c.min_contrast ? c.col_b : c.col_a);
}

// Circle(): half[r][k] = the half width of the widest span the midpoint walk of radius r draws on the rows cy -+ k
__global__ __launch_bounds__(256) void shapes_halfwidth_kernel(short* half)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > MP_SHAPES_MAX_RADIUS) return;
    circle_halfwidths(r, half + r * HALF_STRIDE);
}

__global__ __launch_bounds__(256) void shapes_pixel_kernel(const mp_shapes_cmd* cmds, const int* offset, int step,
                                                           const double* fields, float* canvas, long long HW)
{
    const int img = blockIdx.y;
    const mp_shapes_cmd* c = command(cmds, offset, img, step);
    if (!c || (c->kind != MP_SHAPES_THRESHOLD && c->kind != MP_SHAPES_RANDU)) return;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= HW) return;
    if (c->kind == MP_SHAPES_RANDU) {
        canvas[img * HW + p] = (float)hash_uniform(c->key, (unsigned long long)p);
    } else {
        const double u = c->a[0] < 0 ? hash_uniform(c->key, (unsigned long long)p) : fields[c->a[0] * HW + p];
        canvas[img * HW + p] = u > c->t ? 1.f : 0.f;
    }
}

// MEAN_PARTS workgroups per image sum interleaved chunks in double; shapes_mean_final_kernel adds the parts in order
__global__ __launch_bounds__(256) void shapes_mean_kernel(const mp_shapes_cmd* cmds, const int* offset, int step,
                                                          const float* canvas, long long HW, double* partial)
{
    const int img = blockIdx.y;
    const mp_shapes_cmd* c = command(cmds, offset, img, step);
    if (!c || c->kind != MP_SHAPES_MEAN) return;
    const float* x = canvas + img * HW;
    double s = 0.0;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += (long long)MEAN_PARTS * blockDim.x)
        s += (double)x[p];
    __shared__ double part[256];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[img * MEAN_PARTS + blockIdx.x] = part[0];
}

__global__ __launch_bounds__(64) void shapes_mean_final_kernel(const mp_shapes_cmd* cmds, const int* offset, int step, int n,
                                                               const double* partial, long long HW, double* mean)
{
    const int img = blockIdx.x * blockDim.x + threadIdx.x;
    if (img >= n) return;
    const mp_shapes_cmd* c = command(cmds, offset, img, step);
    if (!c || c->kind != MP_SHAPES_MEAN) return;
    double s = 0.0;
    for (int k = 0; k < MEAN_PARTS; ++k) s += partial[img * MEAN_PARTS + k];
    mean[img] = s / (double)HW;
}

// dynamic LDS: one int per circle of the largest blob command of the step
__global__ __launch_bounds__(TILE * TILE) void shapes_blobs_kernel(const mp_shapes_cmd* cmds, const int* offset, int step,
                                                                   const int* circles, const double* colors,
                                                                   const short* half, const double* mean, float* canvas,
                                                                   float* aux, int H, int W)
{
    const int img = blockIdx.z;
    const mp_shapes_cmd* c = command(cmds, offset, img, step);
    if (!c || c->kind != MP_SHAPES_BLOBS) return;
    extern __shared__ int list[];
    __shared__ int count;
    if (threadIdx.x == 0) count = 0;
    __syncthreads();
    const int first = c->a[0], n = c->a[1];
    const int x0 = blockIdx.x * TILE, y0 = blockIdx.y * TILE;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int* q = circles + 3 * (first + i);
        if (q[0] + q[2] >= x0 && q[0] - q[2] < x0 + TILE && q[1] + q[2] >= y0 && q[1] - q[2] < y0 + TILE)
            list[atomicAdd(&count, 1)] = i;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x % TILE, y = y0 + threadIdx.x / TILE;
    if (x >= W || y >= H) return;
    int best = -1;
    for (int j = 0; j < count; ++j) {
        const int i = list[j];
        if (i < best) continue;
        const int* q = circles + 3 * (first + i);
        const int dy = abs(y - q[1]);
        if (dy <= q[2] && abs(x - q[0]) <= half[q[2] * HALF_STRIDE + dy]) best = i;
    }
    float* dst = (c->target ? aux : canvas) + ((long long)img * H + y) * W + x;
    const double m = mean[img];
    if (best >= 0) {
        const double a = colors[2 * (first + best)], b = colors[2 * (first + best) + 1];
        *dst = (float)(c->resolve && fabs(a - m) < c->min_contrast ? b : a);
    } else if (c->a[2]) {
        *dst = resolve_color(*c, m);
    }
}

// row sums: one workgroup per (row, image); dynamic LDS: the reflected row as doubles (W + k - 1)
__global__ __launch_bounds__(256) void shapes_box_rows_kernel(const mp_shapes_cmd* cmds, const int* offset, int step,
                                                              const float* canvas, const float* aux, int H, int W, double* tmp)
{
    const int img = blockIdx.y, y = blockIdx.x;
    const mp_shapes_cmd* c = command(cmds, offset, img, step);
    if (!c || c->kind != MP_SHAPES_BOX_BLUR) return;
    const int k = c->a[0], a = k / 2;
    extern __shared__ double ext[];
    const float* src = (c->target ? aux : canvas) + ((long long)img * H + y) * W;
    for (int i = threadIdx.x; i < W + k - 1; i += blockDim.x) ext[i] = (double)src[reflect101(i - a, W)];
    __syncthreads();
    double* dst = tmp + ((long long)img * H + y) * W;
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        double s = 0.0;
        for (int j = 0; j < k; ++j) s += ext[x + j];
        dst[x] = s;
    }
}

// column sums: each thread slides the window down BOX_ROWS rows of one column
__global__ __launch_bounds__(256) void shapes_box_cols_kernel(const mp_shapes_cmd* cmds, const int* offset, int step,
                                                              const double* tmp, int H, int W, float* canvas, float* aux)
{
    const int img = blockIdx.z;
    const mp_shapes_cmd* c = command(cmds, offset, img, step);
    if (!c || c->kind != MP_SHAPES_BOX_BLUR) return;
    const int k = c->a[0], a = k / 2;
    const int x = blockIdx.x * BOX_COLS + threadIdx.x % BOX_COLS;
    const int y0 = (blockIdx.y * 4 + threadIdx.x / BOX_COLS) * BOX_ROWS;
    if (x >= W || y0 >= H) return;
    const double* src = tmp + (long long)img * H * W + x;
    float* dst = (c->target ? aux : canvas) + (long long)img * H * W + x;
    const double scale = 1.0 / ((double)k * (double)k);
    double s = 0.0;
    for (int j = 0; j < k; ++j) s += src[(long long)reflect101(y0 - a + j, H) * W];
    const int y1 = min(y0 + BOX_ROWS, H);
    for (int y = y0; y < y1; ++y) {
        dst[(long long)y * W] = (float)(s * scale);
        s += src[(long long)reflect101(y + 1 - a + k - 1, H) * W] - src[(long long)reflect101(y - a, H) * W];
    }
}

__global__ __launch_bounds__(256) void shapes_draw_kernel(const mp_shapes_cmd* cmds, const int* offset, int step,
                                                          const int* verts, const short* half, const double* mean,
                                                          float* canvas, const float* aux, int H, int W)
{
    const int img = blockIdx.y, split = blockIdx.x, nsplit = gridDim.x;
    const mp_shapes_cmd* c = command(cmds, offset, img, step);
    if (!c || c->kind < MP_SHAPES_LINE || c->kind > MP_SHAPES_ELLIPSE) return;
    float* dst = canvas + (long long)img * H * W;
    const float* src = c->kind == MP_SHAPES_POLY && c->a[2] ? aux + (long long)img * H * W : nullptr;
    const float color = resolve_color(*c, mean[img]);
    __shared__ long long vx[MAX_VERTS], vy[MAX_VERTS], rx[MAX_VERTS], ry[MAX_VERTS];
    __shared__ int npts_s;
    const int tid = threadIdx.x;
    const auto paint = [&](int x, int y) {                   // (x, y) inside the frame
        const long long p = (long long)y * W + x;
        dst[p] = src ? src[p] : color;
    };
    const auto put = [&](long long x, long long y) {
        if (0 <= x && x < W && 0 <= y && y < H) paint((int)x, (int)y);
    };
    const auto span = [&](int y, int a, int b) {             // 0 <= y < H, the span clipped; this workgroup's rows only
        if ((y / ROW_BAND) % nsplit != split) return;
        for (int x = a + tid; x <= b; x += blockDim.x) paint(x, y);
    };
    const auto circle = [&](int cx, int cy, int r) {
        for (int k = 0; k <= r; ++k) {
            const int hw = half[r * HALF_STRIDE + k];
            const int a = max(cx - hw, 0), b = min(cx + hw, W - 1);
            if (hw < 0 || a > b) continue;
            if (cy - k >= 0 && cy - k < H) span(cy - k, a, b);
            if (k > 0 && cy + k >= 0 && cy + k < H) span(cy + k, a, b);
        }
    };
    const auto outline2 = [&](int npts) {                    // Line2 between consecutive 16.16 vertices
        if (split == 0 && tid < npts) {
            const int t0 = tid == 0 ? npts - 1 : tid - 1;
            line2(H, W, vx[t0], vy[t0], vx[tid], vy[tid], put);
        }
    };
    switch (c->kind) {
    case MP_SHAPES_ELLIPSE: {
        ellipse_poly(c->a, vx, vy, rx, ry, &npts_s);
        outline2(npts_s);
        convex_spans(vx, vy, npts_s, H, W, span);
        break;
    }
    case MP_SHAPES_LINE: {
        const int thickness = c->a[4];
        if (thickness <= 1) {
            if (split == 0 && tid == 0) thin_line(H, W, c->a[0], c->a[1], c->a[2], c->a[3], paint);
            break;
        }
        // ThickLine: the rectangle around the segment in 16.16, then the two end circles
        const long long p0x = (long long)c->a[0] << XY_SHIFT, p0y = (long long)c->a[1] << XY_SHIFT;
        const long long p1x = (long long)c->a[2] << XY_SHIFT, p1y = (long long)c->a[3] << XY_SHIFT;
        const double inv = 1.0 / (double)XY_ONE;
        const double dx = (double)(p0x - p1x) * inv, dy = (double)(p1y - p0y) * inv;
        double r = dx * dx + dy * dy;
        const int odd = thickness & 1;
        const long long t = (long long)thickness << (XY_SHIFT - 1);
        const bool rect = fabs(r) > 2.220446049250313e-16;
        if (rect) {
            r = ((double)t + odd * (double)XY_ONE * 0.5) / sqrt(r);
            const long long dpx = cv_round(dy * r), dpy = cv_round(dx * r);
            if (tid == 0) {
                vx[0] = p0x + dpx; vy[0] = p0y + dpy;
                vx[1] = p0x - dpx; vy[1] = p0y - dpy;
                vx[2] = p1x - dpx; vy[2] = p1y - dpy;
                vx[3] = p1x + dpx; vy[3] = p1y + dpy;
            }
            __syncthreads();
            outline2(4);
            convex_spans(vx, vy, 4, H, W, span);
        }
        const int rad = (int)((t + (XY_ONE >> 1)) >> XY_SHIFT);
        circle(c->a[0], c->a[1], rad);
        circle(c->a[2], c->a[3], rad);
        break;
    }
    case MP_SHAPES_CONVEX:
    case MP_SHAPES_POLY: {
        const int npts = c->a[1];
        const int* v = verts + 2 * c->a[0];
        if (tid < npts) {
            vx[tid] = v[2 * tid];                            // whole pixels here, 16.16 below
            vy[tid] = v[2 * tid + 1];
        }
        __syncthreads();
        if (split == 0 && tid < npts) {                      // the outline: Line() between consecutive vertices
            const int t0 = tid == 0 ? npts - 1 : tid - 1;
            thin_line(H, W, vx[t0], vy[t0], vx[tid], vy[tid], paint);
        }
        if (c->kind == MP_SHAPES_CONVEX) {
            __syncthreads();
            if (tid < npts) { vx[tid] <<= XY_SHIFT; vy[tid] <<= XY_SHIFT; }
            __syncthreads();
            convex_spans(vx, vy, npts, H, W, span);
            break;
        }
        // FillEdgeCollection: on row y the active edges (y0 <= y < y1) sorted by x pair up, and a pair covers the pixels
        // from the ceiling of its left x to the floor of its right x; x advances by dx per row from the edge's top.  For a
        // pixel at X = x << 16 that is: some active edge has x == X, or an odd number of them has x < X.
        // rx: the edge's x at its top row (16.16), ry: dx; vx / vy are reused for y0 / y1 after the outline
        __syncthreads();
        long long ex = 0, edx = 0, ey0 = 0, ey1 = 0;
        if (tid < npts) {
            const int t0 = tid == 0 ? npts - 1 : tid - 1;
            const long long ax = vx[t0], ay = vy[t0], bx = vx[tid], by = vy[tid];
            if (ay != by) {
                edx = ((bx - ax) * XY_ONE) / (by - ay);
                if (ay < by) { ey0 = ay; ey1 = by; ex = ax * XY_ONE; }
                else { ey0 = by; ey1 = ay; ex = bx * XY_ONE; }
            }
        }
        __syncthreads();
        if (tid < npts) { rx[tid] = ex; ry[tid] = edx; vx[tid] = ey0; vy[tid] = ey1; }
        __syncthreads();
        long long ymin = vx[0], ymax = vy[0], xlo = rx[0], xhi = rx[0];
        bool any = false;
        for (int e = 0; e < npts; ++e) {
            if (vx[e] == vy[e]) continue;                    // a horizontal edge is no edge
            const long long xe = rx[e] + (vy[e] - vx[e]) * ry[e];
            if (!any) { ymin = vx[e]; ymax = vy[e]; xlo = min(rx[e], xe); xhi = max(rx[e], xe); any = true; }
            ymin = min(ymin, vx[e]); ymax = max(ymax, vy[e]);
            xlo = min(xlo, min(rx[e], xe)); xhi = max(xhi, max(rx[e], xe));
        }
        if (!any) break;
        const int ya = (int)max(ymin, 0LL), yb = (int)min(ymax, (long long)H);         // rows [ya, yb)
        const int xa = (int)max((xlo + XY_ONE - 1) >> XY_SHIFT, 0LL), xb = (int)min(xhi >> XY_SHIFT, (long long)W - 1);
        if (xa > xb) break;
        const int bw = xb - xa + 1;
        for (int y = ya; y < yb; ++y) {
            if ((y / ROW_BAND) % nsplit != split) continue;
            for (int i = tid; i < bw; i += blockDim.x) {
                const long long X = (long long)(xa + i) << XY_SHIFT;
                int below = 0;
                bool on = false;
                for (int e = 0; e < npts; ++e) {
                    if (y < vx[e] || y >= vy[e]) continue;
                    const long long xe = rx[e] + (y - vx[e]) * ry[e];
                    below += xe < X;
                    on = on || xe == X;
                }
                if (on || (below & 1)) paint(xa + i, y);
            }
        }
        break;
    }
    default:
        break;
    }
}

// cv2.resize(..., INTER_LINEAR) of a float image: the float weight pair of resize.cpp, indices clamped
__device__ __forceinline__ void linear_tap(int d, double scale, int n, int& i0, int& i1, float& f)
{
    float fx = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(fx);
    fx -= (float)s;
    if (s < 0) { s = 0; fx = 0.f; }
    if (s >= n - 1) { s = n - 1; fx = 0.f; }
    i0 = s;
    i1 = min(s + 1, n - 1);
    f = fx;
}

__global__ __launch_bounds__(256) void shapes_resize_kernel(const float* canvas, int H, int W, float* out, int oh, int ow,
                                                            double scale_y, double scale_x)
{
    const int img = blockIdx.y;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (long long)oh * ow) return;
    const int oy = (int)(p / ow), ox = (int)(p % ow);
    const float* src = canvas + (long long)img * H * W;
    int x0, x1, y0, y1;
    float fx, fy;
    linear_tap(ox, scale_x, W, x0, x1, fx);
    linear_tap(oy, scale_y, H, y0, y1, fy);
    const float top = src[(long long)y0 * W + x0] * (1.f - fx) + src[(long long)y0 * W + x1] * fx;
    const float bot = src[(long long)y1 * W + x0] * (1.f - fx) + src[(long long)y1 * W + x1] * fx;
    out[(long long)img * oh * ow + p] = top * (1.f - fy) + bot * fy;
}

struct ShapesWorkspace {
    mp_shapes_cmd* cmds;      // [n_cmds]
    int* offset;              // [n + 1]
    int* verts;               // [n_verts][2]
    int* circles;             // [n_circles][3]
    double* colors;           // [n_circles][2]
    short* half;              // [256][256]
    int* ksize;               // [2][n]  mp_shapes_finish
    double* partial;          // [n][MEAN_PARTS]
    float* weights;           // [n][MP_PHOTO_MAX_BLUR]
    float* aux;               // [n][H][W]  second canvas; the row-filtered frame of the Gaussian blurs
    double* tmp;              // [n][H][W]  row sums of the box blur
    size_t bytes;
};

ShapesWorkspace shapes_workspace(void* base, int n, int H, int W, int n_cmds, int n_verts, int n_circles)
{
    const size_t px = (size_t)n * H * W;
    const auto atleast1 = [](int v) { return (size_t)(v > 0 ? v : 1); };
    Carver c(base);
    ShapesWorkspace w;
    w.cmds = c.take<mp_shapes_cmd>(atleast1(n_cmds));
    w.offset = c.take<int>((size_t)n + 1);
    w.verts = c.take<int>(2 * atleast1(n_verts));
    w.circles = c.take<int>(3 * atleast1(n_circles));
    w.colors = c.take<double>(2 * atleast1(n_circles));
    w.half = c.take<short>((size_t)HALF_STRIDE * HALF_STRIDE);
    w.ksize = c.take<int>(2 * (size_t)n);
    w.partial = c.take<double>(MEAN_PARTS * (size_t)n);
    w.weights = c.take<float>(MP_PHOTO_MAX_BLUR * (size_t)n);
    w.aux = c.take<float>(px);
    w.tmp = c.take<double>(px);
    w.bytes = c.bytes();
    return w;
}

bool frame_ok(int n, int H, int W)
{
    return frames_ok(n, H, W, 1, 32768) && (long long)n * H * W <= (1LL << 32);
}

bool coord_ok(int v) { return v >= -MP_SHAPES_MAX_COORD && v <= MP_SHAPES_MAX_COORD; }

}  // namespace

extern "C" {

int mp_shapes_workspace_bytes(int n, int H, int W, int n_cmds, int n_verts, int n_circles, long long* bytes)
{
    if (!bytes || !frame_ok(n, H, W) || n_cmds < 0 || n_verts < 0 || n_circles < 0) return MP_EINVAL;
    *bytes = (long long)shapes_workspace(nullptr, n, H, W, n_cmds, n_verts, n_circles).bytes;
    return MP_OK;
}

int mp_shapes_render(mp_handle* h, float* canvas, double* mean, int n, int H, int W, const mp_shapes_cmd* cmds,
                     const int* cmd_offset, const int* verts, int n_verts, const int* circles, const double* circle_colors,
                     int n_circles, const double* fields, int n_fields, void* workspace, long long workspace_bytes,
                     void* stream)
{
    if (!h) return MP_EINVAL;
    const std::string f = "mp_shapes_render";
    if (!canvas || !mean || !cmds || !cmd_offset) return fail(h, MP_EINVAL, f + ": NULL argument");
    if (!frame_ok(n, H, W)) return fail(h, MP_EINVAL, f + ": need 0 < n <= 65535 frames of at most 32768 x 32768 pixels");
    if (n_verts < 0 || n_circles < 0 || n_fields < 0 || (n_verts && !verts) || (n_circles && (!circles || !circle_colors)) ||
        (n_fields && !fields))
        return fail(h, MP_EINVAL, f + ": bad tables");
    if (cmd_offset[0] != 0) return fail(h, MP_EINVAL, f + ": cmd_offset[0] must be 0");
    int steps = 0;
    for (int i = 0; i < n; ++i) {
        if (cmd_offset[i + 1] < cmd_offset[i]) return fail(h, MP_EINVAL, f + ": cmd_offset must not decrease");
        steps = std::max(steps, cmd_offset[i + 1] - cmd_offset[i]);
    }
    const int n_cmds = cmd_offset[n];
    for (int i = 0; i < n_verts * 2; ++i)
        if (!coord_ok(verts[i])) return fail(h, MP_EINVAL, f + ": vertex coordinate out of range");
    for (int i = 0; i < n_circles; ++i)
        if (!coord_ok(circles[3 * i]) || !coord_ok(circles[3 * i + 1]) || circles[3 * i + 2] < 0 ||
            circles[3 * i + 2] > MP_SHAPES_MAX_RADIUS)
            return fail(h, MP_EINVAL, f + ": circle " + std::to_string(i) + " out of range (radius 0.." +
                        std::to_string(MP_SHAPES_MAX_RADIUS) + ")");
    for (int i = 0; i < n_cmds; ++i) {
        const mp_shapes_cmd& c = cmds[i];
        const std::string at = f + ": command " + std::to_string(i);
        if (c.target != 0 && !(c.target == 1 && (c.kind == MP_SHAPES_BLOBS || c.kind == MP_SHAPES_BOX_BLUR)))
            return fail(h, MP_EINVAL, at + ": bad target");
        switch (c.kind) {
        case MP_SHAPES_THRESHOLD:
            if (c.a[0] >= n_fields) return fail(h, MP_EINVAL, at + ": noise field out of range");
            break;
        case MP_SHAPES_MEAN:
        case MP_SHAPES_RANDU:
            break;
        case MP_SHAPES_BLOBS:
            if (c.a[0] < 0 || c.a[1] < 0 || c.a[1] > MP_SHAPES_MAX_BLOBS || (long long)c.a[0] + c.a[1] > n_circles)
                return fail(h, MP_EINVAL, at + ": circles outside the table (at most " + std::to_string(MP_SHAPES_MAX_BLOBS) +
                            " per command)");
            break;
        case MP_SHAPES_BOX_BLUR:
            if (c.a[0] < 1 || (size_t)(W + c.a[0] - 1) * sizeof(double) > 65536)
                return fail(h, MP_EINVAL, at + ": box size must be >= 1 and W + k - 1 <= 8192");
            break;
        case MP_SHAPES_LINE:
            if (!coord_ok(c.a[0]) || !coord_ok(c.a[1]) || !coord_ok(c.a[2]) || !coord_ok(c.a[3]) || c.a[4] < 1 ||
                c.a[4] > MP_SHAPES_MAX_RADIUS)
                return fail(h, MP_EINVAL, at + ": line out of range (thickness 1.." + std::to_string(MP_SHAPES_MAX_RADIUS) + ")");
            break;
        case MP_SHAPES_CONVEX:
        case MP_SHAPES_POLY:
            if (c.a[0] < 0 || c.a[1] < 1 || c.a[1] > MP_SHAPES_MAX_VERTS || (long long)c.a[0] + c.a[1] > n_verts)
                return fail(h, MP_EINVAL, at + ": vertices outside the table (1.." + std::to_string(MP_SHAPES_MAX_VERTS) +
                            " per polygon)");
            break;
        case MP_SHAPES_ELLIPSE:
            if (!coord_ok(c.a[0]) || !coord_ok(c.a[1]) || abs(c.a[2]) > 16384 || abs(c.a[3]) > 16384 || abs(c.a[4]) > 36000)
                return fail(h, MP_EINVAL, at + ": ellipse out of range");
            break;
        default:
            return fail(h, MP_EINVAL, at + ": unknown kind " + std::to_string(c.kind));
        }
    }
    const ShapesWorkspace w = shapes_workspace(workspace, n, H, W, n_cmds, n_verts, n_circles);
    if (!workspace || workspace_bytes < (long long)w.bytes)
        return fail(h, MP_EINVAL, f + ": workspace smaller than mp_shapes_workspace_bytes");
    MP_HIP(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_cmds) MP_HIP(hipMemcpyAsync(w.cmds, cmds, sizeof(mp_shapes_cmd) * n_cmds, hipMemcpyHostToDevice, s));
    MP_HIP(hipMemcpyAsync(w.offset, cmd_offset, sizeof(int) * (n + 1), hipMemcpyHostToDevice, s));
    if (n_verts) MP_HIP(hipMemcpyAsync(w.verts, verts, sizeof(int) * 2 * n_verts, hipMemcpyHostToDevice, s));
    if (n_circles) {
        MP_HIP(hipMemcpyAsync(w.circles, circles, sizeof(int) * 3 * n_circles, hipMemcpyHostToDevice, s));
        MP_HIP(hipMemcpyAsync(w.colors, circle_colors, sizeof(double) * 2 * n_circles, hipMemcpyHostToDevice, s));
    }
    // the caller's host arrays may be gone once the entry point returns: wait for the copies to have read them
    MP_HIP(hipStreamSynchronize(s));
    hipLaunchKernelGGL(shapes_halfwidth_kernel, dim3(1), dim3(256), 0, s, w.half);
    const long long HW = (long long)H * W;
    const dim3 pixel_grid((unsigned)((HW + 255) / 256), n);
    for (int step = 0; step < steps; ++step) {
        bool kinds[MP_SHAPES_RANDU + 1] = {};
        int max_blobs = 0, max_k = 1;
        for (int i = 0; i < n; ++i) {
            if (cmd_offset[i] + step >= cmd_offset[i + 1]) continue;
            const mp_shapes_cmd& c = cmds[cmd_offset[i] + step];
            kinds[c.kind] = true;
            if (c.kind == MP_SHAPES_BLOBS) max_blobs = std::max(max_blobs, c.a[1]);
            if (c.kind == MP_SHAPES_BOX_BLUR) max_k = std::max(max_k, c.a[0]);
        }
        if (kinds[MP_SHAPES_THRESHOLD] || kinds[MP_SHAPES_RANDU])
            hipLaunchKernelGGL(shapes_pixel_kernel, pixel_grid, dim3(256), 0, s, w.cmds, w.offset, step, fields, canvas, HW);
        if (kinds[MP_SHAPES_MEAN])
        {
            hipLaunchKernelGGL(shapes_mean_kernel, dim3(MEAN_PARTS, n), dim3(256), 0, s, w.cmds, w.offset, step, canvas, HW,
                               w.partial);
            hipLaunchKernelGGL(shapes_mean_final_kernel, dim3((n + 63) / 64), dim3(64), 0, s, w.cmds, w.offset, step, n,
                               w.partial, HW, mean);
        }
        if (kinds[MP_SHAPES_BLOBS])
            hipLaunchKernelGGL(shapes_blobs_kernel, dim3((W + TILE - 1) / TILE, (H + TILE - 1) / TILE, n), dim3(TILE * TILE),
                               sizeof(int) * (size_t)std::max(max_blobs, 1), s, w.cmds, w.offset, step, w.circles, w.colors,
                               w.half, mean, canvas, w.aux, H, W);
        if (kinds[MP_SHAPES_BOX_BLUR]) {
            hipLaunchKernelGGL(shapes_box_rows_kernel, dim3(H, n), dim3(256), sizeof(double) * (size_t)(W + max_k - 1), s,
                               w.cmds, w.offset, step, canvas, w.aux, H, W, w.tmp);
            hipLaunchKernelGGL(shapes_box_cols_kernel, dim3((W + BOX_COLS - 1) / BOX_COLS, (H + 4 * BOX_ROWS - 1) / (4 * BOX_ROWS), n),
                               dim3(256), 0, s, w.cmds, w.offset, step, w.tmp, H, W, canvas, w.aux);
        }
        if (kinds[MP_SHAPES_LINE] || kinds[MP_SHAPES_CONVEX] || kinds[MP_SHAPES_POLY] || kinds[MP_SHAPES_ELLIPSE])
            hipLaunchKernelGGL(shapes_draw_kernel, dim3(DRAW_SPLIT, n), dim3(256), 0, s, w.cmds, w.offset, step, w.verts, w.half,
                               mean, canvas, w.aux, H, W);
    }
    return launch_status(h);
}

int mp_shapes_finish(mp_handle* h, float* canvas, int n, int H, int W, const int* blur1, const int* blur2, float* out, int oh,
                     int ow, void* workspace, long long workspace_bytes, void* stream)
{
    if (!h) return MP_EINVAL;
    const std::string f = "mp_shapes_finish";
    if (!canvas || !out || !blur1 || !blur2) return fail(h, MP_EINVAL, f + ": NULL argument");
    if (!frame_ok(n, H, W) || !sides_ok(oh, ow, 1, 32768))
        return fail(h, MP_EINVAL, f + ": need 0 < n <= 65535 frames of at most 32768 x 32768 pixels");
    int kmax[2] = {0, 0};
    for (int i = 0; i < n; ++i) {
        const int k[2] = {blur1[i], blur2[i]};
        for (int j = 0; j < 2; ++j) {
            if (k[j] < 0 || k[j] > MP_PHOTO_MAX_BLUR || (k[j] > 0 && (k[j] & 1) == 0))
                return fail(h, MP_EINVAL, f + ": blur sizes must be odd and <= " + std::to_string(MP_PHOTO_MAX_BLUR) + " (0: none)");
            kmax[j] = std::max(kmax[j], k[j]);
        }
    }
    if (gaussian_blur_lds_bytes(std::max(kmax[0], kmax[1]), W) > 65536)
        return fail(h, MP_EINVAL, f + ": frame too wide for the blur size");
    const ShapesWorkspace w = shapes_workspace(workspace, n, H, W, 0, 0, 0);
    if (!workspace || workspace_bytes < (long long)w.bytes)
        return fail(h, MP_EINVAL, f + ": workspace smaller than mp_shapes_workspace_bytes");
    MP_HIP(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    MP_HIP(hipMemcpyAsync(w.ksize, blur1, sizeof(int) * n, hipMemcpyHostToDevice, s));
    MP_HIP(hipMemcpyAsync(w.ksize + n, blur2, sizeof(int) * n, hipMemcpyHostToDevice, s));
    MP_HIP(hipStreamSynchronize(s));
    for (int j = 0; j < 2; ++j)
        if (kmax[j] > 0) launch_gaussian_blur_frames(canvas, w.aux, w.weights, w.ksize + j * n, kmax[j], n, H, W, s);
    if (oh == H && ow == W) {
        MP_HIP(hipMemcpyAsync(out, canvas, sizeof(float) * (size_t)n * H * W, hipMemcpyDeviceToDevice, s));
    } else {
        const long long op = (long long)oh * ow;
        hipLaunchKernelGGL(shapes_resize_kernel, dim3((unsigned)((op + 255) / 256), n), dim3(256), 0, s, canvas, H, W, out, oh,
                           ow, 1.0 / ((double)oh / (double)H), 1.0 / ((double)ow / (double)W));
    }
    return launch_status(h);
}

}  // extern "C"
