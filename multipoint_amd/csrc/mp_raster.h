// OpenCV's LINE_8 drawing rules, shared by the shade ellipses of photometric.hip, the synthetic shapes of shapes.hip and the
// result views of draw.hip: clipLine, Line2, ellipse2Poly and the FillConvexPoly edge walk in 16.16 fixed point, Line (the
// LineIterator) and the half widths of Circle's midpoint walk in whole pixels (drawing.cpp).  Internal header.
// The callers supply where a pixel or a row span goes: put(x, y) is called for any integer pixel (the callee clips),
// span(y, a, b) for every row y >= 0 the walk visits with the span already clipped to [0, W - 1] (a > b: empty row).
#pragma once
#include <hip/hip_runtime.h>

namespace mp_raster {

constexpr int XY_SHIFT = 16;
constexpr long long XY_ONE = 1LL << XY_SHIFT;
constexpr int MAX_VERTS = 80;           // ellipse2Poly with delta >= 5: at most 73 points

// OpenCV's SinTable[d]: sin of d degrees with 7 decimals, as float
__device__ __forceinline__ float sin_table(int d)
{
    return (float)(rint(sin((double)d * (3.141592653589793 / 180.0)) * 1e7) / 1e7);
}

__device__ __forceinline__ long long cv_round(double v) { return (long long)rint(v); }

// clipLine(Size2l(right + 1, bottom + 1), p1, p2) with the inclusive limits given (16.16 or whole pixels)
__device__ __forceinline__ bool clip_line_to(long long right, long long bottom, long long& x1, long long& y1, long long& x2, long long& y2)
{
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        long long a;
        if (c1 & 12) {
            a = c1 < 8 ? 0 : bottom;
            x1 += (long long)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            a = c2 < 8 ? 0 : bottom;
            x2 += (long long)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                a = c1 == 1 ? 0 : right;
                y1 += (long long)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                a = c2 == 1 ? 0 : right;
                y2 += (long long)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    return (c1 | c2) == 0;
}

// clipLine(Size2l(W << 16, H << 16), p1, p2)
__device__ __forceinline__ bool clip_line(int W, int H, long long& x1, long long& y1, long long& x2, long long& y2)
{
    return clip_line_to(((long long)W << XY_SHIFT) - 1, ((long long)H << XY_SHIFT) - 1, x1, y1, x2, y2);
}

// Line2: the LINE_8 segment between two 16.16 points
template <typename Put>
__device__ __forceinline__ void line2(int H, int W, long long x1, long long y1, long long x2, long long y2, Put put)
{
    if (!clip_line(W, H, x1, y1, x2, y2)) return;
    long long dx = x2 - x1, dy = y2 - y1;
    const long long j = dx < 0 ? -1 : 0, ax = (dx ^ j) - j;
    const long long i = dy < 0 ? -1 : 0, ay = (dy ^ i) - i;
    long long x_step = 0, y_step = 0;
    long long ecount;
    if (ax > ay) {
        if (j) { long long t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; }
        dy = (dy ^ j) - j;
        y_step = (dy * XY_ONE) / (ax | 1);
        ecount = (x2 - x1) >> XY_SHIFT;
    } else {
        if (i) { long long t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; }
        dx = (dx ^ i) - i;
        x_step = (dx * XY_ONE) / (ay | 1);
        ecount = (y2 - y1) >> XY_SHIFT;
    }
    x1 += XY_ONE >> 1;
    y1 += XY_ONE >> 1;
    put((x2 + (XY_ONE >> 1)) >> XY_SHIFT, (y2 + (XY_ONE >> 1)) >> XY_SHIFT);
    if (ax > ay) {
        x1 >>= XY_SHIFT;
        for (; ecount >= 0; --ecount, ++x1, y1 += y_step) put(x1, y1 >> XY_SHIFT);
    } else {
        y1 >>= XY_SHIFT;
        for (; ecount >= 0; --ecount, ++y1, x1 += x_step) put(x1 >> XY_SHIFT, y1);
    }
}

// Line(): LineIterator(img, p1, p2, 8, leftToRight) -- clipped to the frame, then Bresenham from the left end
template <typename Paint>
__device__ __forceinline__ void thin_line(int H, int W, long long x1, long long y1, long long x2, long long y2, Paint paint)
{
    if (x1 < 0 || x1 >= W || x2 < 0 || x2 >= W || y1 < 0 || y1 >= H || y2 < 0 || y2 >= H)
        if (!clip_line_to(W - 1, H - 1, x1, y1, x2, y2)) return;
    if (x2 < x1) { long long t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; }
    int dx = (int)(x2 - x1), dy = (int)(y2 - y1);
    const int sy = dy < 0 ? -1 : 1;
    dy = abs(dy);
    const bool steep = dy > dx;
    if (steep) { const int t = dx; dx = dy; dy = t; }
    int err = dx - (dy + dy);
    const int plus = dx + dx, minus = -(dy + dy);
    int x = (int)x1, y = (int)y1;
    for (int i = 0; i <= dx; ++i) {
        paint(x, y);
        const bool minor = err < 0;
        err += minus + (minor ? plus : 0);
        if (steep) { y += sy; x += minor ? 1 : 0; }
        else { x += 1; y += minor ? sy : 0; }
    }
}

// Circle(): half[k] = the half width of the widest span the midpoint walk of radius r draws on the rows cy -+ k, k = 0 .. r
__device__ __forceinline__ void circle_halfwidths(int r, short* h)
{
    for (int k = 0; k <= r; ++k) h[k] = -1;
    int err = 0, dx = r, dy = 0, plus = 1, minus = (r << 1) - 1;
    while (dx >= dy) {
        h[dy] = max((int)h[dy], dx);
        h[dx] = max((int)h[dx], dy);
        ++dy;
        err += plus;
        plus += 2;
        const int mask = (err <= 0) - 1;
        err -= minus & mask;
        dx += mask;
        minus -= mask & 2;
    }
}

// EllipseEx + ellipse2Poly (drawing.cpp), arc 0 .. 360, of the ellipse el = (x, y, ax, ay, angle in whole degrees): one lane
// per polygon point into rx / ry, then lane 0 drops the consecutive duplicates in order into vx / vy.  Called by every lane
// of the workgroup (it synchronises); returns the number of vertices through *npts_s (LDS).
__device__ __forceinline__ void ellipse_poly(const int* el, long long* vx, long long* vy, long long* rx, long long* ry, int* npts_s)
{
    const long long cxl = (long long)el[0] << XY_SHIFT, cyl = (long long)el[1] << XY_SHIFT;
    const long long aw = (long long)abs(el[2]) << XY_SHIFT, ah = (long long)abs(el[3]) << XY_SHIFT;
    int delta = (int)((max(aw, ah) + (XY_ONE >> 1)) >> XY_SHIFT);
    delta = delta < 3 ? 90 : delta < 10 ? 30 : delta < 15 ? 18 : 5;
    int angle = el[4];
    while (angle < 0) angle += 360;
    while (angle > 360) angle -= 360;
    const int npoly = (360 + delta - 1) / delta + 1;      // i = 0, delta, ... < 360 + delta
    {
        const float alpha = sin_table(450 - angle), beta = sin_table(angle);
        const double cx = (double)cxl, cy = (double)cyl;
        for (int k = threadIdx.x; k < npoly; k += blockDim.x) {
            const int t = min(k * delta, 360);
            const double x = (double)aw * (double)sin_table(450 - t), y = (double)ah * (double)sin_table(t);
            const double fx = cx + x * (double)alpha - y * (double)beta;
            const double fy = cy + x * (double)beta + y * (double)alpha;
            long long qx = cv_round(fx / (double)XY_ONE) << XY_SHIFT, qy = cv_round(fy / (double)XY_ONE) << XY_SHIFT;
            qx += cv_round(fx - (double)qx);
            qy += cv_round(fy - (double)qy);
            rx[k] = qx;
            ry[k] = qy;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int k = 0; k < npoly; ++k)
            if (n == 0 || rx[k] != vx[n - 1] || ry[k] != vy[n - 1]) { vx[n] = rx[k]; vy[n] = ry[k]; ++n; }
        if (npoly == 1 || n == 1) { vx[0] = vx[1] = cxl; vy[0] = vy[1] = cyl; n = 2; }
        *npts_s = n;
    }
    __syncthreads();
}

// FillConvexPoly (LINE_8, shift 16) without its outline: the edge walk, one span per row
template <typename Span>
__device__ __forceinline__ void convex_spans(const long long* vx, const long long* vy, int npts, int H, int W, Span span)
{
    const long long delta = XY_ONE >> 1;
    long long xmin = vx[0], xmax = vx[0], ymin = vy[0], ymax = vy[0];
    int imin = 0;
    for (int k = 0; k < npts; ++k) {
        if (vy[k] < ymin) { ymin = vy[k]; imin = k; }
        ymax = max(ymax, vy[k]); xmax = max(xmax, vx[k]); xmin = min(xmin, vx[k]);
    }
    xmin = (xmin + delta) >> XY_SHIFT; xmax = (xmax + delta) >> XY_SHIFT;
    ymin = (ymin + delta) >> XY_SHIFT; ymax = (ymax + delta) >> XY_SHIFT;
    if (npts < 3 || (int)xmax < 0 || (int)ymax < 0 || (int)xmin >= W || (int)ymin >= H) return;
    ymax = min(ymax, (long long)H - 1);
    int e_idx[2] = {imin, imin}, e_di[2] = {1, npts - 1};
    long long e_x[2] = {-XY_ONE, -XY_ONE}, e_dx[2] = {0, 0};
    int e_ye[2] = {(int)ymin, (int)ymin};
    int y = (int)ymin, edges = npts;
    do {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (y >= e_ye[s]) {
                int idx0 = e_idx[s], di = e_di[s];
                int idx = idx0 + di;
                if (idx >= npts) idx -= npts;
                for (; edges-- > 0;) {
                    const int ty = (int)((vy[idx] + delta) >> XY_SHIFT);
                    if (ty > y) {
                        const long long xs = vx[idx0], xe = vx[idx];
                        e_ye[s] = ty;
                        e_dx[s] = ((xe - xs) * 2 + (ty - y)) / (2LL * (ty - y));
                        e_x[s] = xs;
                        e_idx[s] = idx;
                        break;
                    }
                    idx0 = idx;
                    idx += di;
                    if (idx >= npts) idx -= npts;
                }
            }
        }
        if (edges < 0) break;
        if (y >= 0) {
            const int xx1 = (int)((min(e_x[0], e_x[1]) + delta) >> XY_SHIFT);      // the left edge is the smaller x
            const int xx2 = (int)((max(e_x[0], e_x[1]) + delta) >> XY_SHIFT);
            int a = 1, b = 0;                           // empty
            if (xx2 >= 0 && xx1 < W) { a = max(xx1, 0); b = min(xx2, W - 1); }
            span(y, a, b);
        }
        e_x[0] += e_dx[0];
        e_x[1] += e_dx[1];
    } while (++y <= (int)ymax);
}

}  // namespace mp_raster
