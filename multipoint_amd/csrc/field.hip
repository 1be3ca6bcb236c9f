// Local alignment correction: a smooth displacement field fitted to a lattice of measured displacements, and frames
// sampled through such a field.
//
//   field_fit_kernel   one workgroup (eight waves) per frame solves (W + lambda L) u = W d for both axes at once by
//                      Jacobi-preconditioned conjugate gradients in float64, L the graph Laplacian of the 4-neighbour lattice.  Node k
//                      belongs to thread k mod 512: the weight, the residual r and the product A p live in the caller's workspace
//                      and are touched by their own thread alone, the solution x is out_u itself.  Only the search direction p is
//                      read by neighbours; it lives in LDS while 16 bytes per node fit (8192 nodes), else in the workspace --
//                      the storage changes no bit.  An iteration has three barriers: behind p^T A p, behind r^T z and r^T r, and
//                      behind the update of p.
//                      Every sum is taken in one fixed order: a thread adds its nodes k, k + 512, ... in that order, a wave
//                      folds by butterflies (xor 32, 16, .. 1), and every thread adds the eight wave sums from wave 0 up.  So a
//                      frame has the same bits alone, in any batch, in any batch order and from run to run.
//   field_warp_kernel  one workgroup per 64 x 16 tile of dst: a wave writes one 256-byte line of a row at a time.  The nodes the
//                      tile's pixels interpolate between (a few at any stride a lattice is measured with) are staged in LDS; a tile
//                      that would need more than 1024 reads them from global memory with the same arithmetic.  The field and the
//                      position are float64, the blend of the four source taps is fp32, nothing is contracted.
//   No atomics; ordinary per-lane vector stores only.
#include "../../include/multipoint_hip.h"
#include "mp_common.h"
#include "mp_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int FIT_THREADS = 512, FIT_WAVES = FIT_THREADS / MP_WAVE, FIT_RED = 6;
constexpr int FIT_LDS_NODES = 8192;                                  // 128 KiB of search direction
constexpr double BIG = 1.7976931348623157e308;
// v[k] <- the sum of v[k] over the workgroup, the same bits in every thread.  Two buffers take turns, so one barrier is enough: a
// buffer is written again two sums later, behind the barrier of the sum in between.
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], double (*red)[FIT_WAVES][FIT_RED], int& turn, int lane, int wave)
{
    double(*buf)[FIT_RED] = red[turn & 1];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        v[k] = wave_add(v[k]);
        if (lane == 0) buf[wave][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = buf[0][k];
        for (int w = 1; w < FIT_WAVES; ++w) s += buf[w][k];
        v[k] = s;
    }
    ++turn;
}

// the lattice degree of node (i, j)
__device__ __forceinline__ int degree(int i, int j, int gy, int gx) { return (i > 0) + (j > 0) + (j < gx - 1) + (i < gy - 1); }

// (A p)_k of both axes, neighbours in the order up, left, right, down; diag = A_kk
__device__ __forceinline__ void apply(const double* p, int k, int i, int j, int gy, int gx, double wk, double lambda, double& qy,
                                      double& qx, double& diag)
{
    double sy = 0.0, sx = 0.0;
    if (i > 0) sy += p[2 * (k - gx)], sx += p[2 * (k - gx) + 1];
    if (j > 0) sy += p[2 * (k - 1)], sx += p[2 * (k - 1) + 1];
    if (j < gx - 1) sy += p[2 * (k + 1)], sx += p[2 * (k + 1) + 1];
    if (i < gy - 1) sy += p[2 * (k + gx)], sx += p[2 * (k + gx) + 1];
    diag = wk + lambda * (double)degree(i, j, gy, gx);
    qy = diag * p[2 * k] - lambda * sy;
    qx = diag * p[2 * k + 1] - lambda * sx;
}

__global__ __launch_bounds__(FIT_THREADS) void field_fit_kernel(FieldFitParams P)
{
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ double red[2][FIT_WAVES][FIT_RED];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x;
    const int gy = P.gy, gx = P.gx, N = gy * gx;
    const double lambda = P.lambda, c = P.robust_px;
    const double* d = P.d + (size_t)b * N * 2;
    const double* w0 = P.weight + (size_t)b * N;
    double* ws = P.ws + (size_t)b * N * MP_FIELD_WS_DOUBLES;
    double *w = ws, *r = ws + N, *q = ws + 3 * (size_t)N;
    double* p = P.p_in_lds ? reinterpret_cast<double*>(lds) : ws + 5 * (size_t)N;
    double* x = P.out_u + (size_t)b * N * 2;
    int turn = 0;

    // the input weight of node k as the fit takes it: zero unless it is positive and finite and d_k is finite (d_k is read only then)
    auto input = [&](int k, double& dy, double& dx, bool& bad) -> double {
        const double wk = w0[k];
        dy = dx = 0.0, bad = false;
        if (!(wk > 0.0) || !(wk <= BIG)) return 0.0;
        const double ay = d[2 * k], ax = d[2 * k + 1];
        if (!finite64(ay) || !finite64(ax)) {
            bad = true;
            return 0.0;
        }
        dy = ay, dx = ax;
        return wk;
    };

    double cnt[2] = {0.0, 0.0};
    for (int k = tid; k < N; k += FIT_THREADS) {
        double dy, dx;
        bool bad;
        const double wk = input(k, dy, dx, bad);
        w[k] = wk, x[2 * k] = 0.0, x[2 * k + 1] = 0.0;
        cnt[0] += wk > 0.0 ? 1.0 : 0.0, cnt[1] += bad ? 1.0 : 0.0;
    }
    block_sum(cnt, red, turn, lane, wave);
    int nz = (int)cnt[0];
    const int nbad = (int)cnt[1];
    int status = MP_FIELD_NO_DATA, iters = 0;
    double rel = 0.0;
    const int rounds = c > 0.0 ? P.rounds : 0;
    for (int t = 0; nz > 0; ++t) {
        if (t > 0) {                                                 // a robust round: Tukey's biweight of the residual |u_k - d_k|
            double left[1] = {0.0};
            for (int k = tid; k < N; k += FIT_THREADS) {
                double dy, dx, nw = 0.0;
                bool bad;
                const double wk = input(k, dy, dx, bad);
                if (wk > 0.0) {
                    const double ey = x[2 * k] - dy, ex = x[2 * k + 1] - dx;
                    const double e = sqrt(ey * ey + ex * ex);
                    if (e < c) {
                        const double s = e / c, g = 1.0 - s * s;
                        nw = wk * (g * g);
                    }
                }
                q[2 * k] = nw;
                left[0] += nw > 0.0 ? 1.0 : 0.0;
            }
            block_sum(left, red, turn, lane, wave);
            if (left[0] == 0.0) {                                    // the solution and the weights of the round before stay
                status = MP_FIELD_ALL_REJECTED;
                break;
            }
            nz = (int)left[0];
            for (int k = tid; k < N; k += FIT_THREADS) w[k] = q[2 * k];
        }
        // r = b - A x from the x at hand (zero in the first solve, the previous solution in a robust round), z = r / diag, p = z
        for (int k = tid; k < N; k += FIT_THREADS) p[2 * k] = x[2 * k], p[2 * k + 1] = x[2 * k + 1];
        __syncthreads();
        double s6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = tid; k < N; k += FIT_THREADS) {
            const int i = k / gx, j = k - i * gx;
            const double wk = w[k];
            const double by = wk > 0.0 ? wk * d[2 * k] : 0.0, bx = wk > 0.0 ? wk * d[2 * k + 1] : 0.0;
            double qy, qx, diag;
            apply(p, k, i, j, gy, gx, wk, lambda, qy, qx, diag);
            const double ry = by - qy, rx = bx - qx;
            r[2 * k] = ry, r[2 * k + 1] = rx;
            const double zy = ry / diag, zx = rx / diag;
            s6[0] += ry * zy, s6[1] += rx * zx, s6[2] += ry * ry, s6[3] += rx * rx, s6[4] += by * by, s6[5] += bx * bx;
        }
        block_sum(s6, red, turn, lane, wave);                        // (every read of p lies in front of this barrier)
        double rz[2] = {s6[0], s6[1]}, rr[2] = {s6[2], s6[3]};
        const double bb[2] = {s6[4], s6[5]};
        const double thr[2] = {(P.tol * P.tol) * bb[0], (P.tol * P.tol) * bb[1]};
        bool dead[2] = {false, false};                               // an axis whose p^T A p is not positive cannot go on
        for (int k = tid; k < N; k += FIT_THREADS) {
            const int i = k / gx, j = k - i * gx;
            const double diag = w[k] + lambda * (double)degree(i, j, gy, gx);
            p[2 * k] = r[2 * k] / diag, p[2 * k + 1] = r[2 * k + 1] / diag;
        }
        __syncthreads();
        int it = 0;
        while (it < P.max_iter) {
            const bool act[2] = {rr[0] > thr[0] && !dead[0], rr[1] > thr[1] && !dead[1]};
            if (!act[0] && !act[1]) break;
            double pq[2] = {0.0, 0.0};
            for (int k = tid; k < N; k += FIT_THREADS) {
                const int i = k / gx, j = k - i * gx;
                double qy, qx, diag;
                apply(p, k, i, j, gy, gx, w[k], lambda, qy, qx, diag);
                q[2 * k] = qy, q[2 * k + 1] = qx;
                pq[0] += p[2 * k] * qy, pq[1] += p[2 * k + 1] * qx;
            }
            block_sum(pq, red, turn, lane, wave);
            double alpha[2];
            bool step[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                step[a] = act[a] && pq[a] > 0.0;
                if (act[a] && !step[a]) dead[a] = true;
                alpha[a] = step[a] ? rz[a] / pq[a] : 0.0;
            }
            double s4[4] = {0.0, 0.0, 0.0, 0.0};
            for (int k = tid; k < N; k += FIT_THREADS) {
                const int i = k / gx, j = k - i * gx;
                const double diag = w[k] + lambda * (double)degree(i, j, gy, gx);
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    double ra = r[2 * k + a];
                    if (step[a]) {
                        x[2 * k + a] += alpha[a] * p[2 * k + a];
                        ra -= alpha[a] * q[2 * k + a];
                        r[2 * k + a] = ra;
                    }
                    s4[a] += ra * (ra / diag), s4[2 + a] += ra * ra;
                }
            }
            block_sum(s4, red, turn, lane, wave);
            double beta[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                beta[a] = step[a] ? s4[a] / rz[a] : 0.0;
                if (step[a]) rz[a] = s4[a], rr[a] = s4[2 + a];
            }
            for (int k = tid; k < N; k += FIT_THREADS) {
                const int i = k / gx, j = k - i * gx;
                const double diag = w[k] + lambda * (double)degree(i, j, gy, gx);
#pragma unroll
                for (int a = 0; a < 2; ++a)
                    if (step[a]) p[2 * k + a] = r[2 * k + a] / diag + beta[a] * p[2 * k + a];
            }
            __syncthreads();
            ++it;
        }
        iters = it;
        rel = 0.0;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const double ra = bb[a] > 0.0 ? sqrt(rr[a] / bb[a]) : rr[a] > 0.0 ? __builtin_inf() : 0.0;
            rel = ra <= rel ? rel : ra;                               // (NaN stays)
        }
        // the rule must be MET: a sum that is not finite (weights so large that w d or its square overflows) meets nothing
        const bool met = rr[0] <= thr[0] && rr[1] <= thr[1] && finite64(bb[0]) && finite64(bb[1]);
        status = met ? MP_FIELD_OK : MP_FIELD_MAX_ITER;
        if (t >= rounds) break;
    }
    if (P.out_w)
        for (int k = tid; k < N; k += FIT_THREADS) P.out_w[(size_t)b * N + k] = w[k];
    if (tid == 0) {
        int* info = P.out_info + (size_t)b * MP_FIELD_INFO_INTS;
        info[0] = status, info[1] = iters, info[2] = nz, info[3] = nbad;
        P.out_res[b] = rel;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
constexpr int WARP_TW = 64, WARP_TH = 16, WARP_THREADS = 256, WARP_NODES = 1024;
constexpr double FAR = 1073741824.0;                                 // 2^30

// clamp(floor(t), 0, max(g - 2, 0)): the lattice cell of coordinate t
__device__ __forceinline__ int cell(double t, int g)
{
    const double hi = (double)(g > 2 ? g - 2 : 0);
    const double f = floor(t);
    return (int)(f < 0.0 ? 0.0 : f > hi ? hi : f);
}

// cell and fraction of pixel coordinate v on an axis with g nodes
__device__ __forceinline__ void locate(double v, double origin, double step, int g, int extrapolate, int& i, int& i1, double& f)
{
    const double t = (v - origin) / step;
    i = cell(t, g);
    i1 = i + 1 < g ? i + 1 : g - 1;
    f = t - (double)i;
    if (!extrapolate) f = f < 0.0 ? 0.0 : f > 1.0 ? 1.0 : f;
    if (g == 1) f = 0.0;
}

__global__ __launch_bounds__(WARP_THREADS) void field_warp_kernel(FieldWarpParams P)
{
    __shared__ double2 nodes[WARP_NODES];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int xa = blockIdx.x * WARP_TW, ya = blockIdx.y * WARP_TH;
    const int xb = min(xa + WARP_TW, P.W) - 1, yb = min(ya + WARP_TH, P.H) - 1;
    const double2* u = reinterpret_cast<const double2*>(P.u) + (size_t)b * P.gy * P.gx;
    // floor and clamp are monotone: every pixel of the tile has its cell between the cells of the tile's first and last pixel
    int ja, jb, ia, ib, unused;
    double f;
    locate((double)xa, P.x0, P.step, P.gx, 1, ja, unused, f);
    locate((double)xb, P.x0, P.step, P.gx, 1, unused, jb, f);
    locate((double)ya, P.y0, P.step, P.gy, 1, ia, unused, f);
    locate((double)yb, P.y0, P.step, P.gy, 1, unused, ib, f);
    const int jn = jb - ja + 1, in = ib - ia + 1;
    const bool staged = in * jn <= WARP_NODES;
    if (staged)
        for (int n = tid; n < in * jn; n += WARP_THREADS) {
            const int ii = n / jn, jj = n - ii * jn;
            nodes[n] = u[(size_t)(ia + ii) * P.gx + (ja + jj)];
        }
    __syncthreads();
    const int x = xa + (tid & 63);
    if (x >= P.W) return;
    auto node = [&](int i, int j) -> double2 { return staged ? nodes[(i - ia) * jn + (j - ja)] : u[(size_t)i * P.gx + j]; };
    int j, j1;
    double fx;
    locate((double)x, P.x0, P.step, P.gx, P.extrapolate, j, j1, fx);
    const float* S = P.src + (P.n_src > 1 ? (size_t)b * P.Hs * P.Ws : 0);
    const double* h = P.hom ? P.hom + (size_t)b * 9 : nullptr;
    for (int y = ya + (tid >> 6); y <= yb; y += WARP_THREADS / 64) {
        int i, i1;
        double fy;
        locate((double)y, P.y0, P.step, P.gy, P.extrapolate, i, i1, fy);
        const double2 u00 = node(i, j), u01 = node(i, j1), u10 = node(i1, j), u11 = node(i1, j1);
        const double uy = (u00.x * (1.0 - fx) + u01.x * fx) * (1.0 - fy) + (u10.x * (1.0 - fx) + u11.x * fx) * fy;
        const double ux = (u00.y * (1.0 - fx) + u01.y * fx) * (1.0 - fy) + (u10.y * (1.0 - fx) + u11.y * fx) * fy;
        double qy = (double)y + uy, qx = (double)x + ux;
        bool ok = finite64(qy) && finite64(qx);
        if (h) {
            const double X = (h[0] * qx + h[1] * qy) + h[2], Y = (h[3] * qx + h[4] * qy) + h[5], Z = (h[6] * qx + h[7] * qy) + h[8];
            ok = ok && finite64(X) && finite64(Y) && finite64(Z) && Z > 0.0;
            qy = Y / Z, qx = X / Z;
        }
        ok = ok && fabs(qy) <= FAR && fabs(qx) <= FAR;               // (false for NaN)
        float out = 0.f;
        unsigned char v = 0;
        if (ok) {
            const double gy0 = floor(qy), gx0 = floor(qx);
            const int iy = (int)gy0, ix = (int)gx0;
            const float fyf = (float)(qy - gy0), fxf = (float)(qx - gx0);
            const float wy0 = 1.f - fyf, wy1 = fyf, wx0 = 1.f - fxf, wx1 = fxf;
            const bool iny0 = iy >= 0 && iy < P.Hs, iny1 = iy + 1 >= 0 && iy + 1 < P.Hs;
            const bool inx0 = ix >= 0 && ix < P.Ws, inx1 = ix + 1 >= 0 && ix + 1 < P.Ws;
            const float s00 = iny0 && inx0 ? S[(size_t)iy * P.Ws + ix] : 0.f;
            const float s01 = iny0 && inx1 ? S[(size_t)iy * P.Ws + ix + 1] : 0.f;
            const float s10 = iny1 && inx0 ? S[(size_t)(iy + 1) * P.Ws + ix] : 0.f;
            const float s11 = iny1 && inx1 ? S[(size_t)(iy + 1) * P.Ws + ix + 1] : 0.f;
            out = (s00 * wx0 + s01 * wx1) * wy0 + (s10 * wx0 + s11 * wx1) * wy1;
            // a tap's weight is non-zero when both its factors are; 1 - f and f are never both zero, so the rule splits by axis
            v = (wy0 == 0.f || iny0) && (wy1 == 0.f || iny1) && (wx0 == 0.f || inx0) && (wx1 == 0.f || inx1);
        }
        const size_t at = ((size_t)b * P.H + y) * P.W + x;
        P.dst[at] = out;
        if (P.valid) P.valid[at] = v;
    }
}

}  // namespace

size_t field_fit_lds_bytes(int nodes) { return nodes <= FIT_LDS_NODES ? (size_t)nodes * 2 * sizeof(double) : 0; }

hipError_t launch_field_fit(const FieldFitParams& p, int B, hipStream_t s)
{
    const size_t bytes = p.p_in_lds ? field_fit_lds_bytes(p.gy * p.gx) : 0;
    if (bytes > 0) {                                                 // more than the 64 KiB a launch gets unasked
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&field_fit_kernel),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)field_fit_lds_bytes(FIT_LDS_NODES));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(field_fit_kernel, dim3((unsigned)B), dim3(FIT_THREADS), bytes, s, p);
    return hipSuccess;
}

void launch_field_warp(const FieldWarpParams& p, int B, hipStream_t s)
{
    const dim3 grid((unsigned)((p.W + WARP_TW - 1) / WARP_TW), (unsigned)((p.H + WARP_TH - 1) / WARP_TH), (unsigned)B);
    hipLaunchKernelGGL(field_warp_kernel, grid, dim3(WARP_THREADS), 0, s, p);
}
