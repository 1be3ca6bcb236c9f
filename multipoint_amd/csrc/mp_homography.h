// The homography estimators' device code, written once (homography.hip: one model per pair; homography_pooled.hip: one model
// per group of pairs): the exact 4-point solve and the forward reprojection test -- the Homography model of the scoring kernels
// in mp_ransac.h --, the normalised-DLT refit and the Levenberg-Marquardt polish.
// refit_kernel, refine_kernel and lm_sums are templates on the point view (mp_ransac.h: PairView, a pair's list in LDS, or
// PooledView, a group's rows in global memory).  Every floating-point operation, reduction and barrier is in the shared body, so
// the same correspondences give the same bits on either route.
#pragma once
#include "mp_ransac.h"

namespace {

// exact homography through 4 correspondences (x,y) -> (u,v); h[8] = 1.  false if (near-)singular.
__device__ bool solve4(const double* x, const double* y, const double* u, const double* v, double* h)
{
    double a[8][9];
    for (int k = 0; k < 4; ++k) {
        double* r0 = a[2 * k];
        double* r1 = a[2 * k + 1];
        r0[0] = x[k]; r0[1] = y[k]; r0[2] = 1.0; r0[3] = 0.0; r0[4] = 0.0; r0[5] = 0.0; r0[6] = -u[k] * x[k]; r0[7] = -u[k] * y[k]; r0[8] = u[k];
        r1[0] = 0.0; r1[1] = 0.0; r1[2] = 0.0; r1[3] = x[k]; r1[4] = y[k]; r1[5] = 1.0; r1[6] = -v[k] * x[k]; r1[7] = -v[k] * y[k]; r1[8] = v[k];
    }
    for (int c = 0; c < 8; ++c) {
        int piv = c;
        double best = fabs(a[c][c]);
        for (int r = c + 1; r < 8; ++r)
            if (fabs(a[r][c]) > best) { best = fabs(a[r][c]); piv = r; }
        if (best < 1e-10) return false;
        if (piv != c)
            for (int k = c; k < 9; ++k) { const double tmp = a[c][k]; a[c][k] = a[piv][k]; a[piv][k] = tmp; }
        const double inv = 1.0 / a[c][c];
        for (int r = c + 1; r < 8; ++r) {
            const double f = a[r][c] * inv;
            for (int k = c; k < 9; ++k) a[r][k] -= f * a[c][k];
        }
    }
    for (int c = 7; c >= 0; --c) {
        double s = a[c][8];
        for (int k = c + 1; k < 8; ++k) s -= a[c][k] * h[k];
        h[c] = s / a[c][c];
    }
    h[8] = 1.0;
    return true;
}

__device__ __forceinline__ bool inlier(const double* h, double x, double y, double u, double v, double thr2)
{
    const double w = h[6] * x + h[7] * y + h[8];
    if (fabs(w) < 1e-12) return false;
    const double iw = 1.0 / w;
    const double du = (h[0] * x + h[1] * y + h[2]) * iw - u, dv = (h[3] * x + h[4] * y + h[5]) * iw - v;
    return du * du + dv * dv <= thr2;
}

// The homography as a model of the scoring kernels (mp_ransac.h): nine coefficients, h[8] = 1 from the minimal solve.  The two
// functions are NAMED here, not wrapped: a forwarding member in front of solve4 changes the order in which the compiler meets the
// functions of a unit, and with it the fp64 contractions of refit_kernel (the note in front of that kernel).
struct Homography {
    static constexpr int S = 4;          // minimal sample
    static constexpr int COEFFS = 9;
    static constexpr auto minimal = solve4;
    static constexpr auto inlier = ::inlier;
};

// symmetric 9x9 eigen-decomposition by cyclic Jacobi; returns the eigenvector of the smallest eigenvalue
__device__ void smallest_eigvec9(double a[9][9], double* out)
{
    double vv[9][9];
    for (int i = 0; i < 9; ++i) for (int j = 0; j < 9; ++j) vv[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0;
        for (int i = 0; i < 9; ++i) for (int j = i + 1; j < 9; ++j) off += a[i][j] * a[i][j];
        if (off < 1e-30) break;
        for (int pch = 0; pch < 9; ++pch)
            for (int q = pch + 1; q < 9; ++q) {
                if (fabs(a[pch][q]) < 1e-300) continue;
                const double theta = (a[q][q] - a[pch][pch]) / (2.0 * a[pch][q]);
                const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
                for (int k = 0; k < 9; ++k) {
                    const double akp = a[k][pch], akq = a[k][q];
                    a[k][pch] = c * akp - s * akq; a[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 9; ++k) {
                    const double apk = a[pch][k], aqk = a[q][k];
                    a[pch][k] = c * apk - s * aqk; a[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 9; ++k) {
                    const double vkp = vv[k][pch], vkq = vv[k][q];
                    vv[k][pch] = c * vkp - s * vkq; vv[k][q] = s * vkp + c * vkq;
                }
            }
    }
    int m = 0;
    for (int i = 1; i < 9; ++i) if (a[i][i] < a[m][m]) m = i;
    for (int k = 0; k < 9; ++k) out[k] = vv[k][m];
}

// the last step of the normalised-DLT refit, on one thread: the eigenvector of the smallest eigenvalue of ata (A^T A of the
// 2m x 9 DLT matrix on the normalised points), denormalised with the two point sets' centroids (cx, cy), (cu, cv) and scales
// s1, s2, divided by h22 and written to H_out[0..9)
__device__ void dlt_finish(const double* ata, double cx, double cy, double cu, double cv, double s1, double s2, double* H_out)
{
    double a[9][9], hv[9];
    for (int i = 0; i < 9; ++i) for (int j = 0; j < 9; ++j) a[i][j] = ata[i * 9 + j];
    smallest_eigvec9(a, hv);
    // denormalise: H = T2^-1 * Hn * T1, T = [[s,0,-s*c],[0,s,-s*c],[0,0,1]]
    const double hn[3][3] = {{hv[0], hv[1], hv[2]}, {hv[3], hv[4], hv[5]}, {hv[6], hv[7], hv[8]}};
    double tmp[3][3];
    for (int r = 0; r < 3; ++r) {            // Hn * T1
        tmp[r][0] = hn[r][0] * s1; tmp[r][1] = hn[r][1] * s1;
        tmp[r][2] = -hn[r][0] * s1 * cx - hn[r][1] * s1 * cy + hn[r][2];
    }
    double out[3][3];
    for (int c = 0; c < 3; ++c) {            // T2^-1 = [[1/s,0,cu],[0,1/s,cv],[0,0,1]]
        out[0][c] = tmp[0][c] / s2 + cu * tmp[2][c];
        out[1][c] = tmp[1][c] / s2 + cv * tmp[2][c];
        out[2][c] = tmp[2][c];
    }
    const double nrm = fabs(out[2][2]) > 1e-300 ? 1.0 / out[2][2] : 1.0;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) H_out[r * 3 + c] = out[r][c] * nrm;
}

// One workgroup of 256 threads per pair / group: re-derive the winning hypothesis best[index], mark its inliers in the view,
// refit by normalised DLT over them.  H_out[index] and n_inliers[index] are zero if there is no model.
// (The body is the kernel itself and not a function that two kernels call: how the compiler contracts a sum of two products
// into a multiply-add, as in smallest_eigvec9's rotations, depends on how deep the code sits in the inlining order.)
template <class Source>
__global__ __launch_bounds__(256) void refit_kernel(Source src, double thr, unsigned long long seed,
                                                    const unsigned long long* __restrict__ best, double* __restrict__ H_out,
                                                    int* __restrict__ n_inliers)
{
    __shared__ double red[256];
    __shared__ double hsh[9];
    __shared__ double ata[81];
    const int index = blockIdx.x, tid = threadIdx.x;
    const auto pv = src.view(index);
    const int n = pv.n;
    const unsigned long long b = best[index];
    const int cnt = (int)(b >> 32);
    if (n < 4 || cnt < 4) {
        if (tid == 0) { n_inliers[index] = 0; for (int k = 0; k < 9; ++k) H_out[index * 9 + k] = 0.0; }
        return;
    }
    if (tid == 0) {
        double h[9];
        hypothesis<Homography>(pv, seed, index, 0x7fffffff - (int)(b & 0xffffffffull), h);
        for (int k = 0; k < 9; ++k) hsh[k] = h[k];
    }
    __syncthreads();
    // inlier flags of the best hypothesis + normalisation statistics (centroid, mean distance) of both point sets
    const double thr2 = thr * thr;
    double h[9];
    for (int k = 0; k < 9; ++k) h[k] = hsh[k];
    double sx = 0, sy = 0, su = 0, sv = 0, sc = 0;
    for (int i = tid; i < n; i += 256) {
        const float4 q = pv.get(i);
        const bool in = inlier(h, q.x, q.y, q.z, q.w, thr2);
        pv.set_inlier(i, in);
        if (in) { sx += q.x; sy += q.y; su += q.z; sv += q.w; sc += 1.0; }
    }
    const double m = block_sum(sc, red);
    const double cx = block_sum(sx, red) / m, cy = block_sum(sy, red) / m, cu = block_sum(su, red) / m, cv = block_sum(sv, red) / m;
    double d1 = 0, d2 = 0;
    for (int i = tid; i < n; i += 256) {
        if (!pv.is_inlier(i)) continue;
        const float4 q = pv.get(i);
        d1 += sqrt((q.x - cx) * (q.x - cx) + (q.y - cy) * (q.y - cy));
        d2 += sqrt((q.z - cu) * (q.z - cu) + (q.w - cv) * (q.w - cv));
    }
    const double md1 = block_sum(d1, red) / m, md2 = block_sum(d2, red) / m;
    const double s1 = md1 > 1e-12 ? 1.4142135623730951 / md1 : 1.0, s2 = md2 > 1e-12 ? 1.4142135623730951 / md2 : 1.0;
    // A^T A of the 2m x 9 DLT matrix on the normalised points: every thread sums its points' share of the 45 entries of the
    // upper triangle, thread 0 collects the block sums
    double acc9[45];
    for (int k = 0; k < 45; ++k) acc9[k] = 0.0;
    for (int i = tid; i < n; i += 256) {
        if (!pv.is_inlier(i)) continue;
        const float4 q = pv.get(i);
        const double x = (q.x - cx) * s1, y = (q.y - cy) * s1;
        const double u = (q.z - cu) * s2, v = (q.w - cv) * s2;
        const double r0[9] = {x, y, 1.0, 0.0, 0.0, 0.0, -u * x, -u * y, -u};
        const double r1[9] = {0.0, 0.0, 0.0, x, y, 1.0, -v * x, -v * y, -v};
        int k = 0;
        for (int a = 0; a < 9; ++a) for (int c = a; c < 9; ++c, ++k) acc9[k] += r0[a] * r0[c] + r1[a] * r1[c];
    }
    {
        int k = 0;
        for (int a = 0; a < 9; ++a)
            for (int c = a; c < 9; ++c, ++k) {
                const double s = block_sum(acc9[k], red);
                if (tid == 0) { ata[a * 9 + c] = s; ata[c * 9 + a] = s; }
            }
    }
    __syncthreads();
    if (tid == 0) {
        dlt_finish(ata, cx, cy, cu, cv, s1, s2, H_out + index * 9);
        n_inliers[index] = (int)m;
    }
}

// ---- the Levenberg-Marquardt polish ----
// What cv2.findHomography does after its refit (HomographyRefineCallback + createLMSolver(cb, 10)): minimise the forward
// reprojection residuals (x' - u, y' - v) over the inliers in the 8 parameters h0..h7 (h8 = 1).  lambda starts at 1e-3; an
// iteration tries up to 8 steps (J^T J + lambda diag(J^T J))^-1 (-J^T r), accepts the first one that lowers the cost
// (lambda <- max(0.1 lambda, 1e-12)) and multiplies lambda by 10 after every other one; an iteration without an accepted
// step ends the polish.  One workgroup per pair (or group), fp64 throughout.

constexpr int LM_SUMS = 45;       // J^T J upper triangle (36) | J^T r (8) | cost

// solves the symmetric 8x8 system (A + lam diag(A)) x = -g, A given by its upper triangle in row order; false: singular
__device__ bool lm_step(const double* sums, double lam, double* step)
{
    double a[8][9];
    for (int r = 0, k = 0; r < 8; ++r)
        for (int c = r; c < 8; ++c, ++k) { a[r][c] = sums[k]; a[c][r] = sums[k]; }
    for (int r = 0; r < 8; ++r) { a[r][r] += lam * a[r][r]; a[r][8] = -sums[36 + r]; }
    for (int c = 0; c < 8; ++c) {
        int piv = c;
        double best = fabs(a[c][c]);
        for (int r = c + 1; r < 8; ++r)
            if (fabs(a[r][c]) > best) { best = fabs(a[r][c]); piv = r; }
        if (!(best > 0.0) || !isfinite(best)) return false;
        if (piv != c)
            for (int k = c; k < 9; ++k) { const double tmp = a[c][k]; a[c][k] = a[piv][k]; a[piv][k] = tmp; }
        const double inv = 1.0 / a[c][c];
        for (int r = c + 1; r < 8; ++r) {
            const double f = a[r][c] * inv;
            for (int k = c; k < 9; ++k) a[r][k] -= f * a[c][k];
        }
    }
    for (int c = 7; c >= 0; --c) {
        double s = a[c][8];
        for (int k = c + 1; k < 8; ++k) s -= a[c][k] * step[k];
        step[c] = s / a[c][c];
    }
    return true;
}

// adds one inlier (X, Y) -> (U, V) at parameters h to a thread's sums of J^T J, J^T r and r.r
__device__ __forceinline__ void lm_add_point(double* acc /* [LM_SUMS] */, const double* h, float Xf, float Yf, float Uf, float Vf)
{
    const double X = Xf, Y = Yf;
    double ww = h[6] * X + h[7] * Y + 1.0;
    ww = fabs(ww) > 2.220446049250313e-16 ? 1.0 / ww : 0.0;
    const double xi = (h[0] * X + h[1] * Y + h[2]) * ww, yi = (h[3] * X + h[4] * Y + h[5]) * ww;
    const double rx = xi - Uf, ry = yi - Vf;
    const double jx[8] = {X * ww, Y * ww, ww, 0.0, 0.0, 0.0, -X * ww * xi, -Y * ww * xi};
    const double jy[8] = {0.0, 0.0, 0.0, X * ww, Y * ww, ww, -X * ww * yi, -Y * ww * yi};
#pragma unroll
    for (int a = 0, k = 0; a < 8; ++a) {
#pragma unroll
        for (int c = a; c < 8; ++c, ++k) acc[k] += jx[a] * jx[c] + jy[a] * jy[c];
    }
#pragma unroll
    for (int a = 0; a < 8; ++a) acc[36 + a] += jx[a] * rx + jy[a] * ry;
    acc[44] += rx * rx + ry * ry;
}

// out[0..44] = the 256 threads' sums added in a fixed order: the lanes of a wave by the xor butterfly, the four waves' sums in
// wave order through LDS -- the same bits on every run.  All 256 threads call it.
__device__ __forceinline__ void lm_reduce(const double* acc, double* wave_part /* [4][LM_SUMS] LDS */, double* out)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < LM_SUMS; ++k) {
        double v = acc[k];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if ((tid & 63) == 0) wave_part[(tid >> 6) * LM_SUMS + k] = v;
    }
    __syncthreads();
    if (tid < LM_SUMS)
        out[tid] = ((wave_part[tid] + wave_part[LM_SUMS + tid]) + wave_part[2 * LM_SUMS + tid]) + wave_part[3 * LM_SUMS + tid];
    __syncthreads();
}

// out[0..44] = the sums of J^T J, J^T r and r.r at parameters h over the view's inliers.  Fixed order: a thread adds its inliers
// i = tid, tid + 256, ..., then lm_reduce.  All 256 threads call it.
template <class View>
__device__ void lm_sums(View pv, const double* h, double* wave_part /* [4][LM_SUMS] LDS */, double* out)
{
    double acc[LM_SUMS];
#pragma unroll
    for (int k = 0; k < LM_SUMS; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < pv.n; i += 256) {
        if (!pv.is_inlier(i)) continue;
        const float4 q = pv.get(i);
        lm_add_point(acc, h, q.x, q.y, q.z, q.w);
    }
    lm_reduce(acc, wave_part, out);
}

// One workgroup of 256 threads per pair / group: mark the inliers of the input estimate H_io[index] in the view and polish it
// over them.  cost_out (may be NULL): [index][2] = the cost before and after.
template <class Source>
__global__ __launch_bounds__(256) void refine_kernel(Source src, double thr, int iters, double* __restrict__ H_io,
                                                     int* __restrict__ n_inliers, double* __restrict__ cost_out)
{
    __shared__ double wave_part[4 * LM_SUMS];
    __shared__ double cur[LM_SUMS], cand[LM_SUMS];     // the sums at the accepted parameters / at the step being tried
    __shared__ double hcur[8], htry[8];
    __shared__ int count_s[4], state;                  // state: 0 = the trial's system was singular, 1 = evaluate htry
    const int index = blockIdx.x, tid = threadIdx.x;
    const auto pv = src.view(index);
    const int n = pv.n;
    double h[9];
    for (int k = 0; k < 9; ++k) h[k] = H_io[index * 9 + k];
    // the inliers of the INPUT estimate (an all-zero matrix has none: inlier() refuses w = 0)
    const double thr2 = thr * thr;
    int mine = 0;
    for (int i = tid; i < n; i += 256) {
        const float4 q = pv.get(i);
        const bool in = inlier(h, q.x, q.y, q.z, q.w, thr2);
        pv.set_inlier(i, in);
        if (in) ++mine;
    }
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if ((tid & 63) == 0) count_s[tid >> 6] = mine;
    __syncthreads();
    const int m = count_s[0] + count_s[1] + count_s[2] + count_s[3];
    if (m < 4 || !(fabs(h[8]) > 0.0) || !isfinite(h[8])) {
        if (tid == 0) {
            n_inliers[index] = m;
            for (int k = 0; k < 9; ++k) H_io[index * 9 + k] = 0.0;
            if (cost_out) { cost_out[index * 2] = 0.0; cost_out[index * 2 + 1] = 0.0; }
        }
        return;
    }
    if (tid < 8) hcur[tid] = h[tid] / h[8];
    __syncthreads();
    lm_sums(pv, hcur, wave_part, cur);
    const double cost0 = cur[44];
    double lam = 1e-3;                                  // (every thread follows thread 0's decisions through `state` and the sums)
    for (int it = 0; it < iters; ++it) {
        bool accepted = false;
        for (int trial = 0; trial < 8 && !accepted; ++trial) {
            if (tid == 0) {
                double step[8];
                const bool ok = lm_step(cur, lam, step);
                for (int k = 0; k < 8; ++k) htry[k] = hcur[k] + step[k];
                state = ok ? 1 : 0;
            }
            __syncthreads();
            const bool ok = state != 0;
            if (ok) lm_sums(pv, htry, wave_part, cand);
            accepted = ok && cand[44] < cur[44];         // (a NaN cost is not an improvement)
            __syncthreads();
            if (accepted) {
                if (tid < LM_SUMS) cur[tid] = cand[tid];
                if (tid < 8) hcur[tid] = htry[tid];
                lam = fmax(lam * 0.1, 1e-12);
            } else {
                lam *= 10.0;
            }
            __syncthreads();
        }
        if (!accepted) break;
    }
    if (tid == 0) {
        n_inliers[index] = m;
        for (int k = 0; k < 8; ++k) H_io[index * 9 + k] = hcur[k];
        H_io[index * 9 + 8] = 1.0;
        if (cost_out) { cost_out[index * 2] = cost0; cost_out[index * 2 + 1] = cur[44]; }
    }
}

}  // namespace
