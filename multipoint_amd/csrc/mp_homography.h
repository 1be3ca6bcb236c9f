// Device functions shared by the per-pair RANSAC (homography.hip: a pair's correspondences in LDS) and the pooled one
// (homography_pooled.hip: a group's correspondences in global memory): counter-based sampling, the exact 4-point solve, the
// forward reprojection test, the 9x9 eigen-solver of the normalised-DLT refit and the pieces of the Levenberg-Marquardt
// polish.  Both files go through the same code, so the same correspondences give the same model in either.
#pragma once
#include "mp_common.h"
#include "mp_device.h"

namespace {

// 4 distinct indices in [0, n) for hypothesis t of pair p.  Never terminates for n < 4: callers leave before it.
__device__ __forceinline__ void sample4(unsigned long long seed, int p, int t, int n, int idx[4])
{
    unsigned long long ctr = mix64(seed ^ ((unsigned long long)p << 32) ^ (unsigned long long)t);
    for (int k = 0; k < 4; ++k) {
        for (;;) {
            ctr = mix64(ctr);
            const int c = (int)(ctr % (unsigned long long)n);
            bool dup = false;
            for (int j = 0; j < k; ++j) dup |= (idx[j] == c);
            if (!dup) { idx[k] = c; break; }
        }
    }
}

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

}  // namespace
