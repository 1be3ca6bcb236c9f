// The similarity and affine estimators' device code (transform.hip: one model per pair; transform_pooled.hip: one model per
// group of pairs), next to the homography's in mp_homography.h and on the same routes: the ordered compaction, point views and
// sources, counter-based sampling, fixed-order block sums and scoring kernels of mp_ransac.h.  What differs is the model:
//   Similarity  [[a, -b, tx], [b, a, ty], [0, 0, 1]]   minimal sample 2 distinct points, closed form
//   Affine      [[a,  b, tx], [c, d, ty], [0, 0, 1]]   minimal sample 3 non-collinear points, 3x3 elimination
// Both are carried as the six coefficients m[0..5] of the top two rows, so one inlier test (no division) serves both.  The
// refit over a consensus set is the exact least-squares minimiser of the summed squared forward error (closed form on centred
// points / 3x3 normal equations on centred source points), so there is no Levenberg-Marquardt polish: "refine" is local
// optimisation, rounds of { mark the inliers of the current model, refit over them } until the set stops changing.
#pragma once
#include "mp_ransac.h"

namespace {

// ---- the inlier set of a view, kept in the mask bytes alone ----
// (the homography bodies mark a pair's outliers by a NaN in the LDS list, which ends a point's life after one marking; the
// rounds of the refinement mark every point again, so here the set lives in the mask for both views.  A thread reads only
// bytes it wrote itself: every pass walks i = tid, tid + 256, ...; the launchers' callers zero the mask)
__device__ __forceinline__ bool in_set(const PairView& pv, int i) { return pv.mask_row[pv.qidx[i]] != 0; }
__device__ __forceinline__ void put_set(const PairView& pv, int i, bool in) { pv.mask_row[pv.qidx[i]] = in ? 1 : 0; }
__device__ __forceinline__ bool in_set(const PooledView& pv, int i) { return pv.mask[i] != 0; }
__device__ __forceinline__ void put_set(const PooledView& pv, int i, bool in) { pv.mask[i] = in ? 1 : 0; }

// squared forward error of (x, y) -> (u, v) under m
__device__ __forceinline__ double error2(const double* m, double x, double y, double u, double v)
{
    const double du = m[0] * x + m[1] * y + m[2] - u, dv = m[3] * x + m[4] * y + m[5] - v;
    return du * du + dv * dv;
}

// A z = r0 and A z = r1 for one 3x3 matrix by Gaussian elimination with partial pivoting (solve4's style and pivot bound);
// false if (near-)singular
__device__ bool solve3(double a[3][5], double* z0, double* z1)
{
    for (int c = 0; c < 3; ++c) {
        int piv = c;
        double best = fabs(a[c][c]);
        for (int r = c + 1; r < 3; ++r)
            if (fabs(a[r][c]) > best) { best = fabs(a[r][c]); piv = r; }
        if (!(best >= 1e-10)) return false;                 // (also refuses a NaN pivot)
        if (piv != c)
            for (int k = c; k < 5; ++k) { const double tmp = a[c][k]; a[c][k] = a[piv][k]; a[piv][k] = tmp; }
        const double inv = 1.0 / a[c][c];
        for (int r = c + 1; r < 3; ++r) {
            const double f = a[r][c] * inv;
            for (int k = c; k < 5; ++k) a[r][k] -= f * a[c][k];
        }
    }
    for (int c = 2; c >= 0; --c) {
        double s0 = a[c][3], s1 = a[c][4];
        for (int k = c + 1; k < 3; ++k) { s0 -= a[c][k] * z0[k]; s1 -= a[c][k] * z1[k]; }
        z0[c] = s0 / a[c][c];
        z1[c] = s1 / a[c][c];
    }
    return true;
}

// what the two models share as models of the scoring kernels (mp_ransac.h)
struct TopTwoRows {
    static constexpr int COEFFS = 6;
    __device__ __forceinline__ static bool inlier(const double* m, double x, double y, double u, double v, double thr2)
    {
        return error2(m, x, y, u, v) <= thr2;
    }
};

struct Similarity : TopTwoRows {
    static constexpr int S = 2;          // minimal sample
    static constexpr int SUMS = 3;       // centred sums of the refit
    // exact model through 2 correspondences: with d = p1 - p0, e = q1 - q0, (a + ib) = e conj(d) / |d|^2
    __device__ static bool minimal(const double* x, const double* y, const double* u, const double* v, double* m)
    {
        const double dx = x[1] - x[0], dy = y[1] - y[0], ex = u[1] - u[0], ey = v[1] - v[0];
        const double dd = dx * dx + dy * dy;
        if (!(dd >= 1e-10)) return false;
        const double a = (dx * ex + dy * ey) / dd, b = (dx * ey - dy * ex) / dd;
        m[0] = a; m[1] = -b; m[2] = u[0] - (a * x[0] - b * y[0]);
        m[3] = b; m[4] = a; m[5] = v[0] - (b * x[0] + a * y[0]);
        return true;
    }
    // a centred correspondence's share of the sums
    __device__ static void add(double* acc, double x, double y, double u, double v)
    {
        acc[0] += x * u + y * v;
        acc[1] += x * v - y * u;
        acc[2] += x * x + y * y;
    }
    // the least-squares model from the sums and the centroids (cx, cy) -> (cu, cv); cnt: members of the set
    __device__ static bool finish(const double* sum, double cnt, double cx, double cy, double cu, double cv, double* m)
    {
        if (!(sum[2] >= 1e-10)) return false;
        const double a = sum[0] / sum[2], b = sum[1] / sum[2];
        m[0] = a; m[1] = -b; m[2] = cu - (a * cx - b * cy);
        m[3] = b; m[4] = a; m[5] = cv - (b * cx + a * cy);
        return true;
    }
};

struct Affine : TopTwoRows {
    static constexpr int S = 3;
    static constexpr int SUMS = 11;
    // exact model through 3 correspondences: rows (x, y, 1) against u and v
    __device__ static bool minimal(const double* x, const double* y, const double* u, const double* v, double* m)
    {
        double a[3][5];
        for (int k = 0; k < 3; ++k) { a[k][0] = x[k]; a[k][1] = y[k]; a[k][2] = 1.0; a[k][3] = u[k]; a[k][4] = v[k]; }
        return solve3(a, m, m + 3);
    }
    // sums of the normal equations on (x, y, 1): xx xy yy x y | xu yu u | xv yv v
    __device__ static void add(double* acc, double x, double y, double u, double v)
    {
        acc[0] += x * x; acc[1] += x * y; acc[2] += y * y; acc[3] += x; acc[4] += y;
        acc[5] += x * u; acc[6] += y * u; acc[7] += u;
        acc[8] += x * v; acc[9] += y * v; acc[10] += v;
    }
    __device__ static bool finish(const double* sum, double cnt, double cx, double cy, double cu, double cv, double* m)
    {
        double a[3][5] = {{sum[0], sum[1], sum[3], sum[5], sum[8]},
                          {sum[1], sum[2], sum[4], sum[6], sum[9]},
                          {sum[3], sum[4], cnt, sum[7], sum[10]}};
        double z0[3], z1[3];
        if (!solve3(a, z0, z1)) return false;
        m[0] = z0[0]; m[1] = z0[1]; m[2] = cu + z0[2] - (z0[0] * cx + z0[1] * cy);
        m[3] = z1[0]; m[4] = z1[1]; m[5] = cv + z1[2] - (z1[0] * cx + z1[1] * cy);
        return true;
    }
};

// ---- pieces of the refit and the refinement; all 256 threads of the workgroup call each of them ----
// Marks the inliers of m in the view.  Returns their number; changed: whether any mask byte flipped.
template <class View>
__device__ int mark_inliers(View pv, const double* m, double thr2, double* red, bool& changed)
{
    double mine = 0.0, flips = 0.0;
    for (int i = threadIdx.x; i < pv.n; i += 256) {
        const float4 q = pv.get(i);
        const bool in = error2(m, q.x, q.y, q.z, q.w) <= thr2;
        if (in != in_set(pv, i)) { flips += 1.0; put_set(pv, i, in); }
        if (in) mine += 1.0;
    }
    changed = block_sum(flips, red) > 0.0;
    return (int)block_sum(mine, red);            // (whole numbers below 2^24: exact in any order)
}

template <class View>
__device__ void clear_set(View pv)
{
    for (int i = threadIdx.x; i < pv.n; i += 256) put_set(pv, i, false);
}

// the summed squared forward error of m over the set
template <class View>
__device__ double set_cost(View pv, const double* m, double* red)
{
    double c = 0.0;
    for (int i = threadIdx.x; i < pv.n; i += 256) {
        if (!in_set(pv, i)) continue;
        const float4 q = pv.get(i);
        c += error2(m, q.x, q.y, q.z, q.w);
    }
    return block_sum(c, red);
}

// The least-squares model over the set of `cnt` > 0 members, the same in every thread (each finishes from the same block
// sums).  false: the set does not determine the model (coincident or collinear points).
template <class Model, class View>
__device__ bool fit_set(View pv, int cnt, double* red, double* m)
{
    double sx = 0, sy = 0, su = 0, sv = 0;
    for (int i = threadIdx.x; i < pv.n; i += 256) {
        if (!in_set(pv, i)) continue;
        const float4 q = pv.get(i);
        sx += q.x; sy += q.y; su += q.z; sv += q.w;
    }
    const double c = (double)cnt;
    const double cx = block_sum(sx, red) / c, cy = block_sum(sy, red) / c, cu = block_sum(su, red) / c, cv = block_sum(sv, red) / c;
    double acc[Model::SUMS];
    for (int k = 0; k < Model::SUMS; ++k) acc[k] = 0.0;
    for (int i = threadIdx.x; i < pv.n; i += 256) {
        if (!in_set(pv, i)) continue;
        const float4 q = pv.get(i);
        Model::add(acc, q.x - cx, q.y - cy, q.z - cu, q.w - cv);
    }
    double sum[Model::SUMS];
    for (int k = 0; k < Model::SUMS; ++k) sum[k] = block_sum(acc[k], red);
    return Model::finish(sum, c, cx, cy, cu, cv, m);
}

__device__ __forceinline__ void write_model(double* H, const double* m)
{
    for (int k = 0; k < 6; ++k) H[k] = m[k];
    H[6] = 0.0; H[7] = 0.0; H[8] = 1.0;
}

__device__ __forceinline__ void write_none(double* H, int* n_inliers, double* cost)
{
    for (int k = 0; k < 9; ++k) H[k] = 0.0;
    *n_inliers = 0;
    if (cost) { cost[0] = 0.0; cost[1] = 0.0; }
}

// One workgroup of 256 threads per pair / group: re-derive the winning hypothesis best[index], mark its consensus set in the
// view, refit by least squares over it.  With fewer than S + 1 inliers (a model that explains only its own sample is none)
// H_out[index], n_inliers[index] and the mask are zero.
template <class Model, class Source>
__global__ __launch_bounds__(256) void transform_refit_kernel(Source src, double thr, unsigned long long seed,
                                                              const unsigned long long* __restrict__ best,
                                                              double* __restrict__ H_out, int* __restrict__ n_inliers)
{
    __shared__ double red[256];
    __shared__ double msh[6];
    const int index = blockIdx.x, tid = threadIdx.x;
    const auto pv = src.view(index);
    const unsigned long long b = best[index];
    if (pv.n < Model::S + 1 || (int)(b >> 32) < Model::S + 1) {         // (the same for the whole workgroup)
        if (tid == 0) write_none(H_out + index * 9, n_inliers + index, nullptr);
        return;
    }
    if (tid == 0) {
        double m0[6];
        hypothesis<Model>(pv, seed, index, 0x7fffffff - (int)(b & 0xffffffffull), m0);
        for (int k = 0; k < 6; ++k) msh[k] = m0[k];
    }
    __syncthreads();
    double m[6];
    for (int k = 0; k < 6; ++k) m[k] = msh[k];
    bool changed;
    const int cnt = mark_inliers(pv, m, thr * thr, red, changed);
    double fit[6];
    if (cnt < Model::S + 1 || !fit_set<Model>(pv, cnt, red, fit)) {
        clear_set(pv);
        if (tid == 0) write_none(H_out + index * 9, n_inliers + index, nullptr);
        return;
    }
    if (tid == 0) { write_model(H_out + index * 9, fit); n_inliers[index] = cnt; }
}

// One workgroup of 256 threads per pair / group: local optimisation of the estimate H_io[index] (its top two rows divided by
// h22; the last row is taken as (0, 0, h22)).  At most `rounds` times: mark the inliers of the current model, refit over them;
// a round whose marking changes nothing ends it (the refit over the same set is the model already held).  A refit is kept
// only if it does not raise the cost over the set it was fitted to -- true of the exact minimiser, enforced against rounding.
// Out: the last model, the last set marked (the one that model was fitted to; with rounds = 0 the input's own) and its
// size, cost_out (may be NULL) [index][2] = the summed squared error over that set before / after the last refit.  Everything
// is zero for an input that is all zeros, not finite or has h22 = 0, and when a marked set has fewer than S + 1 members.
template <class Model, class Source>
__global__ __launch_bounds__(256) void transform_refine_kernel(Source src, double thr, int rounds, double* __restrict__ H_io,
                                                               int* __restrict__ n_inliers, double* __restrict__ cost_out)
{
    __shared__ double red[256];
    const int index = blockIdx.x, tid = threadIdx.x;
    const auto pv = src.view(index);
    double* H = H_io + index * 9;
    double* cost = cost_out ? cost_out + index * 2 : nullptr;
    double h[9];
    bool finite = true;
    for (int k = 0; k < 9; ++k) { h[k] = H[k]; finite = finite && isfinite(h[k]); }
    __syncthreads();                                     // (every thread has read H before thread 0 writes it)
    if (!finite || !(fabs(h[8]) > 0.0)) {
        if (tid == 0) write_none(H, n_inliers + index, cost);
        return;
    }
    double m[6];
    for (int k = 0; k < 6; ++k) m[k] = h[k] / h[8];
    const double thr2 = thr * thr;
    bool changed;
    int cnt = mark_inliers(pv, m, thr2, red, changed);
    double c0 = 0.0, c1 = 0.0;
    if (cnt >= Model::S + 1) c0 = c1 = set_cost(pv, m, red);
    for (int r = 0; r < rounds && cnt >= Model::S + 1; ++r) {
        if (r > 0) {
            cnt = mark_inliers(pv, m, thr2, red, changed);
            if (!changed || cnt < Model::S + 1) break;
        }
        double fit[6];
        if (!fit_set<Model>(pv, cnt, red, fit)) break;
        const double before = set_cost(pv, m, red), after = set_cost(pv, fit, red);
        if (!(after <= before)) { c0 = c1 = before; break; }
        c0 = before; c1 = after;
        for (int k = 0; k < 6; ++k) m[k] = fit[k];
    }
    if (cnt < Model::S + 1) {
        clear_set(pv);
        if (tid == 0) write_none(H, n_inliers + index, cost);
        return;
    }
    if (tid == 0) {
        write_model(H, m);
        n_inliers[index] = cnt;
        if (cost) { cost[0] = c0; cost[1] = c1; }
    }
}

}  // namespace
