// Batched RANSAC homography estimation for the matched keypoints of P pairs: the step that follows
// matching in the reference (predict_align_image_pair.py:205-216, evaluation.py:330-349:
// cv2.findHomography(optical_pts, thermal_pts, cv2.RANSAC, ransacReprojThreshold)).
// OpenCV is a third-party dependency that is absent here and its RANSAC draws from its own RNG, so this is not a
// bit-level restatement ("parity unpinned"); it follows the published algorithm:
//   T hypotheses per pair, each from 4 distinct random matches (counter-based RNG -> reproducible), exact 4-point
//   solve (8x8 Gaussian elimination, fp64), score = number of matches with forward reprojection error <= threshold,
//   best = most inliers (lowest hypothesis index on ties), final model = normalised DLT over the best inlier set.
// One thread per hypothesis (the matches of the pair sit in LDS); the winner is picked with a 64-bit atomicMax.
// OpenCV's last step, the Levenberg-Marquardt polish of the refitted model, is a launch of its own (refine_kernel).
#include "mp_common.h"
#include "mp_device.h"
#include "mp_homography.h"

namespace {

// gather the matched (x,y)->(u,v) pairs of pair p into LDS / a compact list; returns their number
// pts: [n][4] floats in LDS order x, y, u, v
__device__ int gather(const int* kp_yx, const int* kp_count, const int* match_idx, int p, int K, float* pts, int* qidx)
{
    __shared__ int n_s;
    if (threadIdx.x == 0) n_s = 0;
    __syncthreads();
    const int no = min(kp_count[2 * p], K), nt = min(kp_count[2 * p + 1], K);
    // ordered compaction in chunks of blockDim: keeps query order (as the reference's list comprehension does)
    for (int i0 = 0; i0 < no; i0 += blockDim.x) {
        const int i = i0 + threadIdx.x;
        int j = -1;
        if (i < no) { j = match_idx[(size_t)p * K + i]; if (j >= nt) j = -1; }
        const unsigned long long bal = __ballot(j >= 0);
        __shared__ int wave_base[16];
        const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
        if (ln == 0) wave_base[wv] = __popcll(bal);
        __syncthreads();
        if (threadIdx.x == 0) {
            int run = n_s;
            for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { const int c = wave_base[w]; wave_base[w] = run; run += c; }
            n_s = run;
        }
        __syncthreads();
        if (j >= 0) {
            const int pos = wave_base[wv] + __popcll(bal & ((1ull << ln) - 1ull));
            pts[pos * 4 + 0] = (float)kp_yx[((size_t)(2 * p) * K + i) * 2 + 1];
            pts[pos * 4 + 1] = (float)kp_yx[((size_t)(2 * p) * K + i) * 2];
            pts[pos * 4 + 2] = (float)kp_yx[((size_t)(2 * p + 1) * K + j) * 2 + 1];
            pts[pos * 4 + 3] = (float)kp_yx[((size_t)(2 * p + 1) * K + j) * 2];
            if (qidx) qidx[pos] = i;
        }
        __syncthreads();
    }
    return n_s;
}

__global__ __launch_bounds__(256) void ransac_kernel(const int* __restrict__ kp_yx, const int* __restrict__ kp_count,
                                                     const int* __restrict__ match_idx, int K, int T, double thr,
                                                     unsigned long long seed, unsigned long long* __restrict__ best)
{
    extern __shared__ float pts[];            // [K][4]
    const int p = blockIdx.y;
    const int n = gather(kp_yx, kp_count, match_idx, p, K, pts, nullptr);
    if (n < 4) return;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    int idx[4];
    sample4(seed, p, t, n, idx);
    double x[4], y[4], u[4], v[4], h[9];
    for (int k = 0; k < 4; ++k) { x[k] = pts[idx[k] * 4]; y[k] = pts[idx[k] * 4 + 1]; u[k] = pts[idx[k] * 4 + 2]; v[k] = pts[idx[k] * 4 + 3]; }
    if (!solve4(x, y, u, v, h)) return;
    const double thr2 = thr * thr;
    int cnt = 0;
    for (int i = 0; i < n; ++i) cnt += inlier(h, pts[i * 4], pts[i * 4 + 1], pts[i * 4 + 2], pts[i * 4 + 3], thr2);
    // most inliers, then the LOWEST hypothesis index
    atomicMax(&best[p], ((unsigned long long)cnt << 32) | (unsigned long long)(0x7fffffff - t));
}

// one workgroup per pair: re-derive the winning hypothesis, mark its inliers, refit by normalised DLT over them
__global__ __launch_bounds__(256) void refit_kernel(const int* __restrict__ kp_yx, const int* __restrict__ kp_count,
                                                    const int* __restrict__ match_idx, int K, double thr,
                                                    unsigned long long seed, const unsigned long long* __restrict__ best,
                                                    double* __restrict__ H_out, unsigned char* __restrict__ mask,
                                                    int* __restrict__ n_inliers)
{
    extern __shared__ float pts[];            // [K][4] floats, then [K] ints (query index of each match)
    int* qidx = reinterpret_cast<int*>(pts + (size_t)K * 4);
    __shared__ double red[256];
    __shared__ double hsh[9];
    __shared__ double stat[8];
    __shared__ double ata[81];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n = gather(kp_yx, kp_count, match_idx, p, K, pts, qidx);
    const unsigned long long b = best[p];
    const int cnt = (int)(b >> 32);
    if (n < 4 || cnt < 4) {
        if (tid == 0) { n_inliers[p] = 0; for (int k = 0; k < 9; ++k) H_out[p * 9 + k] = 0.0; }
        return;
    }
    if (tid == 0) {
        const int t = 0x7fffffff - (int)(b & 0xffffffffull);
        int idx[4];
        sample4(seed, p, t, n, idx);
        double x[4], y[4], u[4], v[4], h[9];
        for (int k = 0; k < 4; ++k) { x[k] = pts[idx[k] * 4]; y[k] = pts[idx[k] * 4 + 1]; u[k] = pts[idx[k] * 4 + 2]; v[k] = pts[idx[k] * 4 + 3]; }
        solve4(x, y, u, v, h);
        for (int k = 0; k < 9; ++k) hsh[k] = h[k];
    }
    __syncthreads();
    // inlier flags of the best hypothesis + normalisation statistics (centroid, mean distance) of both point sets
    const double thr2 = thr * thr;
    double h[9];
    for (int k = 0; k < 9; ++k) h[k] = hsh[k];
    auto block_sum = [&](double v) -> double {
        red[tid] = v;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
        const double r = red[0];
        __syncthreads();
        return r;
    };
    double sx = 0, sy = 0, su = 0, sv = 0, sc = 0;
    for (int i = tid; i < n; i += 256) {
        const bool in = inlier(h, pts[i * 4], pts[i * 4 + 1], pts[i * 4 + 2], pts[i * 4 + 3], thr2);
        mask[(size_t)p * K + qidx[i]] = in ? 1 : 0;
        if (in) { sx += pts[i * 4]; sy += pts[i * 4 + 1]; su += pts[i * 4 + 2]; sv += pts[i * 4 + 3]; sc += 1.0; }
        else pts[i * 4] = __int_as_float(0x7fc00000);          // NaN marks an outlier for the passes below
    }
    const double m = block_sum(sc);
    const double cx = block_sum(sx) / m, cy = block_sum(sy) / m, cu = block_sum(su) / m, cv = block_sum(sv) / m;
    double d1 = 0, d2 = 0;
    for (int i = tid; i < n; i += 256) {
        if (pts[i * 4] != pts[i * 4]) continue;
        d1 += sqrt((pts[i * 4] - cx) * (pts[i * 4] - cx) + (pts[i * 4 + 1] - cy) * (pts[i * 4 + 1] - cy));
        d2 += sqrt((pts[i * 4 + 2] - cu) * (pts[i * 4 + 2] - cu) + (pts[i * 4 + 3] - cv) * (pts[i * 4 + 3] - cv));
    }
    const double md1 = block_sum(d1) / m, md2 = block_sum(d2) / m;
    const double s1 = md1 > 1e-12 ? 1.4142135623730951 / md1 : 1.0, s2 = md2 > 1e-12 ? 1.4142135623730951 / md2 : 1.0;
    // A^T A of the 2m x 9 DLT matrix on the normalised points: thread (r, c) owns one entry
    for (int e = tid; e < 81; e += 256) ata[e] = 0.0;
    __syncthreads();
    double acc9[45];
    for (int k = 0; k < 45; ++k) acc9[k] = 0.0;
    for (int i = tid; i < n; i += 256) {
        if (pts[i * 4] != pts[i * 4]) continue;
        const double x = (pts[i * 4] - cx) * s1, y = (pts[i * 4 + 1] - cy) * s1;
        const double u = (pts[i * 4 + 2] - cu) * s2, v = (pts[i * 4 + 3] - cv) * s2;
        const double r0[9] = {x, y, 1.0, 0.0, 0.0, 0.0, -u * x, -u * y, -u};
        const double r1[9] = {0.0, 0.0, 0.0, x, y, 1.0, -v * x, -v * y, -v};
        int k = 0;
        for (int a = 0; a < 9; ++a) for (int c = a; c < 9; ++c, ++k) acc9[k] += r0[a] * r0[c] + r1[a] * r1[c];
    }
    {
        int k = 0;
        for (int a = 0; a < 9; ++a)
            for (int c = a; c < 9; ++c, ++k) {
                const double s = block_sum(acc9[k]);
                if (tid == 0) { ata[a * 9 + c] = s; ata[c * 9 + a] = s; }
            }
    }
    __syncthreads();
    if (tid == 0) {
        dlt_finish(ata, cx, cy, cu, cv, s1, s2, H_out + p * 9);
        n_inliers[p] = (int)m;
    }
}

// ---- the Levenberg-Marquardt polish (mp_refine_homography; the algorithm and its pieces: mp_homography.h) ----
// out[0..44] = the sums of J^T J, J^T r and r.r at parameters h over the inliers among pts[0..n) (a NaN x marks an
// outlier).  Fixed order: a thread adds its inliers i = tid, tid + 256, ..., then lm_reduce.  All 256 threads call it.
__device__ void lm_sums(const float* pts, int n, const double* h, double* wave_part /* [4][LM_SUMS] LDS */, double* out)
{
    const int tid = threadIdx.x;
    double acc[LM_SUMS];
#pragma unroll
    for (int k = 0; k < LM_SUMS; ++k) acc[k] = 0.0;
    for (int i = tid; i < n; i += 256) {
        if (pts[i * 4] != pts[i * 4]) continue;
        lm_add_point(acc, h, pts[i * 4], pts[i * 4 + 1], pts[i * 4 + 2], pts[i * 4 + 3]);
    }
    lm_reduce(acc, wave_part, out);
}

__global__ __launch_bounds__(256) void refine_kernel(const int* __restrict__ kp_yx, const int* __restrict__ kp_count,
                                                     const int* __restrict__ match_idx, int K, double thr, int iters,
                                                     double* __restrict__ H_io, unsigned char* __restrict__ mask,
                                                     int* __restrict__ n_inliers, double* __restrict__ cost_out)
{
    extern __shared__ float pts[];            // [K][4] floats, then [K] ints (query index of each match)
    int* qidx = reinterpret_cast<int*>(pts + (size_t)K * 4);
    __shared__ double wave_part[4 * LM_SUMS];
    __shared__ double cur[LM_SUMS], cand[LM_SUMS];     // the sums at the accepted parameters / at the step being tried
    __shared__ double hcur[8], htry[8];
    __shared__ int count_s[4], state;                  // state: 0 = the trial's system was singular, 1 = evaluate htry
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n = gather(kp_yx, kp_count, match_idx, p, K, pts, qidx);
    double h[9];
    for (int k = 0; k < 9; ++k) h[k] = H_io[p * 9 + k];
    // the inliers of the INPUT estimate (an all-zero matrix has none: inlier() refuses w = 0)
    const double thr2 = thr * thr;
    int mine = 0;
    for (int i = tid; i < n; i += 256) {
        const bool in = inlier(h, pts[i * 4], pts[i * 4 + 1], pts[i * 4 + 2], pts[i * 4 + 3], thr2);
        mask[(size_t)p * K + qidx[i]] = in ? 1 : 0;
        if (in) ++mine; else pts[i * 4] = __int_as_float(0x7fc00000);          // NaN marks an outlier for lm_sums
    }
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if ((tid & 63) == 0) count_s[tid >> 6] = mine;
    __syncthreads();
    const int m = count_s[0] + count_s[1] + count_s[2] + count_s[3];
    if (m < 4 || !(fabs(h[8]) > 0.0) || !isfinite(h[8])) {
        if (tid == 0) {
            n_inliers[p] = m;
            for (int k = 0; k < 9; ++k) H_io[p * 9 + k] = 0.0;
            if (cost_out) { cost_out[p * 2] = 0.0; cost_out[p * 2 + 1] = 0.0; }
        }
        return;
    }
    if (tid < 8) hcur[tid] = h[tid] / h[8];
    __syncthreads();
    lm_sums(pts, n, hcur, wave_part, cur);
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
            if (ok) lm_sums(pts, n, htry, wave_part, cand);
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
        n_inliers[p] = m;
        for (int k = 0; k < 8; ++k) H_io[p * 9 + k] = hcur[k];
        H_io[p * 9 + 8] = 1.0;
        if (cost_out) { cost_out[p * 2] = cost0; cost_out[p * 2 + 1] = cur[44]; }
    }
}

}  // namespace

void launch_ransac_homography(const int* kp_yx, const int* kp_count, const int* match_idx, int P, int K, int T, double thr,
                              unsigned long long seed, unsigned long long* best, double* H_out, unsigned char* mask,
                              int* n_inliers, hipStream_t s)
{
    const size_t lds1 = (size_t)K * 4 * sizeof(float), lds2 = lds1 + (size_t)K * sizeof(int);
    hipLaunchKernelGGL(ransac_kernel, dim3((T + 255) / 256, P), dim3(256), lds1, s, kp_yx, kp_count, match_idx, K, T, thr, seed, best);
    hipLaunchKernelGGL(refit_kernel, dim3(P), dim3(256), lds2, s, kp_yx, kp_count, match_idx, K, thr, seed, best, H_out, mask,
                       n_inliers);
}

// mask must be zeroed by the caller (only the matched optical keypoints are written)
void launch_refine_homography(const int* kp_yx, const int* kp_count, const int* match_idx, int P, int K, double thr, int iters,
                              double* H_io, unsigned char* mask, int* n_inliers, double* cost, hipStream_t s)
{
    const size_t lds = (size_t)K * 4 * sizeof(float) + (size_t)K * sizeof(int);
    hipLaunchKernelGGL(refine_kernel, dim3(P), dim3(256), lds, s, kp_yx, kp_count, match_idx, K, thr, iters, H_io, mask,
                       n_inliers, cost);
}
