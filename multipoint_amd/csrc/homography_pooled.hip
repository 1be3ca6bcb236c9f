// One homography per GROUP of pairs from their pooled matches (mp_pool_matches, mp_find_homography_pooled,
// mp_refine_homography_pooled): the estimator for a rig whose optical -> thermal transform is the same for a whole recording,
// where a single cross-spectral pair has too few good matches and many pairs together have thousands.
// The algorithm is the one homography.hip documents, through the same device functions (mp_homography.h), with the group
// index in the place of the pair index: counter-based sampling sample4(seed, g, t, n_g), exact 4-point solve, forward
// reprojection test, most inliers wins (lowest hypothesis index on ties), normalised-DLT refit, Levenberg-Marquardt polish.
// What differs is where the correspondences live.  The per-pair kernels keep a pair's list in LDS (at most 3200); here the
// lists of all pairs are compacted once into global memory,
//   pts [N][4] fp32 (x, y, u, v), pair-major, query order inside a pair (the order homography.hip's gather produces),
// and a group is a contiguous range of it (group_offsets [G + 1]).  Scoring, the only step whose cost grows as T x N, runs
// on a grid of hypothesis blocks x point splits x groups: a thread owns one hypothesis (its 9 coefficients in registers), the
// group's points pass through LDS in chunks of POOL_CHUNK that every lane reads at the same address (a broadcast), and the
// splits' partial counts are added with integer atomics -- order-independent, so every run gives the same bits.
#include "mp_common.h"
#include "mp_device.h"
#include "mp_homography.h"

namespace {

constexpr int POOL_CHUNK = MP_POOLED_CHUNK;            // points per staged chunk: 16 KB of LDS
constexpr int POOL_MAX_SPLITS = MP_POOLED_MAX_SPLITS;  // most blocks that share the points of one (hypothesis block, group)

// a pair's number of usable matches: j = match_idx[p][i] with 0 <= j < nt, for i < no (as gather drops them)
__global__ __launch_bounds__(256) void pool_count_kernel(const int* __restrict__ kp_count, const int* __restrict__ match_idx, int K,
                                                         int* __restrict__ pair_cnt)
{
    __shared__ int wave_cnt[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int no = min(kp_count[2 * p], K), nt = min(kp_count[2 * p + 1], K);
    int c = 0;
    for (int i = tid; i < no; i += 256) {
        const int j = match_idx[(size_t)p * K + i];
        c += (j >= 0 && j < nt) ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((tid & 63) == 0) wave_cnt[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) pair_cnt[p] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// one workgroup: pair_offsets = exclusive prefix sum of pair_cnt (pair_offsets[P] = N), then group_offsets[g] = the offset of
// the first pair whose group id is >= g (ids non-decreasing: a binary search; groups == NULL: one group)
__global__ __launch_bounds__(256) void pool_scan_kernel(const int* __restrict__ pair_cnt, const int* __restrict__ groups, int P, int G,
                                                        int* __restrict__ pair_offsets, int* __restrict__ group_offsets)
{
    __shared__ int sh[256];
    __shared__ int carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int p0 = 0; p0 < P; p0 += 256) {
        const int p = p0 + tid;
        const int c = p < P ? pair_cnt[p] : 0;
        sh[tid] = c;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int v = tid >= off ? sh[tid - off] : 0;
            __syncthreads();
            sh[tid] += v;
            __syncthreads();
        }
        if (p < P) pair_offsets[p] = carry + sh[tid] - c;
        __syncthreads();
        if (tid == 255) carry += sh[255];
        __syncthreads();
    }
    if (tid == 0) pair_offsets[P] = carry;
    __syncthreads();                       // (the offsets above are read below by other threads of this workgroup)
    const int total = carry;
    for (int g = tid; g <= G; g += 256) {
        int first = P;                     // first pair with groups[pair] >= g
        if (!groups) first = g == 0 ? 0 : P;
        else {
            int lo = 0, hi = P;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (groups[mid] >= g) hi = mid; else lo = mid + 1;
            }
            first = lo;
        }
        group_offsets[g] = first < P ? pair_offsets[first] : total;
    }
}

// one workgroup per pair: its usable matches in query order to pts / query_index from row pair_offsets[p] on (the ordered
// compaction of homography.hip's gather: ballot + prefix, no atomics).  Rows at or beyond `capacity` are not written.
__global__ __launch_bounds__(256) void pool_write_kernel(const int* __restrict__ kp_yx, const int* __restrict__ kp_count,
                                                         const int* __restrict__ match_idx, int K,
                                                         const int* __restrict__ pair_offsets, long long capacity,
                                                         float4* __restrict__ pts, int* __restrict__ query_index)
{
    __shared__ int run_s;
    __shared__ int wave_base[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) run_s = 0;
    __syncthreads();
    const int no = min(kp_count[2 * p], K), nt = min(kp_count[2 * p + 1], K);
    const long long base = pair_offsets[p];
    for (int i0 = 0; i0 < no; i0 += 256) {
        const int i = i0 + tid;
        int j = -1;
        if (i < no) { j = match_idx[(size_t)p * K + i]; if (j >= nt) j = -1; }
        const unsigned long long bal = __ballot(j >= 0);
        const int wv = tid >> 6, ln = tid & 63;
        if (ln == 0) wave_base[wv] = __popcll(bal);
        __syncthreads();
        if (tid == 0) {
            int run = run_s;
            for (int w = 0; w < 4; ++w) { const int c = wave_base[w]; wave_base[w] = run; run += c; }
            run_s = run;
        }
        __syncthreads();
        if (j >= 0) {
            const long long pos = base + wave_base[wv] + __popcll(bal & ((1ull << ln) - 1ull));
            if (pos < capacity) {
                const int* o = kp_yx + ((size_t)(2 * p) * K + i) * 2;
                const int* t = kp_yx + ((size_t)(2 * p + 1) * K + j) * 2;
                pts[pos] = make_float4((float)o[1], (float)o[0], (float)t[1], (float)t[0]);
                query_index[pos] = i;
            }
        }
        __syncthreads();
    }
}

// the rows [start, start + n) of group g, clamped to [0, N] (the offsets are device data: nothing they hold may lead outside pts)
__device__ __forceinline__ int group_range(const int* group_offsets, int g, int N, int& start)
{
    const int a = min(max(group_offsets[g], 0), N), b = min(max(group_offsets[g + 1], 0), N);
    start = a;
    return max(b - a, 0);
}

// hypothesis t of group g from the group's points in global memory; false if the 4-point system is singular
__device__ __forceinline__ bool hypothesis(const float4* pts, int n, unsigned long long seed, int g, int t, double* h)
{
    int idx[4];
    sample4(seed, g, t, n, idx);
    double x[4], y[4], u[4], v[4];
    for (int k = 0; k < 4; ++k) { const float4 q = pts[idx[k]]; x[k] = q.x; y[k] = q.y; u[k] = q.z; v[k] = q.w; }
    return solve4(x, y, u, v, h);
}

// grid (hypothesis blocks, point splits, groups).  Block (bx, s, g) scores hypotheses bx * 256 .. + 255 of group g on the
// chunks s, s + splits, ... of its points and adds the counts to counts[g][t].  A thread without a hypothesis (t >= T, or a
// singular sample) still takes part in every staging barrier: the only early exits are the same for the whole workgroup.
__global__ __launch_bounds__(256) void pooled_score_kernel(const float4* __restrict__ pts, const int* __restrict__ group_offsets,
                                                           int N, int T, double thr, unsigned long long seed,
                                                           unsigned int* __restrict__ counts)
{
    __shared__ float4 chunk[POOL_CHUNK];
    const int g = blockIdx.z, tid = threadIdx.x;
    int start;
    const int n = group_range(group_offsets, g, N, start);
    if (n < 4) return;                                       // (sample4 needs 4 points; the whole workgroup leaves)
    const int nchunks = (n + POOL_CHUNK - 1) / POOL_CHUNK;
    if ((int)blockIdx.y >= nchunks) return;                  // (no chunk for this split; the whole workgroup leaves)
    pts += start;
    const int t = blockIdx.x * 256 + tid;
    double h[9];
    bool ok = t < T;
    if (ok) ok = hypothesis(pts, n, seed, g, t, h);
    const double thr2 = thr * thr;
    int cnt = 0;
    for (int c = blockIdx.y; c < nchunks; c += gridDim.y) {
        const int base = c * POOL_CHUNK, m = min(POOL_CHUNK, n - base);
        __syncthreads();                                     // the previous chunk has been read by every thread
        for (int i = tid; i < m; i += 256) chunk[i] = pts[base + i];
        __syncthreads();
        if (ok)
            for (int i = 0; i < m; ++i) {
                const float4 q = chunk[i];
                cnt += inlier(h, q.x, q.y, q.z, q.w, thr2);
            }
    }
    if (ok && cnt > 0) atomicAdd(&counts[(size_t)g * T + t], (unsigned int)cnt);
}

// best[g] = max over t of (count << 32) | (0x7fffffff - t): most inliers, then the LOWEST hypothesis index
__global__ __launch_bounds__(256) void pooled_select_kernel(const unsigned int* __restrict__ counts, int T,
                                                            unsigned long long* __restrict__ best)
{
    __shared__ unsigned long long wave_best[4];
    const int g = blockIdx.x, tid = threadIdx.x;
    unsigned long long b = 0;
    for (int t = tid; t < T; t += 256) {
        const unsigned long long key = ((unsigned long long)counts[(size_t)g * T + t] << 32) | (unsigned long long)(0x7fffffff - t);
        b = key > b ? key : b;
    }
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(b, off); b = o > b ? o : b; }
    if ((tid & 63) == 0) wave_best[tid >> 6] = b;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) b = wave_best[w] > b ? wave_best[w] : b;
        best[g] = b;
    }
}

// one workgroup per group: re-derive the winning hypothesis, mark its inliers in mask, refit by normalised DLT over them.
// The per-thread stride (i = tid, tid + 256, ...) and the order of the reductions are refit_kernel's (homography.hip); the
// points are read from global memory and an outlier is known by its mask byte, which this thread wrote itself.
__global__ __launch_bounds__(256) void pooled_refit_kernel(const float4* __restrict__ pts, const int* __restrict__ group_offsets,
                                                           int N, double thr, unsigned long long seed,
                                                           const unsigned long long* __restrict__ best, double* __restrict__ H_out,
                                                           unsigned char* __restrict__ mask, int* __restrict__ n_inliers)
{
    __shared__ double red[256];
    __shared__ double hsh[9];
    __shared__ double ata[81];
    const int g = blockIdx.x, tid = threadIdx.x;
    int start;
    const int n = group_range(group_offsets, g, N, start);
    const unsigned long long b = best[g];
    const int cnt = (int)(b >> 32);
    if (n < 4 || cnt < 4) {
        if (tid == 0) { n_inliers[g] = 0; for (int k = 0; k < 9; ++k) H_out[g * 9 + k] = 0.0; }
        return;
    }
    pts += start; mask += start;
    if (tid == 0) {
        double h[9];
        hypothesis(pts, n, seed, g, 0x7fffffff - (int)(b & 0xffffffffull), h);
        for (int k = 0; k < 9; ++k) hsh[k] = h[k];
    }
    __syncthreads();
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
    // inlier flags of the best hypothesis + normalisation statistics (centroid, mean distance) of both point sets
    double sx = 0, sy = 0, su = 0, sv = 0, sc = 0;
    for (int i = tid; i < n; i += 256) {
        const float4 q = pts[i];
        const bool in = inlier(h, q.x, q.y, q.z, q.w, thr2);
        mask[i] = in ? 1 : 0;
        if (in) { sx += q.x; sy += q.y; su += q.z; sv += q.w; sc += 1.0; }
    }
    const double m = block_sum(sc);
    const double cx = block_sum(sx) / m, cy = block_sum(sy) / m, cu = block_sum(su) / m, cv = block_sum(sv) / m;
    double d1 = 0, d2 = 0;
    for (int i = tid; i < n; i += 256) {
        if (!mask[i]) continue;
        const float4 q = pts[i];
        d1 += sqrt((q.x - cx) * (q.x - cx) + (q.y - cy) * (q.y - cy));
        d2 += sqrt((q.z - cu) * (q.z - cu) + (q.w - cv) * (q.w - cv));
    }
    const double md1 = block_sum(d1) / m, md2 = block_sum(d2) / m;
    const double s1 = md1 > 1e-12 ? 1.4142135623730951 / md1 : 1.0, s2 = md2 > 1e-12 ? 1.4142135623730951 / md2 : 1.0;
    // A^T A of the 2m x 9 DLT matrix on the normalised points
    double acc9[45];
    for (int k = 0; k < 45; ++k) acc9[k] = 0.0;
    for (int i = tid; i < n; i += 256) {
        if (!mask[i]) continue;
        const float4 q = pts[i];
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
                const double s = block_sum(acc9[k]);
                if (tid == 0) { ata[a * 9 + c] = s; ata[c * 9 + a] = s; }
            }
    }
    __syncthreads();
    if (tid == 0) {
        dlt_finish(ata, cx, cy, cu, cv, s1, s2, H_out + g * 9);
        n_inliers[g] = (int)m;
    }
}

// lm_sums of homography.hip on a group's points in global memory: the inliers are the rows whose mask byte is set
__device__ void lm_sums_pooled(const float4* pts, const unsigned char* mask, int n, const double* h, double* wave_part, double* out)
{
    const int tid = threadIdx.x;
    double acc[LM_SUMS];
#pragma unroll
    for (int k = 0; k < LM_SUMS; ++k) acc[k] = 0.0;
    for (int i = tid; i < n; i += 256) {
        if (!mask[i]) continue;
        const float4 q = pts[i];
        lm_add_point(acc, h, q.x, q.y, q.z, q.w);
    }
    lm_reduce(acc, wave_part, out);
}

// one workgroup per group: refine_kernel (homography.hip) on the group's points.  A thread reads only mask bytes it wrote.
__global__ __launch_bounds__(256) void pooled_refine_kernel(const float4* __restrict__ pts, const int* __restrict__ group_offsets,
                                                            int N, double thr, int iters, double* __restrict__ H_io,
                                                            unsigned char* __restrict__ mask, int* __restrict__ n_inliers,
                                                            double* __restrict__ cost_out)
{
    __shared__ double wave_part[4 * LM_SUMS];
    __shared__ double cur[LM_SUMS], cand[LM_SUMS];     // the sums at the accepted parameters / at the step being tried
    __shared__ double hcur[8], htry[8];
    __shared__ int count_s[4], state;                  // state: 0 = the trial's system was singular, 1 = evaluate htry
    const int g = blockIdx.x, tid = threadIdx.x;
    int start;
    const int n = group_range(group_offsets, g, N, start);
    pts += start; mask += start;
    double h[9];
    for (int k = 0; k < 9; ++k) h[k] = H_io[g * 9 + k];
    // the inliers of the INPUT estimate (an all-zero matrix has none: inlier() refuses w = 0)
    const double thr2 = thr * thr;
    int mine = 0;
    for (int i = tid; i < n; i += 256) {
        const float4 q = pts[i];
        const bool in = inlier(h, q.x, q.y, q.z, q.w, thr2);
        mask[i] = in ? 1 : 0;
        if (in) ++mine;
    }
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if ((tid & 63) == 0) count_s[tid >> 6] = mine;
    __syncthreads();
    const int m = count_s[0] + count_s[1] + count_s[2] + count_s[3];
    if (m < 4 || !(fabs(h[8]) > 0.0) || !isfinite(h[8])) {
        if (tid == 0) {
            n_inliers[g] = m;
            for (int k = 0; k < 9; ++k) H_io[g * 9 + k] = 0.0;
            if (cost_out) { cost_out[g * 2] = 0.0; cost_out[g * 2 + 1] = 0.0; }
        }
        return;
    }
    if (tid < 8) hcur[tid] = h[tid] / h[8];
    __syncthreads();
    lm_sums_pooled(pts, mask, n, hcur, wave_part, cur);
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
            if (ok) lm_sums_pooled(pts, mask, n, htry, wave_part, cand);
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
        n_inliers[g] = m;
        for (int k = 0; k < 8; ++k) H_io[g * 9 + k] = hcur[k];
        H_io[g * 9 + 8] = 1.0;
        if (cost_out) { cost_out[g * 2] = cost0; cost_out[g * 2 + 1] = cur[44]; }
    }
}

}  // namespace

void launch_pool_matches(const int* kp_yx, const int* kp_count, const int* match_idx, const int* groups, int P, int K, int G,
                         float* pts, int* query_index, long long capacity, int* pair_offsets, int* group_offsets, int* pair_cnt,
                         hipStream_t s)
{
    hipLaunchKernelGGL(pool_count_kernel, dim3(P), dim3(256), 0, s, kp_count, match_idx, K, pair_cnt);
    hipLaunchKernelGGL(pool_scan_kernel, dim3(1), dim3(256), 0, s, pair_cnt, groups, P, G, pair_offsets, group_offsets);
    hipLaunchKernelGGL(pool_write_kernel, dim3(P), dim3(256), 0, s, kp_yx, kp_count, match_idx, K, pair_offsets, capacity,
                       reinterpret_cast<float4*>(pts), query_index);
}

void launch_find_homography_pooled(const float* pts, const int* group_offsets, int N, int G, int T, double thr,
                                   unsigned long long seed, unsigned int* counts, unsigned long long* best, double* H_out,
                                   unsigned char* mask, int* n_inliers, hipStream_t s)
{
    const float4* p4 = reinterpret_cast<const float4*>(pts);
    const int splits = min(max((N + POOL_CHUNK - 1) / POOL_CHUNK, 1), POOL_MAX_SPLITS);
    hipLaunchKernelGGL(pooled_score_kernel, dim3((T + 255) / 256, splits, G), dim3(256), 0, s, p4, group_offsets, N, T, thr, seed,
                       counts);
    hipLaunchKernelGGL(pooled_select_kernel, dim3(G), dim3(256), 0, s, counts, T, best);
    hipLaunchKernelGGL(pooled_refit_kernel, dim3(G), dim3(256), 0, s, p4, group_offsets, N, thr, seed, best, H_out, mask, n_inliers);
}

void launch_refine_homography_pooled(const float* pts, const int* group_offsets, int N, int G, double thr, int iters, double* H_io,
                                     unsigned char* mask, int* n_inliers, double* cost, hipStream_t s)
{
    hipLaunchKernelGGL(pooled_refine_kernel, dim3(G), dim3(256), 0, s, reinterpret_cast<const float4*>(pts), group_offsets, N, thr,
                       iters, H_io, mask, n_inliers, cost);
}
