// The model-free half of the RANSAC estimators, written once for the homography (mp_homography.h) and the similarity / affine
// models (mp_transform.h) on both routes -- one model per pair (homography.hip, transform.hip) and one per group of pairs
// (homography_pooled.hip, transform_pooled.hip): the ordered compaction of a pair's usable matches, the point views and their
// sources, counter-based sampling, the fixed-order block sum and the two scoring kernels.
// One body, two views.  hypothesis and the refit / refine kernels of the model headers are templates on where the
// correspondences live and how an outlier is marked: PairView (a pair's list in LDS) or PooledView (a group's rows in global
// memory).  A kernel gets its view from a Source, the struct of launch arguments that locates the points of pair / group `index`
// (PairSource gathers them into LDS, PooledSource looks up the group's range).
// A Model (Homography, Similarity, Affine) tells the scoring kernels what differs between them:
//   S        the minimal sample          COEFFS   the coefficients a thread carries (9 / 6)
//   minimal(x, y, u, v, m)   the exact model through S correspondences; false if they are degenerate
//   inlier(m, x, y, u, v, thr2)   the forward error test
#pragma once
#include "mp_common.h"
#include "mp_device.h"

namespace {

// ---- a pair's usable matches ----
// the partner j = match_idx[p][i] of query i if the match is usable (i < no, 0 <= j < nt), else -1
__device__ __forceinline__ int usable_match(const int* match_idx, int p, int K, int i, int no, int nt)
{
    if (i >= no) return -1;
    const int j = match_idx[(size_t)p * K + i];
    return (j >= 0 && j < nt) ? j : -1;
}

// the correspondence (x, y) -> (u, v) of query i and partner j of pair p (kp_yx: [2P][K] (y, x), slot 2p optical, 2p + 1 thermal)
// KP: int (pixel keypoints) or float (sub-pixel ones, mp_refine_keypoints): everything behind this cast is one body
template <class KP>
__device__ __forceinline__ float4 match_point(const KP* kp_yx, int p, int K, int i, int j)
{
    const KP* o = kp_yx + ((size_t)(2 * p) * K + i) * 2;
    const KP* t = kp_yx + ((size_t)(2 * p + 1) * K + j) * 2;
    return make_float4((float)o[1], (float)o[0], (float)t[1], (float)t[0]);
}

// Ordered compaction of pair p's usable matches by a workgroup of 256 threads (all of them call it): the queries are walked in
// steps of 256, a survivor's position comes from the wave's ballot and the prefix of the four waves' counts -- query order, as
// the reference's list comprehension keeps it, and no atomics.  put(pos, i, j) is called once per usable match; returns their
// number.
template <class Put>
__device__ int compact_matches(const int* kp_count, const int* match_idx, int p, int K, Put put)
{
    __shared__ int run_s;
    __shared__ int wave_base[4];
    const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
    if (tid == 0) run_s = 0;
    __syncthreads();
    const int no = min(kp_count[2 * p], K), nt = min(kp_count[2 * p + 1], K);
    for (int i0 = 0; i0 < no; i0 += 256) {
        const int i = i0 + tid;
        const int j = usable_match(match_idx, p, K, i, no, nt);
        const unsigned long long bal = __ballot(j >= 0);
        if (ln == 0) wave_base[wv] = __popcll(bal);
        __syncthreads();
        if (tid == 0) {
            int run = run_s;
            for (int w = 0; w < 4; ++w) { const int c = wave_base[w]; wave_base[w] = run; run += c; }
            run_s = run;
        }
        __syncthreads();
        if (j >= 0) put(wave_base[wv] + __popcll(bal & ((1ull << ln) - 1ull)), i, j);
        __syncthreads();
    }
    return run_s;
}

// ---- the two point views ----
// a pair's list in LDS: pts [n][4] floats (x, y, u, v), qidx [n] the query index of each match, mask_row the pair's row of the
// mask (one byte per optical keypoint).  An outlier is marked by a NaN x.
struct PairView {
    float* pts;
    const int* qidx;
    unsigned char* mask_row;
    int n;
    __device__ float4 get(int i) const { return make_float4(pts[i * 4], pts[i * 4 + 1], pts[i * 4 + 2], pts[i * 4 + 3]); }
    __device__ bool is_inlier(int i) const { return pts[i * 4] == pts[i * 4]; }
    __device__ void set_inlier(int i, bool in) const
    {
        mask_row[qidx[i]] = in ? 1 : 0;
        if (!in) pts[i * 4] = __int_as_float(0x7fc00000);
    }
};

// a group's rows in global memory, pts and mask advanced by the group's start.  An outlier is known by its mask byte; a thread
// reads only bytes it wrote itself (the bodies walk i = tid, tid + 256, ... in every pass).
struct PooledView {
    const float4* pts;
    unsigned char* mask;
    int n;
    __device__ float4 get(int i) const { return pts[i]; }
    __device__ bool is_inlier(int i) const { return mask[i] != 0; }
    __device__ void set_inlier(int i, bool in) const { mask[i] = in ? 1 : 0; }
};

// ---- the two sources: what locates the view of pair / group `index` ----
// gather the matched (x,y)->(u,v) pairs of pair p into LDS in query order; returns their number
// pts: [n][4] floats in LDS order x, y, u, v; qidx (may be NULL): [n] the query index of each match
template <class KP>
__device__ int gather(const KP* kp_yx, const int* kp_count, const int* match_idx, int p, int K, float* pts, int* qidx)
{
    return compact_matches(kp_count, match_idx, p, K, [&](int pos, int i, int j) {
        const float4 q = match_point(kp_yx, p, K, i, j);
        pts[pos * 4 + 0] = q.x; pts[pos * 4 + 1] = q.y; pts[pos * 4 + 2] = q.z; pts[pos * 4 + 3] = q.w;
        if (qidx) qidx[pos] = i;
    });
}

// what the refit / refine kernels are launched with: the view of pair p is its gathered list in LDS
// (dynamic LDS: [K][4] floats, then [K] ints) and its row of the mask.  KP: the keypoint type (int pixels or float sub-pixel
// positions); it only decides what gather reads
template <class KP>
struct PairSource {
    const KP* kp_yx;
    const int* kp_count;
    const int* match_idx;
    int K;
    unsigned char* mask;
    __device__ PairView view(int p) const
    {
        extern __shared__ float pts[];
        int* qidx = reinterpret_cast<int*>(pts + (size_t)K * 4);
        const int n = gather(kp_yx, kp_count, match_idx, p, K, pts, qidx);
        return PairView{pts, qidx, mask + (size_t)p * K, n};
    }
};

// the rows [start, start + n) of group g, clamped to [0, N] (the offsets are device data: nothing they hold may lead outside pts)
__device__ __forceinline__ int group_range(const int* group_offsets, int g, int N, int& start)
{
    const int a = min(max(group_offsets[g], 0), N), b = min(max(group_offsets[g + 1], 0), N);
    start = a;
    return max(b - a, 0);
}

// what the refit / refine kernels are launched with: the view of group g is its range of pts and mask
struct PooledSource {
    const float4* pts;
    const int* group_offsets;
    int N;
    unsigned char* mask;
    __device__ PooledView view(int g) const
    {
        int start;
        const int n = group_range(group_offsets, g, N, start);
        return PooledView{pts + start, mask + start, n};
    }
};

// the sum of v over the 256 threads of the workgroup (a tree in LDS: the same bits on every run).  All 256 threads call it.
__device__ __forceinline__ double block_sum(double v, double* red /* [256] LDS */)
{
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    const double r = red[0];
    __syncthreads();
    return r;
}

// ---- hypotheses ----
// S distinct indices in [0, n) for hypothesis t of pair / group p.  Never terminates for n < S: callers leave before it.
template <int S>
__device__ __forceinline__ void sample_distinct(unsigned long long seed, int p, int t, int n, int* idx)
{
    unsigned long long ctr = mix64(seed ^ ((unsigned long long)p << 32) ^ (unsigned long long)t);
    for (int k = 0; k < S; ++k) {
        for (;;) {
            ctr = mix64(ctr);
            const int c = (int)(ctr % (unsigned long long)n);
            bool dup = false;
            for (int j = 0; j < k; ++j) dup |= (idx[j] == c);
            if (!dup) { idx[k] = c; break; }
        }
    }
}

// hypothesis t of pair / group `index` from S sampled points of the view; false if the sample is degenerate
template <class Model, class View>
__device__ __forceinline__ bool hypothesis(View pv, unsigned long long seed, int index, int t, double* m)
{
    int idx[Model::S];
    sample_distinct<Model::S>(seed, index, t, pv.n, idx);
    double x[Model::S], y[Model::S], u[Model::S], v[Model::S];
    for (int k = 0; k < Model::S; ++k) { const float4 q = pv.get(idx[k]); x[k] = q.x; y[k] = q.y; u[k] = q.z; v[k] = q.w; }
    return Model::minimal(x, y, u, v, m);
}

// ---- scoring, per pair ----
// grid (hypothesis blocks, pairs): one thread per hypothesis, the matches of the pair sit in LDS ([K][4] floats, dynamic); the
// winner best[p] (pre-set to 0) is picked with a 64-bit atomicMax
template <class Model, class KP>
__global__ __launch_bounds__(256) void ransac_kernel(const KP* __restrict__ kp_yx, const int* __restrict__ kp_count,
                                                     const int* __restrict__ match_idx, int K, int T, double thr,
                                                     unsigned long long seed, unsigned long long* __restrict__ best)
{
    extern __shared__ float pts[];            // [K][4]
    const int p = blockIdx.y;
    const int n = gather(kp_yx, kp_count, match_idx, p, K, pts, nullptr);
    if (n < Model::S) return;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    double m[Model::COEFFS];
    if (!hypothesis<Model>(PairView{pts, nullptr, nullptr, n}, seed, p, t, m)) return;
    const double thr2 = thr * thr;
    int cnt = 0;
    for (int i = 0; i < n; ++i) cnt += Model::inlier(m, pts[i * 4], pts[i * 4 + 1], pts[i * 4 + 2], pts[i * 4 + 3], thr2);
    // most inliers, then the LOWEST hypothesis index
    atomicMax(&best[p], ((unsigned long long)cnt << 32) | (unsigned long long)(0x7fffffff - t));
}

// ---- scoring, pooled ----
constexpr int POOL_CHUNK = MP_POOLED_CHUNK;            // points per staged chunk: 16 KB of LDS
constexpr int POOL_MAX_SPLITS = MP_POOLED_MAX_SPLITS;  // most blocks that share the points of one (hypothesis block, group)

// the point splits of a scoring launch over N pooled rows (the grid's y)
inline int pool_splits(int N) { return min(max((N + POOL_CHUNK - 1) / POOL_CHUNK, 1), POOL_MAX_SPLITS); }

// grid (hypothesis blocks, point splits, groups).  Block (bx, s, g) scores hypotheses bx * 256 .. + 255 of group g on the
// chunks s, s + splits, ... of its points and adds the counts to counts[g][t].  A thread without a hypothesis (t >= T, or a
// degenerate sample) still takes part in every staging barrier: the only early exits are the same for the whole workgroup.
template <class Model>
__global__ __launch_bounds__(256) void pooled_score_kernel(const float4* __restrict__ pts, const int* __restrict__ group_offsets,
                                                           int N, int T, double thr, unsigned long long seed,
                                                           unsigned int* __restrict__ counts)
{
    __shared__ float4 chunk[POOL_CHUNK];
    const int g = blockIdx.z, tid = threadIdx.x;
    int start;
    const int n = group_range(group_offsets, g, N, start);
    if (n < Model::S) return;                                // (the sampling needs S points; the whole workgroup leaves)
    const int nchunks = (n + POOL_CHUNK - 1) / POOL_CHUNK;
    if ((int)blockIdx.y >= nchunks) return;                  // (no chunk for this split; the whole workgroup leaves)
    pts += start;
    const int t = blockIdx.x * 256 + tid;
    double m[Model::COEFFS];
    bool ok = t < T;
    if (ok) ok = hypothesis<Model>(PooledView{pts, nullptr, n}, seed, g, t, m);
    const double thr2 = thr * thr;
    int cnt = 0;
    for (int c = blockIdx.y; c < nchunks; c += gridDim.y) {
        const int base = c * POOL_CHUNK, len = min(POOL_CHUNK, n - base);
        __syncthreads();                                     // the previous chunk has been read by every thread
        for (int i = tid; i < len; i += 256) chunk[i] = pts[base + i];
        __syncthreads();
        if (ok)
            for (int i = 0; i < len; ++i) {
                const float4 q = chunk[i];
                cnt += Model::inlier(m, q.x, q.y, q.z, q.w, thr2);
            }
    }
    if (ok && cnt > 0) atomicAdd(&counts[(size_t)g * T + t], (unsigned int)cnt);
}

}  // namespace
