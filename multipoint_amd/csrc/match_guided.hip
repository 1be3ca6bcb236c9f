// Guided matching of P pairs: mutual nearest neighbours INSIDE a geometric gate.  With a first estimate H_p of the pair's
// homography, optical keypoint i and thermal keypoint j are candidates for each other only if H_p maps i within `radius`
// pixels of j; among the candidates the rule is the one of mp_match_mutual_nn (match_mfma.hip), on the same fp32 MFMA
// distance tiles and the same walk (mp_match.h: walk_tiles), whose gate policy the predicate enters through:
//     wa_i       = H_p (x_i, y_i, 1) in double, divided by its third component, rounded once to fp32
//                  (no candidates at all: third component 0, or a result that is not finite)
//     gate(i, j) = (wa_i.x - x_j)^2 + (wa_i.y - y_j)^2 <= radius^2 in fp32
//     i ~ j  iff  j = argmin d(i, .) over {j : gate(i, j)}  and  i = argmin d(., j) over {i : gate(i, j)}  [and d < threshold]
// Both directions must decide gate(i, j) from the same bits, or the mutual test would compare arg-mins over different
// candidate sets: positions_kernel writes wa and the thermal positions as fp32 ONCE, the A->B pass holds its row's wa_i in
// registers and reads the tile's 32 thermal positions from LDS, the B->A pass holds b_j and reads the tile's wa, and both
// call in_gate() with the operands in the same order.  A pair whose H_p is all zeros (mp_find_homography's "no estimate")
// has third component 0 in every row: no matches.
#include "mp_match.h"

namespace {

// pos [2][P][K][2] fp32 (x, y): plane 0 = wa (the optical keypoints under H_p; NaN = no candidates), plane 1 = the thermal
// keypoints.  Row r of pair p of either side lies at kp + (p * kp_stride + r) * 2 ints (y, x).
__global__ __launch_bounds__(256) void positions_kernel(const int* __restrict__ kpA, const int* __restrict__ kpB,
                                                       long long kp_stride, int K, const double* __restrict__ hom,
                                                       float* __restrict__ pos)
{
    const int p = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= K) return;
    const double* h = hom + (long long)p * 9;
    const long long at = ((long long)p * kp_stride + i) * 2;
    const double x = kpA[at + 1], y = kpA[at];
    const double w = h[6] * x + h[7] * y + h[8];
    float2 wa = {__builtin_nanf(""), __builtin_nanf("")};
    if (w != 0.0) {
        const float u = (float)((h[0] * x + h[1] * y + h[2]) / w), v = (float)((h[3] * x + h[4] * y + h[5]) / w);
        if (isfinite(u) && isfinite(v)) wa = {u, v};
    }
    float2* out = reinterpret_cast<float2*>(pos);
    out[(long long)p * K + i] = wa;
    out[((long long)gridDim.y + p) * K + i] = {(float)kpB[at + 1], (float)kpB[at]};
}

// THE gate: wa = a warped optical position, b = a thermal position.  (Written with the rounding intrinsics so that no
// instantiation contracts the sum into an fma that the other one does not; a NaN wa fails the comparison.)
__device__ __forceinline__ bool in_gate(float2 wa, float2 b, float r2)
{
    const float dx = __fsub_rn(wa.x, b.x), dy = __fsub_rn(wa.y, b.y);
    return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)) <= r2;
}

// The walk's gate policy (mp_match.h: NoGate).  The positions of a tile's 32 Y rows are staged by the workgroup's first 32
// threads next to the tile, through the same double buffer and barriers.
struct RadiusGate {
    const float2* ypos;      // positions of the pair's Y rows
    float2 mine;             // ... of the lane's X row
    float r2;
    bool y_is_thermal;       // A -> B pass: mine = wa_i, the tile holds b_j; B -> A pass: the other way round
    float2 staged;
    __device__ __forceinline__ float2 (*tile() const)[32]
    {
        __shared__ float2 ptile[2][32];
        return ptile;
    }
    __device__ __forceinline__ void fetch(int c0, int ny)
    {
        if (threadIdx.x < 32) staged = ypos[min(c0 + (int)threadIdx.x, ny - 1)];
    }
    __device__ __forceinline__ void stash(int buf)
    {
        if (threadIdx.x < 32) tile()[buf][threadIdx.x] = staged;
    }
    __device__ __forceinline__ bool pass(int buf, int slot) const
    {
        const float2 t = tile()[buf][slot];
        return in_gate(y_is_thermal ? mine : t, y_is_thermal ? t : mine, r2);
    }
};

// nn_rows_kernel (match_mfma.hip) behind the gate: best[x] = min over the GATED y of (dist(x, y) bits << 32 | y), NO_KEY for a
// row without candidates.  grid: (row-block groups, pairs, 2 directions x column shares)
template <int D>
__global__ __launch_bounds__(256) void guided_rows_kernel(const float* __restrict__ dA, const int* __restrict__ nA,
                                                         const float* __restrict__ dB, const int* __restrict__ nB,
                                                         long long pair_stride, int count_stride, int K,
                                                         const float* __restrict__ pos, float r2,
                                                         unsigned long long* __restrict__ bestA,
                                                         unsigned long long* __restrict__ bestB, int* __restrict__ match_count,
                                                         int nsplit)
{
    // (the pair's match counter, which guided_mutual_kernel adds to behind this launch, is zeroed here)
    if (blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x == 0) match_count[blockIdx.y] = 0;
    const int p = blockIdx.y, dir = blockIdx.z & 1, share = blockIdx.z >> 1;
    const float* X = (dir == 0 ? dA : dB) + (long long)p * pair_stride;
    const float* Y = (dir == 0 ? dB : dA) + (long long)p * pair_stride;
    const int nx = min((dir == 0 ? nA : nB)[p * count_stride], K);
    const int ny = min((dir == 0 ? nB : nA)[p * count_stride], K);
    const float2* xpos = reinterpret_cast<const float2*>(pos) + ((long long)dir * gridDim.y + p) * K;
    const float2* ypos = reinterpret_cast<const float2*>(pos) + ((long long)(dir ^ 1) * gridDim.y + p) * K;
    unsigned long long* best = (dir == 0 ? bestA : bestB) + ((long long)share * gridDim.y + p) * K;
    const ColumnShare cs = column_share(ny, share, nsplit);
    if ((int)blockIdx.x * 128 >= nx) return;             // (the whole workgroup)
    const int lane = threadIdx.x & 63, li = lane & 31, half = lane >> 5;
    const int r0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    KeepNearest keep;
    RadiusGate gate{ypos, xpos[min(r0 + li, nx - 1)], r2, dir == 0, {}};
    if (!walk_tiles<D>(X, Y, nx, ny, cs.c_begin, cs.c_end, r0, li, half, keep, gate)) return;
    // the two half-waves hold the two halves of the row's columns
    const unsigned long long o = __shfl_xor(keep.run, 32);
    const int row = r0 + li;
    if (half == 0 && row < nx) best[row] = o < keep.run ? o : keep.run;
}

// mutual_kernel (match_mfma.hip) where a row or a column may have no candidate
__global__ __launch_bounds__(256) void guided_mutual_kernel(const unsigned long long* __restrict__ bestA,
                                                           const unsigned long long* __restrict__ bestB,
                                                           const int* __restrict__ nA, const int* __restrict__ nB,
                                                           int count_stride, int K, float thr,
                                                           int* __restrict__ match_idx, float* __restrict__ match_dist,
                                                           int* __restrict__ match_count, int nsplit)
{
    const int na = min(nA[blockIdx.y * count_stride], K), nb = min(nB[blockIdx.y * count_stride], K);
    write_matches(K, match_idx, match_dist, match_count, nullptr, nullptr, [&](int p, int i) {
        RowMatch m;
        if (i < na && nb > 0) {
            unsigned long long v, w, unused;
            merge_shares<1>(bestA, (long long)p * K + i, K, nsplit, v, unused);
            if (v != NO_KEY) {
                const int jj = (int)(v & 0xffffffffu);
                m.d = __uint_as_float((unsigned)(v >> 32));
                merge_shares<1>(bestB, (long long)p * K + jj, K, nsplit, w, unused);
                const bool mutual = (int)(w & 0xffffffffu) == i;      // (i is in j's gate, so w is a key)
                const bool close = (thr < 0.f) || (m.d < thr);
                if (mutual && close) m.j = jj;
            }
        }
        return m;
    });
}

}  // namespace

// rowbest/colbest: [MATCH_SHARES][P][K] packed each, pos: [2][P][K][2] floats; match_count is zeroed by the row launch
void launch_match_guided(const float* dA, const int* nA, const float* dB, const int* nB, long long pair_stride,
                         int count_stride, int P, int K, int D, const int* kpA_yx, const int* kpB_yx, const double* hom,
                         float radius, float thr, float* pos, unsigned long long* rowbest, unsigned long long* colbest,
                         int* match_idx, float* match_dist, int* match_count, hipStream_t s)
{
    if (P <= 0 || K <= 0) return;
    hipLaunchKernelGGL(positions_kernel, dim3((K + 255) / 256, P), dim3(256), 0, s, kpA_yx, kpB_yx, pair_stride / D, K, hom,
                       pos);
    for_width(D, [&](auto d) {
        hipLaunchKernelGGL(guided_rows_kernel<decltype(d)::value>, dim3((K + 127) / 128, P, 2 * MATCH_SHARES), dim3(256), 0,
                           s, dA, nA, dB, nB, pair_stride, count_stride, K, pos, radius * radius, rowbest, colbest,
                           match_count, MATCH_SHARES);
    });
    hipLaunchKernelGGL(guided_mutual_kernel, dim3((K + 255) / 256, P), dim3(256), 0, s, rowbest, colbest, nA, nB,
                       count_stride, K, thr, match_idx, match_dist, match_count, MATCH_SHARES);
}
