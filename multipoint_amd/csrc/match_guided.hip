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

// what nn_rows_kernel (mp_match.h) builds the gate from
struct RadiusGateArgs {
    const float* pos;
    float r2;
    __device__ __forceinline__ RadiusGate gate(int dir, int p, int K, int row) const
    {
        const float2* xpos = reinterpret_cast<const float2*>(pos) + ((long long)dir * gridDim.y + p) * K;
        const float2* ypos = reinterpret_cast<const float2*>(pos) + ((long long)(dir ^ 1) * gridDim.y + p) * K;
        return RadiusGate{ypos, xpos[row], r2, dir == 0, {}};
    }
};

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
        hipLaunchKernelGGL((nn_rows_kernel<decltype(d)::value, RadiusGateArgs>), dim3((K + 127) / 128, P, 2 * MATCH_SHARES),
                           dim3(256), 0, s, dA, nA, dB, nB, pair_stride, count_stride, K, rowbest, colbest, match_count,
                           MATCH_SHARES, RadiusGateArgs{pos, radius * radius});
    });
    launch_match_mutual_rows(rowbest, colbest, nA, nB, count_stride, P, K, thr, match_idx, match_dist, match_count, s);
}
