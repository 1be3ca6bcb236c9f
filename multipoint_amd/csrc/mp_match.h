// The MFMA matchers' walk over the distance tiles (match_mfma.hip): packed keys, column shares, the two running states and
// the tile loop that nn_rows_kernel and near2_rows_kernel share.  Internal header.
//
// X rows against Y rows, both unit: d = sqrt(u), u = 2 - 2 clip(x.y, -1, 1).  Each wave owns one 32-row block of X; the four
// waves of a workgroup walk the same 32-column tiles of Y, which reach them through LDS: a tile is 32 x D contiguous floats,
// staged with fully coalesced 16-byte loads (one 1 KiB run per wave instruction) one tile ahead, and read back as MFMA
// fragments (padded rows: conflict free).  Fetching the fragments straight from global memory -- 16 bytes out of every
// 128-byte line of 32 lines per load instruction, each wave for itself -- kept the kernel at twice its MFMA time (131 us for
// 62 us of v_mfma_f32_32x32x2_f32).  The products are formed TRANSPOSED (Y fragment as the A operand): lane li owns X row
// r0 + li, its 16 accumulator registers are 16 columns of the tile, and the columns reach a lane in ascending order.
#pragma once
#include "mp_common.h"

#include <type_traits>

constexpr unsigned long long NO_KEY = ~0ull;             // (distance bits 0xffffffff are a NaN: never a real key)

// (distance bits << 32 | column): ordered by distance, equal distances by the lower column
__device__ __forceinline__ unsigned long long match_key(float u, int col)
{
    return ((unsigned long long)__float_as_uint(sqrtf(u)) << 32) | (unsigned)col;
}

// the two smallest of the union of two ascending key pairs
__device__ __forceinline__ void merge2(unsigned long long& k1, unsigned long long& k2, unsigned long long o1,
                                       unsigned long long o2)
{
    const unsigned long long lo = k1 < o1 ? k1 : o1, hi = k1 < o1 ? o1 : k1, s = k2 < o2 ? k2 : o2;
    k1 = lo;
    k2 = hi < s ? hi : s;
}

// The Y columns are cut into `nsplit` contiguous shares of whole tiles, each share leaves its own array of keys (the epilogue
// kernels merge them) -- twice the waves per SIMD for the same work: the epilogue of one wave has another wave's MFMAs to
// hide behind.
struct ColumnShare { int c_begin, c_end; };
__device__ __forceinline__ ColumnShare column_share(int ny, int share, int nsplit)
{
    const int ntile = (ny + 31) >> 5, per = (ntile + nsplit - 1) / nsplit;
    return {min(share * per, ntile) * 32, min(min((share + 1) * per, ntile) * 32, ny)};
}

// ONE running arg-min per lane, over columns that arrive in ascending order, so a later column replaces the best one only
// with a strictly smaller distance.  d = sqrt(u) is monotone in u: "u < the smallest u seen" is a necessary condition that
// costs one compare, and the correctly rounded sqrt (~20 instructions) + 64-bit key update run only for candidates that pass
// it -- a lane has seen 16 (t - 1) columns before tile t, so few do.  Keys, hence ties (lowest index wins), are exactly those
// of the per-element form.
struct KeepNearest {
    unsigned long long run = NO_KEY;
    float ub = __builtin_inff();
    __device__ __forceinline__ void offer(float u, int col, bool in_range)
    {
        if (in_range && u < ub) {
            ub = u;
            const unsigned long long key = match_key(u, col);
            run = key < run ? key : run;
        }
    }
};

// Two running keys per lane, k1 < k2, and the u each of them came from.  A column whose u is not below ub2 has d >= the
// second distance and a larger index: its key cannot enter.  "u < ub2" (strict) is the one compare every element pays; the
// correctly rounded sqrt and the 64-bit updates run only behind it.  Keys are distinct (the index is part of the key), so
// "the two smallest keys of a row" is a pure function of the inputs whatever the order in which lanes, half-waves and shares
// are merged, and exact distance ties go to the lower index first.
struct KeepTwoNearest {
    float ub1 = __builtin_inff(), ub2 = __builtin_inff();
    unsigned long long k1 = NO_KEY, k2 = NO_KEY;
    __device__ __forceinline__ void offer(float u, int col, bool in_range)
    {
        if (in_range && u < ub2) {
            const unsigned long long key = match_key(u, col);
            if (key < k1) { k2 = k1; ub2 = ub1; k1 = key; ub1 = u; }
            else if (key < k2) { k2 = key; ub2 = u; }                 // (equal d, larger index: neither)
        }
    }
};

// The walk's gate: one more predicate on every (row, column) element, with whatever it needs of the tile's 32 columns staged
// next to the tile itself.  fetch(c0, ny) loads the part of tile c0 this thread stages into registers (it runs with the tile's
// own global loads, one tile ahead), stash(buf) puts it into LDS buffer `buf` (with the tile's own LDS stores, in front of the
// same barrier), pass(buf, slot) decides column c0 + slot of the tile in `buf` for the lane's row.  NoGate admits everything
// and compiles to nothing: the matchers without a gate are the code they were.
struct NoGate {
    __device__ __forceinline__ void fetch(int, int) {}
    __device__ __forceinline__ void stash(int) {}
    __device__ __forceinline__ bool pass(int, int) const { return true; }
};

// Offers every column of [c_begin, c_end) of Y (ny rows) that `gate` admits to `keep` for X row r0 + li, li = lane & 31; the
// lane's half-wave, half = lane >> 5, sees the columns with (col & 4) == 4 * half.  Called by all 256 threads of the
// workgroup: a wave without rows (returns false) still stages tiles and meets the barriers.
template <int D, class Keep, class Gate = NoGate>
__device__ __forceinline__ bool walk_tiles_whole(const float* __restrict__ X, const float* __restrict__ Y, int nx, int ny,
                                                 int c_begin, int c_end, int r0, int li, int half, Keep& keep, Gate gate = Gate())
{
    constexpr int RS = D + 4;                            // LDS row stride in floats
    __shared__ __attribute__((aligned(16))) float ytile[2][32 * RS];
    const int tid = threadIdx.x;
    const bool active = r0 < nx;

    constexpr int NG = D / 8;
    f32x4 a[NG];
    {
        const int row = min(r0 + li, nx - 1);
#pragma unroll
        for (int g = 0; g < NG; ++g)
            a[g] = *reinterpret_cast<const f32x4*>(X + (long long)row * D + g * 8 + half * 4);
    }
    // staging: the tile's 32 * D / 4 granules of 16 bytes, D / 32 per thread (rows beyond ny repeat row ny - 1; never selected)
    constexpr int GPT = D / 32, GPR = D / 4;
    f32x4 stage[GPT];
    auto gload = [&](int c0) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < GPT; ++k) {
            const int gran = tid + k * 256;
            const int row = gran / GPR, q = gran - row * GPR;
            stage[k] = *reinterpret_cast<const f32x4*>(Y + (long long)min(c0 + row, ny - 1) * D + q * 4);
        }
    };
    auto lstore = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < GPT; ++k) {
            const int gran = tid + k * 256;
            const int row = gran / GPR, q = gran - row * GPR;
            *reinterpret_cast<f32x4*>(&ytile[buf][row * RS + q * 4]) = stage[k];
        }
    };
    if (c_begin < c_end) { gload(c_begin); gate.fetch(c_begin, ny); lstore(0); gate.stash(0); }
    __syncthreads();
    for (int c0 = c_begin, buf = 0; c0 < c_end; c0 += 32, buf ^= 1) {
        const bool more = c0 + 32 < c_end;
        if (more) { gload(c0 + 32); gate.fetch(c0 + 32, ny); }     // in flight across this tile's MFMAs
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(&ytile[buf][li * RS + g * 8 + half * 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[e], a[g][e], acc, 0, 0, 0);      // acc[r]: column i(r) of the tile, row li
        }
        if (active) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int slot = (r & 3) + 8 * (r >> 2) + 4 * half, col = c0 + slot;
                const float t = fminf(fmaxf(acc[r], -1.f), 1.f);               // np.clip, matching.py:51
                keep.offer(2.f - 2.f * t, col, col < ny && gate.pass(buf, slot));
            }
        }
        if (more) { lstore(buf ^ 1); gate.stash(buf ^ 1); }       // last read one barrier ago
        __syncthreads();
    }
    return active;
}

// The same walk for rows wider than 256 floats, where neither a double-buffered tile of whole rows (2 x 32 x (D + 4) floats) fits
// the 64 KiB of static LDS nor the X row (D / 2 registers per lane) the register file next to the staging registers: D is walked
// in slices of 128 floats.  A step is (tile, slice); the steps are staged one ahead through the two LDS buffers exactly as the
// tiles are above, the lane re-reads its X row's slice at every step (L1 / L2 hits), and the 16 accumulators simply continue
// across the slices of a tile -- the products are added in ascending k, as for the other widths.  The gate's data belongs to a
// TILE: it is fetched with slice 0 of the tile and lies in the gate's buffer tile & 1.
template <int D, class Keep, class Gate = NoGate>
__device__ __forceinline__ bool walk_tiles_sliced(const float* __restrict__ X, const float* __restrict__ Y, int nx, int ny,
                                                  int c_begin, int c_end, int r0, int li, int half, Keep& keep, Gate gate = Gate())
{
    constexpr int SL = 128, NS = D / SL, RS = SL + 4;
    static_assert(D % SL == 0, "sliced walk: D must be a multiple of 128");
    __shared__ __attribute__((aligned(16))) float yslice[2][32 * RS];
    const int tid = threadIdx.x;
    const bool active = r0 < nx;
    const float* xrow = X + (long long)min(r0 + li, nx - 1) * D + half * 4;
    constexpr int NG = SL / 8, GPT = SL / 32, GPR = SL / 4;
    f32x4 stage[GPT];
    auto gload = [&](int c0, int sl) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < GPT; ++k) {
            const int gran = tid + k * 256;
            const int row = gran / GPR, q = gran - row * GPR;
            stage[k] = *reinterpret_cast<const f32x4*>(Y + (long long)min(c0 + row, ny - 1) * D + sl * SL + q * 4);
        }
    };
    auto lstore = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < GPT; ++k) {
            const int gran = tid + k * 256;
            const int row = gran / GPR, q = gran - row * GPR;
            *reinterpret_cast<f32x4*>(&yslice[buf][row * RS + q * 4]) = stage[k];
        }
    };
    if (c_begin < c_end) { gload(c_begin, 0); gate.fetch(c_begin, ny); lstore(0); gate.stash(0); }
    __syncthreads();
    int buf = 0;
    for (int c0 = c_begin, tb = 0; c0 < c_end; c0 += 32, tb ^= 1) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int sl = 0; sl < NS; ++sl, buf ^= 1) {
            const bool last = sl == NS - 1;
            const bool more = !last || c0 + 32 < c_end;
            if (more) {                                             // the next step, in flight across this one's MFMAs
                if (last) { gload(c0 + 32, 0); gate.fetch(c0 + 32, ny); }
                else gload(c0, sl + 1);
            }
            f32x4 a[NG];
#pragma unroll
            for (int g = 0; g < NG; ++g) a[g] = *reinterpret_cast<const f32x4*>(xrow + sl * SL + g * 8);
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const f32x4 bv = *reinterpret_cast<const f32x4*>(&yslice[buf][li * RS + g * 8 + half * 4]);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[e], a[g][e], acc, 0, 0, 0);
            }
            if (last && active) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int slot = (r & 3) + 8 * (r >> 2) + 4 * half, col = c0 + slot;
                    const float t = fminf(fmaxf(acc[r], -1.f), 1.f);
                    keep.offer(2.f - 2.f * t, col, col < ny && gate.pass(tb, slot));
                }
            }
            if (more) { lstore(buf ^ 1); if (last) gate.stash(tb ^ 1); }      // last read one barrier ago
            __syncthreads();
        }
    }
    return active;
}

// walk_tiles<D>: whole rows up to 256 floats, slices above
template <int D, class Keep, class Gate = NoGate>
__device__ __forceinline__ bool walk_tiles(const float* __restrict__ X, const float* __restrict__ Y, int nx, int ny,
                                           int c_begin, int c_end, int r0, int li, int half, Keep& keep, Gate gate = Gate())
{
    if constexpr (D > 256) return walk_tiles_sliced<D>(X, Y, nx, ny, c_begin, c_end, r0, li, half, keep, gate);
    else return walk_tiles_whole<D>(X, Y, nx, ny, c_begin, c_end, r0, li, half, keep, gate);
}

// What a rows kernel builds its walk's gate from, handed over as one by-value kernel argument: gate(dir, p, K, row) is the
// policy for the lane's X row `row` (clamped to the pair's rows) of pair p in direction dir.  Nothing at all for NoGate.
struct NoGateArgs {
    __device__ __forceinline__ NoGate gate(int, int, int, int) const { return {}; }
};

// best[x] = min over the y the gate admits of (dist(x,y) bits << 32 | y), X rows against the share's Y rows; NO_KEY for a row
// without candidates.
// grid: (row-block groups, pairs, 2 directions x column shares): blockIdx.z = direction + 2 * column share
template <int D, class GateArgs>
__global__ __launch_bounds__(256) void nn_rows_kernel(const float* __restrict__ dA, const int* __restrict__ nA,
                                                     const float* __restrict__ dB, const int* __restrict__ nB,
                                                     long long pair_stride, int count_stride, int K,
                                                     unsigned long long* __restrict__ bestA,
                                                     unsigned long long* __restrict__ bestB, int* __restrict__ match_count,
                                                     int nsplit, GateArgs gate_args)
{
    // (the pair's match counter, which the mutual epilogue adds to behind this launch, is zeroed here: one fill launch fewer)
    if (blockIdx.x == 0 && blockIdx.z == 0 && threadIdx.x == 0) match_count[blockIdx.y] = 0;
    const int p = blockIdx.y, dir = blockIdx.z & 1, share = blockIdx.z >> 1;
    const float* X = (dir == 0 ? dA : dB) + (long long)p * pair_stride;
    const float* Y = (dir == 0 ? dB : dA) + (long long)p * pair_stride;
    const int nx = min((dir == 0 ? nA : nB)[p * count_stride], K);
    const int ny = min((dir == 0 ? nB : nA)[p * count_stride], K);
    unsigned long long* best = (dir == 0 ? bestA : bestB) + ((long long)share * gridDim.y + p) * K;
    const ColumnShare cs = column_share(ny, share, nsplit);
    if ((int)blockIdx.x * 128 >= nx) return;             // (the whole workgroup)
    const int lane = threadIdx.x & 63, li = lane & 31, half = lane >> 5;
    const int r0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 32;
    KeepNearest keep;
    if (!walk_tiles<D>(X, Y, nx, ny, cs.c_begin, cs.c_end, r0, li, half, keep, gate_args.gate(dir, p, K, min(r0 + li, nx - 1)))) return;
    // the two half-waves hold the two halves of the row's columns
    const unsigned long long o = __shfl_xor(keep.run, 32);
    const int row = r0 + li;
    if (half == 0 && row < nx) best[row] = o < keep.run ? o : keep.run;
}

// ---- what the epilogue kernels and the launches of match_mfma.hip and match_guided.hip share ----

// the N smallest keys (k2 is untouched for N = 1) of row `at` over the column shares' arrays, which lie [share][pair][K][N]
template <int N>
__device__ __forceinline__ void merge_shares(const unsigned long long* __restrict__ best, long long at, int K, int nsplit,
                                             unsigned long long& k1, unsigned long long& k2)
{
    const long long share_stride = (long long)gridDim.y * K * N;
    at *= N;
    k1 = best[at];
    if constexpr (N == 2) k2 = best[at + 1];
    for (int sh = 1; sh < nsplit; ++sh) {
        if constexpr (N == 1) { const unsigned long long o = best[at + sh * share_stride]; k1 = o < k1 ? o : k1; }
        else merge2(k1, k2, best[at + sh * share_stride], best[at + sh * share_stride + 1]);
    }
}

// One best-or-no match per query row.  j < 0: none; j2 / d2: the second-nearest train row, for the entry that reports it
struct RowMatch { int j = -1, j2 = -1; float d = 0.f, d2 = 0.f; };

// The epilogue kernels' frame, one thread per query row i of pair p: match(p, i) decides the row, which is written
// (second_* may be NULL), and the workgroup adds its matches to the pair's count.
template <class Match>
__device__ __forceinline__ void write_matches(int K, int* __restrict__ match_idx, float* __restrict__ match_dist,
                                              int* __restrict__ match_count, int* __restrict__ second_idx,
                                              float* __restrict__ second_dist, Match match)
{
    const int p = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int hit = 0;
    if (i < K) {
        const RowMatch m = match(p, i);
        const long long o = (long long)p * K + i;
        match_idx[o] = m.j;
        match_dist[o] = m.j >= 0 ? m.d : 0.f;
        if (second_idx) second_idx[o] = m.j2;
        if (second_dist) second_dist[o] = m.j2 >= 0 ? m.d2 : 0.f;
        hit = m.j >= 0;
    }
    const int c = __syncthreads_count(hit);
    if (threadIdx.x == 0 && c) atomicAdd(&match_count[p], c);
}

// the mutual epilogue (match_mfma.hip) behind a launch of nn_rows_kernel: rowbest / colbest [MATCH_SHARES][P][K]
void launch_match_mutual_rows(const unsigned long long* rowbest, const unsigned long long* colbest, const int* nA, const int* nB,
                              int count_stride, int P, int K, float thr, int* match_idx, float* match_dist, int* match_count,
                              hipStream_t s);

// the row kernels exist for the descriptor widths the C entries admit: launch(integral_constant<int, D>)
template <class Launch>
void for_width(int D, Launch launch)
{
    if (D == 64) launch(std::integral_constant<int, 64>{});
    else if (D == 128) launch(std::integral_constant<int, 128>{});
    else if (D == 256) launch(std::integral_constant<int, 256>{});
    else launch(std::integral_constant<int, 384>{});
}
