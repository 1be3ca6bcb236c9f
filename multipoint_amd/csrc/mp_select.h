// Ordered stream compaction and exact top-k selection shared by keypoints.hip and sift.hip (gfx950, wave64).  Internal header.
// Ballot-free shuffle scans give every kept entry its rank in thread order without atomics, so the output order of a compaction
// is the input order; an 8-bit radix select over fp32 score bits finds the exact k-th largest score of a list.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ int wave_incl_scan(int v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int n = __shfl_up(v, off);
        if (lane >= off) v += n;
    }
    return v;
}

// exclusive prefix of `c` over a workgroup of NT threads in thread order; returns block total via *total
template <int NT>
__device__ __forceinline__ int block_excl_scan(int c, int* s_wave, int* total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int inc = wave_incl_scan(c, lane);
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) {
        const int x = s_wave[i];
        if (i < w) base += x;
        tot += x;
    }
    __syncthreads();
    *total = tot;
    return base + inc - c;
}

// The cut of the k largest of nk keys (key_at(i), i < nk, nk > k > 0; non-negative fp32 bits order like the floats): admit the
// keys > T plus the first `need` entries == T.  A 4-pass 8-bit radix select by a workgroup of NT >= 256 threads; s_hist [256],
// s_wave [NT / 64] and s_sel [2] are its LDS scratch.  Every thread returns the same (T, need).
template <int NT, class KeyAt>
__device__ __forceinline__ void radix_select_cut(KeyAt key_at, int nk, int k, unsigned* s_hist, int* s_wave, unsigned* s_sel,
                                                 unsigned* T, int* need)
{
    const int tid = threadIdx.x;
    unsigned prefix = 0, mask = 0;
    int kk = k;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) s_hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < nk; i += NT) {
            const unsigned key = key_at(i);
            if ((key & mask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        // the digit d with (#keys of a larger digit) < kk <= (#keys of digit >= d), found by all 256 threads at once (thread t
        // holds bin t; suffix count = total - exclusive prefix): a single thread walking the bins down took a dependent LDS
        // read per bin, 256 x 4 passes = half of the kernel's 66 us
        {
            const int hcnt = tid < 256 ? (int)s_hist[tid] : 0;
            int tot;
            const int before = block_excl_scan<NT>(hcnt, s_wave, &tot);      // bins 0 .. t-1
            const int ge = tot - before;                                 // bins t .. 255
            if (tid == 0) { s_sel[0] = 0u; s_sel[1] = (unsigned)(tot - hcnt); }      // (fewer than kk keys: digit 0, as the walk did)
            __syncthreads();
            if (tid > 0 && tid < 256 && ge >= kk && ge - hcnt < kk) { s_sel[0] = (unsigned)tid; s_sel[1] = (unsigned)(ge - hcnt); }
        }
        __syncthreads();
        prefix |= s_sel[0] << shift;
        mask |= 255u << shift;
        kk -= (int)s_sel[1];
        __syncthreads();
    }
    *T = prefix;
    *need = kk;
}
