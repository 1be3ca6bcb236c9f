// fp16 convolution path (model config `mixed_precision: true`, reference MultiPoint.py:99-103: the forward
// runs under torch.cuda.amp.autocast, i.e. Conv2d on fp16 inputs/weights with fp32 accumulation and fp16
// outputs, BatchNorm evaluated in fp32 on fp16 activations, fp16 results).  BASELINE config 5.
//
// Same implicit GEMM as conv_mfma.hip with the byte geometry kept: an LDS pixel is 64 fp16 channels (128 B,
// stride 144 B -> conflict-free ds_read_b128), a step is (tap, 16-channel group) and one 16-byte operand per
// lane feeds ONE v_mfma_f32_32x32x16_f16 (32 cycles, 16x the fp32 instruction's rate), so the operand
// streams have to be fetched much further ahead: weights 5 steps (ring of 6), activations 2 steps (ring of 3).
// Rounding points (all round-to-nearest-even, as autocast produces them):
//   conv: fp32 accumulate (+ fp16 bias) -> fp16;  ReLU;  BN: fp32 affine on the fp16 value -> fp16;  max-pool.
#include "mp_common.h"
#include "mp_device.h"
#include "mp_f16.h"
#include "mp_tile.h"

#include <algorithm>
#include <type_traits>

// developer instrumentation: per-workgroup cycle sums per phase (wave 0), see tools/conv_timing.py f16
MP_TIMING_TABLE(g_timing_h, 512 * 8, mp_debug_read_timing_f16)
MP_TIMING_HEIGHT(g_timing_h_sel, 1024, mp_debug_select_height_f16)       // only launches whose input height matches are recorded

namespace {

constexpr int CKH = 64;        // input channels per LDS chunk
constexpr int PSH = CKH + 8;   // LDS pixel stride in halfs (144 B)

template <int TAPS, int MBW>
struct GeoH {
    static constexpr int MBH = 32 / MBW;
    static constexpr int TW = MBW;
    static constexpr int TH = 256 / MBW;
    static constexpr int HALO = (TAPS == 9) ? 1 : 0;
    static constexpr int LW = TW + 2 * HALO;
    static constexpr int LH = TH + 2 * HALO;
    static constexpr int NPIX = LW * LH;
    static constexpr int NV = NPIX * (CKH / 8);          // 16-byte vectors per chunk tile
    static constexpr int NITER = (NV + 255) / 256;       // staging vectors per thread
    static constexpr int STEPS = TAPS * (CKH / 16);      // k16-steps per chunk
};

__device__ __forceinline__ float round_h(float v) { return (float)(_Float16)v; }

template <int TAPS, int MBW, bool POOL, bool BNF>
__global__ __launch_bounds__(256, 2) void conv_f16_kernel(const ConvParamsH p)
{
    using G = GeoH<TAPS, MBW>;
    constexpr bool RELU = (TAPS == 9);
    constexpr bool SWAP = !POOL;      // weights as the MFMA A operand -> lane = pixel, register quad = 4 channels
    __shared__ __attribute__((aligned(16))) _Float16 lds[G::NPIX * PSH];
    // bias | BN scale | BN shift of the current 64-channel slice: fetched from global memory only when the slice
    // changes (a global load in every epilogue costs its L2 latency per item)
    __shared__ __attribute__((aligned(16))) float prm[3 * 64];
    // un-pooled layers: the waves' staging blocks of mp_f16_store_lines.inc, 4 KiB each
    __shared__ __attribute__((aligned(16))) _Float16 ostage[POOL ? 8 : 4 * 2048];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5;
    const int li = lane & 31;

    // ---- persistent workgroup: walks work items (tile, slice) of its XCD's contiguous eighth of the item space,
    //      gridDim.x/8 items apart, and fetches the NEXT item's activation tile while multiplying the current one
    //      (an fp16 tile is only ~4.6 k cycles of MFMA: without the prefetch the HBM latency of every tile is exposed)
    const XcdRange xr = xcd_range(p.nitems, p.xcd_shift);
    const int stride = xr.stride, item_end = xr.item_end;
    int item = xr.item;

    using Where = TileWhere<_Float16>;
    auto decode = [&](int it) __attribute__((always_inline)) -> Where { return tile_decode<_Float16, TAPS, G::TH, G::TW>(p, it); };
    // per-thread staging offsets in halfs and the base pointer the staging loads of item w add them to (mp_tile.h)
    int goff[G::NITER];
    bool goff_rel = false;          // goff currently holds the item-invariant relative offsets
    bool cur_pad = false;           // the LDS image being written has padding slots
    auto offsets = [&](const Where& w) __attribute__((always_inline)) -> const _Float16* {
        return stage_offsets<TAPS, G::TH, G::TW, 8, 8>(p, w, tid, goff, goff_rel);
    };

    const int a_base = (((2 * wave) * G::MBH + li / MBW) * G::LW + (li % MBW)) * PSH + half * 8;
    constexpr int A_MB = G::MBH * G::LW * PSH;
    const int nchunks = p.cin / CKH;

    constexpr int RB = (G::STEPS % 6 == 0) ? 6 : 4;      // weight ring (divides STEPS: stays aligned across chunks)
    constexpr int PF = RB - 1;                           // steps of weight prefetch
    constexpr int RA = 3;                                // activation-fragment ring (restarted per chunk)
    static_assert(G::STEPS % RB == 0, "weight ring must stay aligned across chunks");
    h8 af[RA][2], bf[RB][2], stg[G::NITER];
    constexpr int S0 = (TAPS == 9) ? 4 : 0;               // first step that issues a staging load
    constexpr int PER_STEP = (TAPS == 9) ? 1 : 2;
    auto a_off = [](int s) -> int {
        const int tap = s >> 2, gg = s & 3;
        const int kh = (TAPS == 9) ? tap / 3 : 0, kw = (TAPS == 9) ? tap % 3 : 0;
        return (kh * G::LW + kw) * PSH + gg * 16;
    };
    auto mma = [](const h8& a, const h8& b, const f32x16& cc) -> f32x16 {
        return SWAP ? __builtin_amdgcn_mfma_f32_32x32x16_f16(b, a, cc, 0, 0, 0)
                    : __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, cc, 0, 0, 0);
    };

    if (item >= item_end) return;
    Where cur = decode(item);
    const _Float16* src = offsets(cur);                    // staging base of the item being loaded
    cur_pad = !goff_rel;
#pragma unroll
    for (int j = 0; j < G::NITER; ++j)
        stg[j] = *reinterpret_cast<const h8*>(src + (goff[j] >= 0 ? goff[j] : 0));

    auto lds_write = [&]() __attribute__((always_inline)) {
        if (!cur_pad) {
#pragma unroll
            for (int j = 0; j < G::NITER; ++j) {
                const int f = tid + j * 256;
                if (f < G::NV) *reinterpret_cast<h8*>(&lds[(f >> 3) * PSH + (f & 7) * 8]) = stg[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < G::NITER; ++j) {
                const int f = tid + j * 256;
                if (f < G::NV) {
                    h8 v = stg[j];
                    if (goff[j] < 0) v = h8{0, 0, 0, 0, 0, 0, 0, 0};
                    *reinterpret_cast<h8*>(&lds[(f >> 3) * PSH + (f & 7) * 8]) = v;
                }
            }
        }
    };
    lds_write();
    auto load_prm = [&](int slice) __attribute__((always_inline)) {
        if (tid < 64) {
            prm[tid] = p.bias[slice * 64 + tid]; prm[64 + tid] = p.scale[slice * 64 + tid]; prm[128 + tid] = p.shift[slice * 64 + tid];
        }
    };
    load_prm(cur.slice);
    // weights: [slice][chunk][step][nb][lane][8 halfs]; ONE linear stream per item, and the tail of an item's
    // prefetch already reads the head of the next item's stream, so it is never restarted after this point
    const h8* wp = reinterpret_cast<const h8*>(p.wpack) + ((long long)cur.slice * nchunks) * (G::STEPS * 128) + lane;
#pragma unroll
    for (int s = 0; s < PF; ++s) { bf[s][0] = wp[s * 128]; bf[s][1] = wp[s * 128 + 64]; }
    __syncthreads();

#ifdef MP_TIMING
    unsigned long long tsum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const bool t_on = (p.H == g_timing_h_sel);      // read once: a global load inside the loop would add a vmcnt(0) wait
#endif
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (;;) {
        MP_CLOCK(t_item);
        f32x16 acc[2][2];      // not zero-initialised: the first MFMAs of the item take a literal-zero C operand
        const int item_next = item + stride;
        const bool has_next = item_next < item_end;
        Where nxt = cur;
        const h8* wnext = wp;
        const _Float16* cur_src = src;
        bool nxt_pad = cur_pad;

        auto chunk_body = [&](const int c, auto first_tag) __attribute__((always_inline)) {
            constexpr bool FIRST = decltype(first_tag)::value;
            // source of the staging loads issued during this chunk: the next chunk of this item, or chunk 0 of the
            // next item (whose offsets replace goff: the LDS image of the current chunk is already written)
            const bool last = c + 1 == nchunks;
            const _Float16* in_next;
            if (!last) {
                in_next = cur_src + (c + 1) * CKH;
            } else {
                if (has_next) {
                    nxt = decode(item_next);
                    src = offsets(nxt);
                    nxt_pad = !goff_rel;
                    // (from an opaque copy of the lane id: `p.wpack + lane` is item-invariant, and hipcc kept it as a 64-bit register pair
                    // through the MFMA loop -- spilled, and its reload here was an s_waitcnt vmcnt(0) on the loads in flight)
                    int lw = lane;
                    asm volatile("" : "+v"(lw));
                    wnext = reinterpret_cast<const h8*>(p.wpack) + ((long long)nxt.slice * nchunks) * (G::STEPS * 128) + lw;
                }
                in_next = src;                                  // !has_next: dummy re-read of the current tile
            }
            const h8* wc = wp + (long long)c * (G::STEPS * 128);
            const h8* wt = last ? wnext : wc + G::STEPS * 128;   // where the prefetch continues after this chunk
            MP_CLOCK(t_steps0);
            if (c == 0) MP_CLOCK_ADD(0, t_item, t_steps0);          // item start -> first step (decode, offsets)
#pragma unroll
            for (int s = 0; s < RA - 1; ++s) {
                af[s][0] = *reinterpret_cast<const h8*>(&lds[a_base + a_off(s)]);
                af[s][1] = *reinterpret_cast<const h8*>(&lds[a_base + A_MB + a_off(s)]);
            }
#pragma unroll
            for (int s = 0; s < G::STEPS; ++s) {
                // ONE memory instruction behind each MFMA: issued as a burst in front of the four MFMAs of a step, the same
                // loads cost ~45 cycles of matrix-pipe time each instead of ~10 (round-2 probe; docs/HISTORY.md A.3)
                const h8* const wsrc = (s + PF < G::STEPS) ? wc + (s + PF) * 128 : wt + (s + PF - G::STEPS) * 128;
                acc[0][0] = mma(af[s % RA][0], bf[s % RB][0], (FIRST && s == 0) ? zero16 : acc[0][0]);
                __builtin_amdgcn_sched_barrier(0);
                bf[(s + PF) % RB][0] = wsrc[0];
                __builtin_amdgcn_sched_barrier(0);
                acc[0][1] = mma(af[s % RA][0], bf[s % RB][1], (FIRST && s == 0) ? zero16 : acc[0][1]);
                __builtin_amdgcn_sched_barrier(0);
                bf[(s + PF) % RB][1] = wsrc[64];
                __builtin_amdgcn_sched_barrier(0);
                acc[1][0] = mma(af[s % RA][1], bf[s % RB][0], (FIRST && s == 0) ? zero16 : acc[1][0]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < PER_STEP; ++u) {
                    const int j = (s - S0) * PER_STEP + u;
                    if (s >= S0 && j < G::NITER)      // unconditional load: keeps the compiler's vmcnt counting exact
                        stg[j] = *reinterpret_cast<const h8*>(in_next + (goff[j] >= 0 ? goff[j] : 0));
                }
                __builtin_amdgcn_sched_barrier(0);
                acc[1][1] = mma(af[s % RA][1], bf[s % RB][1], (FIRST && s == 0) ? zero16 : acc[1][1]);
                __builtin_amdgcn_sched_barrier(0);
                if (s + RA - 1 < G::STEPS) {
                    const int sn = s + RA - 1;
                    af[sn % RA][0] = *reinterpret_cast<const h8*>(&lds[a_base + a_off(sn)]);
                    af[sn % RA][1] = *reinterpret_cast<const h8*>(&lds[a_base + A_MB + a_off(sn)]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            MP_CLOCK(t_steps1);
            MP_CLOCK_ADD(1, t_steps0, t_steps1);                    // the MFMA steps of a chunk
            __syncthreads();                                   // this chunk's LDS image fully consumed
            MP_CLOCK(t_bar);
            MP_CLOCK_ADD(2, t_steps1, t_bar);                       // barrier skew
            if (last) cur_pad = nxt_pad;
            if (!last || has_next) lds_write();                // staged registers are free again before the epilogue
            MP_CLOCK(t_ldsw);
            MP_CLOCK_ADD(3, t_bar, t_ldsw);                         // staging data landed + LDS write
            if (!last) __syncthreads();
        };
        chunk_body(0, std::true_type{});
        for (int c = 1; c < nchunks; ++c) chunk_body(c, std::false_type{});
        MP_CLOCK(t_epi0);

        // ---------------- epilogue of item `cur` ----------------
        const int slice = cur.slice, img = cur.img, y0 = cur.y0, x0 = cur.x0;
        const long long px0 = cur.px0;
        constexpr bool SLICED = true;
        if constexpr (POOL) {
            int lq = lane;
            asm volatile("" : "+v"(lq));      // (why: mp_f16_store_pooled.inc)
            const int li = lq & 31, half = lq >> 5;
#include "mp_f16_store_pooled.inc"
        } else {
            constexpr int KS = 512;
#define MP_F16_STAGE (ostage + wave * 2048)
#include "mp_f16_store_lines.inc"
        }
        MP_CLOCK(t_epi1);
        MP_CLOCK_ADD(4, t_epi0, t_epi1);                            // epilogue
#ifdef MP_TIMING
        tsum[7] += 1;
        if (!has_next && tid == 0 && t_on)
            for (int i = 0; i < 8; ++i) g_timing_h[blockIdx.x * 8 + i] = tsum[i];
#endif
        if (!has_next) return;
        __syncthreads();                                       // next item's LDS image complete, every epilogue done
        if (nxt.slice != cur.slice) load_prm(nxt.slice);       // (rare) visible to the next epilogue via the post-steps barrier
        MP_CLOCK(t_bar2);
        MP_CLOCK_ADD(5, t_epi1, t_bar2);
        item = item_next;
        cur = nxt;
        wp = wnext;
    }
}

template <int TAPS, int MBW, bool POOL>
int launch_h(const ConvParamsH& p, hipStream_t s)
{
    long long ntiles;
    if (TAPS == 9) ntiles = (long long)p.B * p.tiles_x * p.tiles_y;
    else ntiles = (p.total_px + 255) / 256;
    const long long nitems = ntiles * p.nslices;
    if (nitems <= 0) return 0;
    ConvParamsH q = p;
    if (tile_items(q, nitems)) return 1;
    // persistent workgroups: two per CU, a multiple of the XCD count
    const long long nblk = persistent_grid(nitems, p.ncu, p.xcd_shift, 2);
    const ConvParamsH& pp = q;
    if (p.bn_first)
        hipLaunchKernelGGL((conv_f16_kernel<TAPS, MBW, POOL, true>), dim3((unsigned)nblk), dim3(256), 0, s, pp);
    else
        hipLaunchKernelGGL((conv_f16_kernel<TAPS, MBW, POOL, false>), dim3((unsigned)nblk), dim3(256), 0, s, pp);
    return 0;
}

// ---- first encoder block, fp16 flavour: image (fp32 in HBM, rounded to fp16 as autocast casts the conv input)
//      -> 64 fp16 channels.  HBM-write bound: thread = (pixel, 8 channels), one 16-byte store.
constexpr int FTH = 32, FTW = 64, FLW = FTW + 2, FLH = FTH + 2;

__global__ __launch_bounds__(256) void conv_first_f16_kernel(const Conv1ParamsH p)
{
    __shared__ float tile[FLH * FLW];
    const int tid = threadIdx.x;
    const FirstTile t = first_tile_decode<FTH, FTW>(p, blockIdx.x);
    const int img = t.img, y0 = t.y0, x0 = t.x0;
    patch_load<FTH, FTW, 1>(tile, p.in + (long long)img * p.H * p.W, y0, x0, p.H, p.W, p.pad_zero, tid, round_h);
    // channel pairs in f32x2 registers: the 72 multiply-adds and the activation of a pixel's 8 channels are packed
    // instructions (v_pk_fma_f32 with the pixel value broadcast, act_h2) -- the kernel is otherwise VALU-bound
    // (~180 scalar VALU instructions per 16-byte store against ~116 clocks of HBM time per KiB and CU)
    const int c8 = (tid & 7) * 8;
    f32x2 w[9][4], bia[4], scl[4], sft[4];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) w[k][e] = f32x2{p.w[k * 64 + c8 + 2 * e], p.w[k * 64 + c8 + 2 * e + 1]};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        bia[e] = f32x2{p.bias[c8 + 2 * e], p.bias[c8 + 2 * e + 1]};
        scl[e] = f32x2{p.scale[c8 + 2 * e], p.scale[c8 + 2 * e + 1]};
        sft[e] = f32x2{p.shift[c8 + 2 * e], p.shift[c8 + 2 * e + 1]};
    }
    __syncthreads();
    const int psub = tid >> 3;                    // 32 pixels per pass
    auto pixel = [&](int py, int px) __attribute__((always_inline)) -> h8 {
        float x[9];
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) x[kh * 3 + kw] = tile[(py + kh) * FLW + px + kw];
        h8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            f32x2 a = {0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 9; ++k) a = __builtin_elementwise_fma(f32x2{x[k], x[k]}, w[k][e], a);
            const h2 r = p.bn_first ? act_h2<true, true>(a[0], a[1], bia[e], scl[e], sft[e])
                                    : act_h2<true, false>(a[0], a[1], bia[e], scl[e], sft[e]);
            o[2 * e] = r[0]; o[2 * e + 1] = r[1];
        }
        return o;
    };
    if (p.pool) {
        // double_convolution: false -- Conv -> ReLU -> BN -> MaxPool2d(2,2) under autocast: the maximum of four fp16 values (exact)
        const int Ho = p.H >> 1, Wo = p.W >> 1;
        _Float16* out = p.out + (long long)img * Ho * Wo * 64;
        for (int it = 0; it < (FTH * FTW) / 4 / 32; ++it) {
            const int pix = it * 32 + psub;
            const int py = pix / (FTW / 2), px = pix % (FTW / 2);
            const h8 a = pixel(2 * py, 2 * px), b = pixel(2 * py, 2 * px + 1), c = pixel(2 * py + 1, 2 * px), d = pixel(2 * py + 1, 2 * px + 1);
            h8 o;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const _Float16 m0 = a[i] > b[i] ? a[i] : b[i], m1 = c[i] > d[i] ? c[i] : d[i];
                o[i] = m0 > m1 ? m0 : m1;
            }
            const int oy = (y0 >> 1) + py, ox = (x0 >> 1) + px;
            if (oy < Ho && ox < Wo) *reinterpret_cast<h8*>(out + ((long long)oy * Wo + ox) * 64 + c8) = o;
        }
        return;
    }
    _Float16* out = p.out + (long long)img * p.H * p.W * 64;
#pragma unroll 2
    for (int it = 0; it < (FTH * FTW) / 32; ++it) {
        const int pix = it * 32 + psub;
        const int py = pix / FTW, px = pix % FTW;
        const h8 o = pixel(py, px);
        const int oy = y0 + py, ox = x0 + px;
        if (oy < p.H && ox < p.W) __builtin_nontemporal_store(o, reinterpret_cast<h8*>(out + ((long long)oy * p.W + ox) * 64 + c8));   // streaming, as conv_first.hip
    }
}

}  // namespace

int launch_conv_f16(const ConvParamsH& p, int taps, int mbw, bool pool, hipStream_t s)
{
    if (taps == 1) return launch_h<1, 32, false>(p, s);
    if (p.cout != 64 * p.nslices) return 2;            // 3x3 layers: whole 64-channel slices (the model loader pads them)
    if (mbw == 32) return pool ? launch_h<9, 32, true>(p, s) : launch_h<9, 32, false>(p, s);
    if (mbw == 16) return pool ? launch_h<9, 16, true>(p, s) : launch_h<9, 16, false>(p, s);
    return pool ? launch_h<9, 8, true>(p, s) : launch_h<9, 8, false>(p, s);
}

void launch_conv_first_f16(const Conv1ParamsH& p, hipStream_t s)
{
    const int tiles_x = (p.W + FTW - 1) / FTW, tiles_y = (p.H + FTH - 1) / FTH;
    const long long nblk = (long long)p.B * tiles_x * tiles_y;
    if (nblk <= 0) return;
    hipLaunchKernelGGL(conv_first_f16_kernel, dim3((unsigned)nblk), dim3(256), 0, s, p);
}
