// Second half of the split small launches of the F(4x4,3x3) kernels (single-pair latency, B <= 2: conv_wino43.hip / conv_wino43b.hip
// with p.ks_shift > 0).  Those launches run the input channels of a (tile block, slice) item as 2^ks_shift separate items -- enough
// workgroups to fill the GPU -- and leave each range's PRE-BIAS output tiles in p.split_scratch.  This kernel, the next launch on the
// stream, sums the ranges' shares in range order (deterministic), adds the bias, applies ReLU / BatchNorm [and the 2x2 max-pool] and
// stores the result: one thread per (item, thread of the convolution workgroup, channel pair, pair of output rows), so the 8 values
// x up to 8 ranges a thread needs are ONE round trip of independent loads.  (Round 3 did the same inside the convolution launch --
// the last range to arrive, found through a device-scope counter, gathered the shares: 64 values x 8 ranges per thread are 8-16
// dependent ~1.5 us trips behind a write-through / counter / barrier hand-off, which was most of what a small launch cost.)
// What an item is, which tile and channels a thread of the convolution workgroup owns and where its shares lie is mp_wino43.h's,
// as it is the convolution kernels': the item shape, the item decode, the tile numbering and the share index are the same calls.
#include "mp_common.h"
#include "mp_device.h"
#include "mp_tile.h"
#include "mp_wino43.h"

namespace {

// GEN 1: conv_wino43.hip, GEN 2: conv_wino43b.hip
template <int GEN, bool POOL, bool BNF, int TC4>
__global__ __launch_bounds__(256) void split_reduce_kernel(const ConvParams p)
{
    using Share = W43Share<GEN>;
    constexpr int T = Share::T;
    constexpr int NQ = Share::NV / 8;                  // (m,) h, row pair
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int tid = (int)(gid % T), q = (int)((gid / T) % NQ);
    const int g = (int)(gid / (T * NQ));               // (tile block, slice)
    if (g >= p.nitems) return;
    const W43Item at = w43_item<TC4>(p, g);
    const int lane = tid & 63, wave = tid >> 6;
    int t_ty, t_tx;
    w43_tile_pos<GEN, TC4>(w43_lane_tile(wave & 1, lane), t_ty, t_tx);
    const int ap = q & 1;                              // output rows 2 ap, 2 ap + 1 of the 4 x 4 tile
    const int h = (q >> 1) & 1, m = q >> 2;            // channel pair of the lane's quad, column block (generation 2)
    const int KS = 1 << p.ks_shift;
    const unsigned long long* const part = reinterpret_cast<const unsigned long long*>(p.split_scratch) +
                                           ((long long)g << p.ks_shift) * Share::ITEM + w43_share_index<GEN>(m, h, 2 * ap, 0) + tid;
    unsigned long long rawv[8][8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k < KS) {
#pragma unroll
            for (int i = 0; i < 8; ++i) rawv[k][i] = part[(long long)k * Share::ITEM + w43_share_index<GEN>(0, 0, i >> 2, i & 3)];
        }
    const int ch = at.slice * 64 + w43_lane_channel<GEN>(wave >> 1, lane, m) + 2 * h;            // this thread's two output channels
    const f32x2 bb = {p.bias[ch], p.bias[ch + 1]}, ss = {p.scale[ch], p.scale[ch + 1]}, tt = {p.shift[ch], p.shift[ch + 1]};
    f32x2 yv[2][4];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        f32x2 v = __builtin_bit_cast(f32x2, rawv[0][i]);
#pragma unroll
        for (int k = 1; k < 8; ++k)
            if (k < KS) v += __builtin_bit_cast(f32x2, rawv[k][i]);         // range order: deterministic
        yv[i >> 2][i & 3] = w43_act<BNF>(v, 2 * ap + (i >> 2), i & 3, bb, ss, tt);
    }
    if (ch >= p.cout) return;
    const int oy = at.y0 + 4 * t_ty, ox = at.x0 + 4 * t_tx;
    const int Ho = POOL ? p.H >> 1 : p.H, Wo = POOL ? p.W >> 1 : p.W;
    const int cs = p.out_cstride;
    // NHWC: pixel stride cs floats; planar [B][cout/4][Ho][Wo][4]: the channel pair is floats 2h, 2h+1 of plane ch / 4
    float* const img_base = p.out_planar ? p.out + (long long)at.img * (p.cout / 4) * Ho * Wo * 4 + ((long long)(ch >> 2) * Ho * Wo) * 4 + (ch & 3)
                                         : p.out + (long long)at.img * Ho * Wo * cs + p.out_coff + ch;
    const int ps = p.out_planar ? 4 : cs;
    if (POOL) {
        const int py = (oy >> 1) + ap;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int px = (ox >> 1) + b;
            f32x2 r;
#pragma unroll
            for (int c = 0; c < 2; ++c)
                r[c] = fmaxf(fmaxf(yv[0][2 * b][c], yv[0][2 * b + 1][c]), fmaxf(yv[1][2 * b][c], yv[1][2 * b + 1][c]));
            if (py < Ho && px < Wo) *reinterpret_cast<f32x2*>(img_base + ((long long)py * Wo + px) * ps) = r;
        }
    } else {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int py = oy + 2 * ap + a, px = ox + b;
                if (py < Ho && px < Wo) *reinterpret_cast<f32x2*>(img_base + ((long long)py * Wo + px) * ps) = yv[a][b];
            }
    }
}

template <int GEN>
int launch_r(const ConvParams& p, bool pool, hipStream_t s)
{
    const int tc4 = w43_launch_tc4(p.H, p.W, false);
    ConvParams q = p;
    if (w43_launch_items(q, tc4, false)) return 1;
    if (q.nitems == 0) return 0;
    const long long threads = (long long)q.nitems * W43Share<GEN>::ITEM / 8;        // a thread sums 8 values of every range
    w43_dispatch(tc4, pool, p.bn_first, [&](auto pool_tag, auto bnf_tag, auto tc4_tag) {
        hipLaunchKernelGGL((split_reduce_kernel<GEN, decltype(pool_tag)::value, decltype(bnf_tag)::value, decltype(tc4_tag)::value>),
                           dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, q);
    });
    return 0;
}

}  // namespace

// p: the layer's parameters as forward.hip built them (REAL slices, ks_shift > 0); gen: 1 conv_wino43.hip, 2 conv_wino43b.hip
int launch_split_reduce(const ConvParams& p, int gen, bool pool, hipStream_t s)
{
    return gen == 1 ? launch_r<1>(p, pool, s) : launch_r<2>(p, pool, s);
}
