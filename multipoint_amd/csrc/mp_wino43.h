// What the F(4x4,3x3) sources -- conv_wino43.hip (generation 1), conv_wino43b.hip (generation 2), conv_split.hip and the launch plan
// in forward.hip -- must agree on, and nothing else: which 32 tiles an item holds and how they are numbered, how a launch numbers
// its items, where a lane's four output channels sit, and where a range's share of a split launch lies in split_scratch.
// Internal header.
//
// Item = 32 tiles of 4x4 output pixels x 64 output channels.  The tiles are 4 rows x 8 columns (TC4 = 8: 16 x 32 pixels) or 8 rows x
// 4 columns (TC4 = 4: 32 x 16 pixels); a launch's items are (tile block, slice) with the slice fastest, tile blocks x-fastest inside
// an image.  A SPLIT launch numbers VIRTUAL slices = slice * ranges + range (ranges = 2^ks_shift ranges of input channels).
#pragma once
#include "mp_common.h"
#include "mp_device.h"
#include "mp_tile.h"

#include <type_traits>

constexpr int W43_UC = 4;                          // input channels per unit
constexpr int W43_VUNIT = W43_UC * 32 * 36;        // floats of a (tile block, unit) in vglobal: [ch][tile][pos] (18 KiB)

template <int TC4>
struct W43Shape {
    static_assert(TC4 == 4 || TC4 == 8, "item shape");
    static constexpr int TR4 = 32 / TC4;           // tile rows (TC4: tile columns) of an item
    static constexpr int OY = 4 * TR4, OX = 4 * TC4;   // output pixels of an item
    static constexpr int PY = OY + 2, PX = OX + 2;     // raw patch
};

// A range's share of an item in split_scratch: the pre-bias output tiles as f32x2 (a channel pair) [m][h][a][b][thread] -- thread of
// the convolution workgroup (T), m = MFMA column block (generation 2 only), h = channel pair of the lane's quad, (a, b) = output
// row / column of the lane's tile.  Either generation: 128 KiB per (virtual) item.
template <int GEN>
struct W43Share {
    static_assert(GEN == 1 || GEN == 2, "kernel generation");
    static constexpr int T = GEN == 1 ? 512 : 256;     // threads of a convolution workgroup
    static constexpr int NM = GEN == 1 ? 1 : 2;        // column blocks of 16 output channels per wave
    static constexpr int NV = NM * 2 * 16;             // shares per thread
    static constexpr int ITEM = NV * T;                // f32x2 per (virtual) item
};
static_assert(W43Share<1>::ITEM == W43Share<2>::ITEM, "forward.hip sizes split_scratch for either generation");
template <int GEN>
__host__ __device__ constexpr int w43_share_index(int m, int h, int a, int b) { return (((m * 2 + h) * 4 + a) * 4 + b) * W43Share<GEN>::T; }

// ---- host side ----

// the item shape that covers an H x W frame with fewer items (16 x 32 pixels on a tie: longer contiguous patch rows), and the
// tile blocks of one image in that shape
struct W43Cover { int tc4; long long blocks; };
inline W43Cover w43_cover(int H, int W)
{
    const long long wide = (long long)((W + 31) / 32) * ((H + 15) / 16), tall = (long long)((W + 15) / 16) * ((H + 31) / 32);
    return tall < wide ? W43Cover{4, tall} : W43Cover{8, wide};
}
// the item shape of a launch: the fused first block (conv_wino43.hip F1) is instantiated for 16 x 32-pixel items only
inline int w43_launch_tc4(int H, int W, bool fuse_first) { return fuse_first ? 8 : w43_cover(H, W).tc4; }
// bytes of split_scratch for `vitems` virtual items, floats of vglobal for the layer p
inline size_t w43_split_bytes(long long vitems) { return (size_t)vitems * W43Share<1>::ITEM * sizeof(f32x2); }
inline long long w43_vglobal_floats(const ConvParams& p) { return (long long)p.B * w43_cover(p.H, p.W).blocks * (p.cin / W43_UC) * W43_VUNIT; }

// q, a launch's copy of the layer's parameters: the tile blocks of an image for items of shape tc4, the slices (vslices: the
// virtual slices of a SPLIT launch), the division constants and the item count (0: nothing to launch).  Returns 1 when the
// launch has more items than the decode can address (tile_items), else 0.
inline int w43_launch_items(ConvParams& q, int tc4, bool vslices)
{
    const int OY = 4 * (32 / tc4), OX = 4 * tc4;
    if (vslices) q.nslices <<= q.ks_shift;
    q.tiles_x = (q.W + OX - 1) / OX; q.tiles_y = (q.H + OY - 1) / OY;
    const long long nitems = (long long)q.B * q.tiles_x * q.tiles_y * q.nslices;
    q.nitems = 0;
    return nitems <= 0 ? 0 : tile_items(q, nitems);
}

// One launch of layer p with items of shape tc4, as the launchers of both generations AND mp_forward_plan size it: q = the launch's
// copy of the parameters (w43_launch_items), grid = its persistent workgroups (0: no items, nothing to launch).  Returns
// w43_launch_items' code.
inline int w43_launch_shape(const ConvParams& p, int tc4, bool vslices, ConvParams& q, unsigned& grid)
{
    q = p; grid = 0;
    if (w43_launch_items(q, tc4, vslices)) return 1;
    if (q.nitems > 0) grid = persistent_grid(q.nitems, p.ncu, p.xcd_shift);
    return 0;
}

// runtime (tc4, pool, bn_first) -> f(POOL, BNF, TC4) with the three as std::integral_constant values
template <typename F>
inline void w43_dispatch(int tc4, bool pool, bool bn_first, F&& f)
{
    auto pick = [](bool v, auto&& g) { if (v) g(std::true_type{}); else g(std::false_type{}); };
    pick(pool, [&](auto P) { pick(bn_first, [&](auto B) { pick(tc4 == 4, [&](auto T) { f(P, B, std::integral_constant<int, decltype(T)::value ? 4 : 8>{}); }); }); });
}

// ---- device side ----

// where an item lies: (virtual) slice, image, first output pixel
struct W43Item { int slice, img, y0, x0; };

template <int TC4>
__device__ __forceinline__ W43Item w43_block(const ConvParams& p, int tile)
{
    W43Item w{};
    const int trow = (int)udiv((unsigned)tile, p.magic_tx, (unsigned)p.tiles_x);
    const int tx = tile - trow * p.tiles_x;
    const int bi = (int)udiv((unsigned)trow, p.magic_ty, (unsigned)p.tiles_y);
    const int ty = trow - bi * p.tiles_y;
    w.img = p.img_list ? p.img_list[bi] : bi;
    w.y0 = ty * W43Shape<TC4>::OY; w.x0 = tx * W43Shape<TC4>::OX;
    return w;
}
template <int TC4>
__device__ __forceinline__ W43Item w43_item(const ConvParams& p, int it)
{
    const int tile = (int)udiv((unsigned)it, p.magic_slices, (unsigned)p.nslices);
    const int slice = it - tile * p.nslices;
    W43Item w = w43_block<TC4>(p, tile);
    w.slice = slice;
    return w;
}
// the slice alone
__device__ __forceinline__ int w43_slice(const ConvParams& p, int it)
{
    return it - (int)udiv((unsigned)it, p.magic_slices, (unsigned)p.nslices) * p.nslices;
}

// tile tl of an item -> its tile row / column.  Generation 1 numbers the tiles row by row; generation 2 so that 16 consecutive
// tiles are 4 tile rows x 4 tile columns (TC4 = 8: tl = 16 (tx >> 2) + 4 ty + (tx & 3)), which keeps its column pass free of LDS
// bank conflicts
template <int GEN, int TC4>
__device__ __forceinline__ void w43_tile_pos(int tl, int& t_ty, int& t_tx)
{
    if constexpr (GEN == 1) { t_ty = tl / TC4; t_tx = tl % TC4; }
    else if constexpr (TC4 == 8) { t_ty = (tl >> 2) & 3; t_tx = 4 * (tl >> 4) + (tl & 3); }
    else { t_ty = tl >> 2; t_tx = tl & 3; }
}

// The GEMMs' output fragment: a wave multiplies tile block tb (16 tiles; wave & 1) by channel block cb (wave >> 1: 16 couts,
// generation 2: two column blocks m of 16) with the weights as the A operand -- lane = tile, register quad = 4 consecutive output
// channels.  The lane's tile of the item, and the first of its 4 output channels in the slice:
__device__ __forceinline__ int w43_lane_tile(int tb, int lane) { return tb * 16 + (lane & 15); }
template <int GEN>
__device__ __forceinline__ int w43_lane_channel(int cb, int lane, int m = 0)
{
    return cb * (16 * W43Share<GEN>::NM) + m * 16 + 4 * (lane >> 4);
}

// bias and activation of output (r, c) of a tile, in the model's order (z: the scaled transform's value, at6s())
template <bool BNF>
__device__ __forceinline__ f32x2 w43_act(f32x2 z, int r, int c, f32x2 bias, f32x2 scale, f32x2 shift)
{
    f32x2 v = w43_add_bias(z, r, c, bias);
    if (BNF) { v = v * scale + shift; return f32x2{relu_bits(v[0]), relu_bits(v[1])}; }
    v = f32x2{relu_bits(v[0]), relu_bits(v[1])};
    return v * scale + shift;
}
