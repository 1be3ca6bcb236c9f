// Work-item arithmetic shared by the convolution kernels: a launch numbers its items (tile, slice) linearly and a workgroup
// takes an item apart by multiply-high division with constants the launcher computed; the staging offsets of an item's
// activation patch; the tile decode and the image-patch load of the first-block kernels.  Internal header.
#pragma once
#include "mp_common.h"
#include "mp_device.h"

#include <algorithm>

// Host side: the division constants and item count of a launch into q (ConvParams or ConvParamsH).
// magic = floor(2^32 / d) + 1 gives floor(n / d) == umulhi(n, magic) for all n with n * d < 2^32; returns 1 when the launch
// has more items than that 32-bit decode can address (nothing is launched, the caller reports MP_EINVAL), else 0.
template <typename P>
inline int tile_items(P& q, long long nitems)
{
    auto magic = [](int d) -> unsigned { return d <= 1 ? 0u : (unsigned)((0x100000000ull / (unsigned)d) + 1ull); };
    q.magic_slices = magic(q.nslices); q.magic_tx = magic(q.tiles_x); q.magic_ty = magic(q.tiles_y);
    const long long dmax = std::max(std::max(q.nslices, q.tiles_x), q.tiles_y);
    if (nitems * dmax >= 0x100000000ll) return 1;
    q.nitems = (int)nitems;
    return 0;
}

// exact division by multiply-high with the host's magic number: stays on the scalar unit (a runtime integer division costs
// ~20 VALU instructions, and VALU shares the pipe with fp32 MFMA)
__device__ __forceinline__ unsigned udiv(unsigned n, unsigned magic, unsigned d) { return d == 1 ? n : __umulhi(n, magic); }

// where an item of the 256-pixel-tile kernels lies: output slice, image, tile origin (3x3) or first pixel (flat 1x1 mode), and
// the wave-uniform base its staging loads start from: the image (3x3) or the tile's first pixel (1x1)
template <typename T>
struct TileWhere { int slice, img, y0, x0; long long px0; const T* in_base; };

// TH x TW: the tile; SLICED = false: the launch has one slice and `it` is the tile
template <typename T, int TAPS, int TH, int TW, bool SLICED = true, typename P>
__device__ __forceinline__ TileWhere<T> tile_decode(const P& p, int it)
{
    TileWhere<T> w{};
    int tile = it;
    if constexpr (SLICED) {
        tile = (int)udiv((unsigned)it, p.magic_slices, (unsigned)p.nslices);
        w.slice = it - tile * p.nslices;
    }
    if constexpr (TAPS == 9) {
        const int trow = (int)udiv((unsigned)tile, p.magic_tx, (unsigned)p.tiles_x);
        const int tx = tile - trow * p.tiles_x;
        const int bi = (int)udiv((unsigned)trow, p.magic_ty, (unsigned)p.tiles_y);
        const int ty = trow - bi * p.tiles_y;
        w.img = p.img_list ? p.img_list[bi] : bi;
        w.y0 = ty * TH; w.x0 = tx * TW;
        w.in_base = p.in + (long long)w.img * p.H * p.W * p.in_cstride + p.in_coff;
    } else {
        w.px0 = (long long)tile * 256;
        w.in_base = p.in + w.px0 * p.in_cstride + p.in_coff;
    }
    return w;
}

// every halo pixel of the item lies inside the frame (3x3), or all 256 pixels exist (flat 1x1 mode): no padding slots
template <int TAPS, int TH, int TW, typename T, typename P>
__device__ __forceinline__ bool is_interior(const P& p, const TileWhere<T>& w)
{
    if constexpr (TAPS == 9) return (w.y0 >= 1) && (w.y0 + TH < p.H) && (w.x0 >= 1) && (w.x0 + TW < p.W);
    else return w.px0 + 256 <= p.total_px;
}

// Staging offsets of item w for thread t of the 256 that stage its (TH + halo) x (TW + halo) patch, in elements: LPP lanes share a
// pixel and each fetches VEC channels (8 x 4 floats, 8 x 8 or 4 x 8 halfs), vector j of a thread is slot t + 256 j.  Interior
// items: offsets relative to the item's first halo pixel, IDENTICAL for every such item, so they are computed once (`rel` says
// goff holds them) and only the wave-uniform base pointer moves -- no VALU per item, and a wave that is not streaming MFMAs
// issues its vector instructions very slowly next to one that is.  Boundary items: offsets from in_base with -1 marking the
// padding slots, which are zero-filled at the LDS write.  Returns the base pointer the staging loads add goff to.
template <int TAPS, int TH, int TW, int VEC, int LPP, int NITER, typename T, typename P>
__device__ __forceinline__ const T* stage_offsets(const P& p, const TileWhere<T>& w, int t, int (&goff)[NITER], bool& rel)
{
    static_assert(LPP == 4 || LPP == 8, "lanes per pixel");
    constexpr int SH = LPP == 8 ? 3 : 2;
    constexpr int LW = TW + (TAPS == 9 ? 2 : 0), LH = TH + (TAPS == 9 ? 2 : 0), NV = LW * LH * LPP;
    // (is_interior written out: as a call of it conv_f16_kernel, which has no register to spare, spills ~50 registers)
    bool interior;
    if constexpr (TAPS == 9) interior = (w.y0 >= 1) && (w.y0 + TH < p.H) && (w.x0 >= 1) && (w.x0 + TW < p.W);
    else interior = w.px0 + 256 <= p.total_px;
    if (interior) {
        if (!rel) {
#pragma unroll
            for (int j = 0; j < NITER; ++j) {
                const int f = t + j * 256;
                const int lp = f >> SH;
                int off = 0;
                if (f < NV) {
                    if constexpr (TAPS == 9) {
                        const int ly = lp / LW, lx = lp - ly * LW;
                        off = (ly * p.W + lx) * p.in_cstride + (f & (LPP - 1)) * VEC;
                    } else {
                        off = lp * p.in_cstride + (f & (LPP - 1)) * VEC;
                    }
                }
                goff[j] = off;
            }
            rel = true;
        }
        if constexpr (TAPS == 9) return w.in_base + (long long)((w.y0 - 1) * p.W + (w.x0 - 1)) * p.in_cstride;
        else return w.in_base;
    }
    rel = false;
#pragma unroll
    for (int j = 0; j < NITER; ++j) {
        const int f = t + j * 256;
        const int lp = f >> SH, cv = f & (LPP - 1);
        int off = -1;
        if (f < NV) {
            if constexpr (TAPS == 9) {
                const int ly = lp / LW, lx = lp - ly * LW;
                const PadSource s = pad_source(w.y0 + ly - 1, w.x0 + lx - 1, p.H, p.W, p.pad_zero);
                if (!s.zero) off = (s.y * p.W + s.x) * p.in_cstride + cv * VEC;
            } else {
                if (w.px0 + lp < p.total_px) off = lp * p.in_cstride + cv * VEC;
            }
        }
        goff[j] = off;
    }
    return w.in_base;
}

// ---- first encoder block (Cin = 1): one workgroup of 256 threads per TH x TW tile, tiles numbered x-fastest inside an image ----
struct FirstTile { int img, y0, x0; };
template <int TH, int TW, typename P>
__device__ __forceinline__ FirstTile first_tile_decode(const P& p, int t)
{
    const int tiles_x = (p.W + TW - 1) / TW, tiles_y = (p.H + TH - 1) / TH;
    const int tx = t % tiles_x; t /= tiles_x;
    const int ty = t % tiles_y;
    const int bi = t / tiles_y;
    return {p.img_list ? p.img_list[bi] : bi, ty * TH, tx * TW};
}

// the tile's image patch with a ring of RING pixels, padded by the layer's rule, into patch[TH + 2 RING][TW + 2 RING];
// conv converts an element on its way in (identity, or the rounding to fp16 of autocast)
template <int TH, int TW, int RING, typename Conv>
__device__ __forceinline__ void patch_load(float* patch, const float* image, int y0, int x0, int H, int W, int pad_zero, int tid,
                                           Conv conv)
{
    constexpr int LW = TW + 2 * RING, LH = TH + 2 * RING;
    for (int f = tid; f < LH * LW; f += 256) {
        const int ly = f / LW, lx = f - ly * LW;
        const PadSource s = pad_source(y0 + ly - RING, x0 + lx - RING, H, W, pad_zero);
        patch[f] = conv(s.zero ? 0.f : image[s.y * W + s.x]);
    }
}
