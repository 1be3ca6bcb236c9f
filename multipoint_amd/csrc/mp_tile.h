// Work-item arithmetic shared by the convolution kernels: a launch numbers its items (tile, slice) linearly and a workgroup
// takes an item apart by multiply-high division with constants the launcher computed.  Internal header.
#pragma once
#include "mp_common.h"

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
