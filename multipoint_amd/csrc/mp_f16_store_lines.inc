// Un-pooled epilogue of the fp16 implicit-GEMM kernels.  NOT a header: a fragment of a kernel body, included at the point where
// conv_f16_kernel and conv_f16_res_kernel store an un-pooled item (see mp_f16_store_pooled.inc for why it is text).  Names it
// expects in scope, besides that fragment's G, MBW, RELU, BNF, SLICED, p, acc, prm, wave, slice, img, y0, x0:
//   TAPS, px0                    1: flat mode, the item is 256 consecutive pixels from px0
//   lane, li, half               the lane, its pixel (lane & 31) and its half (lane >> 5)
//   MP_F16_STAGE, KS             macro (undefined again at the end) and constexpr int: the wave's 4 KiB staging block in LDS holds pixel px
//                                of an M-block at MP_F16_STAGE + (px >> 3) * KS + (px & 7) * 64 halfs (KS = 512: one contiguous block)
// lane = pixel, register r = channel (r&3) + 8*(r>>2) + 4*half of the N-block, i.e. 8-byte pieces 128 bytes apart: stored directly
// they cost 32 partial lines per store instruction (measured 20 % of an un-pooled launch).  So per M-block (32 pixels) every lane
// writes its eight 8-byte channel quads into the staging block, [pixel][granule ^ (pixel & 7)][8 halfs] (16-byte granules
// XOR-swizzled by the pixel's low bits instead of a padded stride), then lane l reads granule l & 7 of pixels l >> 3, + 8, + 16,
// + 24 and stores 16 bytes: eight lanes = one pixel's 64 channels = one 128-byte line.  Partial tiles send masked lanes to the
// dummy line, as in the pooled epilogue.
const int cs = p.out_cstride;
_Float16* obase;
bool full;
if constexpr (TAPS == 1) {
    obase = p.out + px0 * cs + p.out_coff + slice * 64;
    full = (px0 + 256 <= p.total_px) && (!SLICED || slice * 64 + 64 <= p.cout);
} else {
    obase = p.out + (((long long)img * p.H + y0) * p.W + x0) * cs + p.out_coff + slice * 64;
    full = (y0 + G::TH <= p.H) && (x0 + G::TW <= p.W) && (!SLICED || slice * 64 + 64 <= p.cout);
}
if (TAPS == 9 || !SLICED || slice * 64 + 64 <= p.cout) {      // (3x3 layers: cout is a multiple of 64, launch_conv_f16 refuses anything else)
    _Float16* const stg = MP_F16_STAGE;
    int lq = lane;
    asm volatile("" : "+v"(lq));              // the addresses below are item-invariant: keep hipcc from holding them in registers through the MFMA loop
    // halfs: this lane's pixel row, + the half's 8 bytes in a granule (KS = 512 written out: hipcc does not fold the general form)
    const int wrow = (KS == 512 ? (lq & 31) * 64 : ((lq & 31) >> 3) * KS + (lq & 7) * 64) + (lq >> 5) * 4, wsw = lq & 7;
    const int rg_l = lq & 7, rp0 = lq >> 3;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                const int cl = nb * 32 + rg * 8 + half * 4;
                const f32x4 b4 = *reinterpret_cast<const f32x4*>(&prm[cl]);
                const f32x4 s4 = *reinterpret_cast<const f32x4*>(&prm[64 + cl]);
                const f32x4 t4 = *reinterpret_cast<const f32x4*>(&prm[128 + cl]);
                const h2 lo = act_h2<RELU, BNF>(acc[mb][nb][rg * 4], acc[mb][nb][rg * 4 + 1], f32x2{b4[0], b4[1]},
                                                f32x2{s4[0], s4[1]}, f32x2{t4[0], t4[1]});
                const h2 hi = act_h2<RELU, BNF>(acc[mb][nb][rg * 4 + 2], acc[mb][nb][rg * 4 + 3], f32x2{b4[2], b4[3]},
                                                f32x2{s4[2], s4[3]}, f32x2{t4[2], t4[3]});
                *reinterpret_cast<h4*>(stg + wrow + (((nb * 4 + rg) ^ wsw) << 3)) = h4{lo[0], lo[1], hi[0], hi[1]};
            }
        asm volatile("" ::: "memory");                                // (same wave: the LDS executes its operations in order)
        _Float16* const mp = (TAPS == 1) ? obase + (long long)((2 * wave + mb) * 32) * cs
                                         : obase + (long long)((2 * wave + mb) * G::MBH) * p.W * cs;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int px = rp0 + 8 * k;                          // (rp0 < 8: px / MBW and the k-part of px % MBW are uniform)
            const h8 v = *reinterpret_cast<const h8*>(stg + (KS == 512 ? px * 64 : k * KS + rp0 * 64) + ((rg_l ^ rp0) << 3));
            _Float16* dst = (TAPS == 1) ? mp + (8 * k) * cs + (rp0 * cs + rg_l * 8)
                                        : mp + (((8 * k) / MBW) * p.W + (8 * k) % MBW) * cs + (rp0 * cs + rg_l * 8);
            if (!full) {
                bool okp;
                if constexpr (TAPS == 1) okp = px0 + (2 * wave + mb) * 32 + px < p.total_px;
                else okp = (y0 + (2 * wave + mb) * G::MBH + px / MBW < p.H) & (x0 + px % MBW < p.W);
                dst = okp ? dst : p.dummy + lane * 8;
            }
            *reinterpret_cast<h8*>(dst) = v;
        }
        asm volatile("" ::: "memory");
    }
} else if constexpr (TAPS == 1) {
    // a partial channel slice (cout = 65: the 1x1 detector head as its own launch): 8-byte stores straight from the registers
    const int lane_off = li * cs + half * 4;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
            const int cl = nb * 32 + rg * 8 + half * 4;
            const f32x4 b4 = *reinterpret_cast<const f32x4*>(&prm[cl]);
            const f32x4 s4 = *reinterpret_cast<const f32x4*>(&prm[64 + cl]);
            const f32x4 t4 = *reinterpret_cast<const f32x4*>(&prm[128 + cl]);
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                const h2 lo = act_h2<RELU, BNF>(acc[mb][nb][rg * 4], acc[mb][nb][rg * 4 + 1], f32x2{b4[0], b4[1]},
                                                f32x2{s4[0], s4[1]}, f32x2{t4[0], t4[1]});
                const h2 hi = act_h2<RELU, BNF>(acc[mb][nb][rg * 4 + 2], acc[mb][nb][rg * 4 + 3], f32x2{b4[2], b4[3]},
                                                f32x2{s4[2], s4[3]}, f32x2{t4[2], t4[3]});
                const h4 v = h4{lo[0], lo[1], hi[0], hi[1]};
                _Float16* const dst = obase + (long long)((2 * wave + mb) * 32) * cs + nb * 32 + rg * 8 + lane_off;
                const bool okp = px0 + (2 * wave + mb) * 32 + li < p.total_px;
                const int ch0 = slice * 64 + cl;
                if (ch0 + 3 < p.cout || !okp) {
                    *reinterpret_cast<h4*>(okp ? dst : p.dummy + lane * 4) = v;
                } else {                     // partial channel quad
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (ch0 + e < p.cout) dst[e] = v[e];
                }
            }
        }
}
#undef MP_F16_STAGE
