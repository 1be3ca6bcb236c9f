// Pooled epilogue of the fp16 implicit-GEMM kernels.  NOT a header: a fragment of a kernel body, included at the point where
// conv_f16_kernel and conv_f16_res_kernel store a pooled item.  It is text and not a function because conv_f16_kernel sits at
// the register limit and hipcc allocates it differently around a callee, although the callee is inlined (DESIGN.md section 9).
// Names it expects in scope:
//   G, MBW, RELU, BNF            the kernel's geometry and activation switches
//   SLICED                       constexpr bool: the layer has several 64-channel slices (false: exactly 64 output channels)
//   p, acc[2][2], prm            launch parameters, the wave's accumulators, bias | BN scale | BN shift of the slice in LDS
//   wave, slice, img, y0, x0     wave of the four, and where the item lies
//   li, half, lq                 the lane's channel (lq & 31), its half (lq >> 5) and the lane -- conv_f16_kernel derives them from an
//                                OPAQUE copy of the lane id so that hipcc recomputes the lane's item-invariant values (parameter
//                                addresses, store offset) per item instead of carrying them through the MFMA loop: it spilled 7
// Addressing: wave-uniform 64-bit base (scalar unit) + one per-lane 32-bit offset computed once per item + uniform per-store
// increments.  `full` items (tile entirely inside the output) store unconditionally; partial tiles send masked lanes to a
// dummy line so that BOTH paths issue the same number of stores and hipcc's vmcnt counting stays exact (a guarded store would
// make the next item's first operand wait cover every store).
// lane = channel (li), register r = pixel (r&3) + 8*(r>>2) + 4*half of the M-block; registers r, r+1 are horizontally adjacent
// pixels -> one packed pair
f32x2 bia[2], scl[2], sft[2];
#pragma unroll
for (int nb = 0; nb < 2; ++nb) {
    const float b = prm[nb * 32 + li], sc = prm[64 + nb * 32 + li], sh = prm[128 + nb * 32 + li];
    bia[nb] = f32x2{b, b}; scl[nb] = f32x2{sc, sc}; sft[nb] = f32x2{sh, sh};
}
const int Ho = p.H >> 1, Wo = p.W >> 1;
const int cs = p.out_cstride;
// Pool BEFORE the activation: bias add, fp16 rounding and ReLU are non-decreasing and the BatchNorm affine is monotonic in the direction of its
// scale's sign, so the maximum of a window's four activations IS the activation of the maximum (scale < 0: the minimum) of its
// four accumulators, bit for bit -- one activation per pooled value instead of four (channels li and 32 + li share a packed pair)
const f32x2 biap = {bia[0][0], bia[1][0]}, sclp = {scl[0][0], scl[1][0]}, sftp = {sft[0][0], sft[1][0]};
const bool neg0 = sclp[0] < 0.f, neg1 = sclp[1] < 0.f;
auto pooled_first = [&](const float (&q)[2][4]) __attribute__((always_inline)) -> h2 {
    const float x0 = fmaxf(fmaxf(q[0][0], q[0][1]), fmaxf(q[0][2], q[0][3])), n0 = fminf(fminf(q[0][0], q[0][1]), fminf(q[0][2], q[0][3]));
    const float x1 = fmaxf(fmaxf(q[1][0], q[1][1]), fmaxf(q[1][2], q[1][3])), n1 = fminf(fminf(q[1][0], q[1][1]), fminf(q[1][2], q[1][3]));
    return act_h2<RELU, BNF>(neg0 ? n0 : x0, neg1 ? n1 : x1, biap, sclp, sftp);
};
const bool full = (y0 + G::TH <= p.H) && (x0 + G::TW <= p.W) && (!SLICED || slice * 64 + 64 <= p.cout);
const int lane_off = 2 * half * cs + li;
_Float16* const obase = p.out + ((long long)img * Ho * Wo) * cs + p.out_coff + slice * 64;
// MBW == 32: rows 2*wave (mb 0) and 2*wave+1 (mb 1) pool together; otherwise both rows of a window are
// registers r and r+RDOWN of one M-block
constexpr int RDOWN = (MBW == 32) ? 0 : (MBW == 16) ? 8 : 4;
constexpr int NMB = (MBW == 32) ? 1 : 2;
auto store_all = [&](auto full_tag) __attribute__((always_inline)) {
    constexpr bool FULL = decltype(full_tag)::value;
#pragma unroll
    for (int mb = 0; mb < NMB; ++mb)
#pragma unroll
        for (int r = 0; r < 16; r += 2) {
            if (RDOWN != 0 && (r & RDOWN) != 0) continue;
            const int iu = (r & 3) + 8 * (r >> 2);                       // lane-independent part of the pixel index
            const int oy = (MBW == 32) ? (y0 + 2 * wave) >> 1 : (y0 + (2 * wave + mb) * G::MBH + iu / MBW) >> 1;
            const int oxu = (x0 + iu % MBW) >> 1;                        // + 2*half per lane
            _Float16* const rowp = obase + ((long long)oy * Wo + oxu) * cs;
            h2 vp;
            {
                float q[2][4];
#pragma unroll
                for (int nb = 0; nb < 2; ++nb) {
                    if constexpr (MBW == 32) {
                        q[nb][0] = acc[0][nb][r]; q[nb][1] = acc[0][nb][r + 1]; q[nb][2] = acc[1][nb][r]; q[nb][3] = acc[1][nb][r + 1];
                    } else {
                        q[nb][0] = acc[mb][nb][r]; q[nb][1] = acc[mb][nb][r + 1];
                        q[nb][2] = acc[mb][nb][r + RDOWN]; q[nb][3] = acc[mb][nb][r + RDOWN + 1];
                    }
                }
                vp = pooled_first(q);
            }
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) {
                const _Float16 v = vp[nb];
                if constexpr (FULL) {
                    rowp[nb * 32 + lane_off] = v;
                } else {
                    const bool ok = (oy < Ho) & (oxu + 2 * half < Wo) & (!SLICED || slice * 64 + nb * 32 + li < p.cout);
                    _Float16* dst = ok ? rowp + nb * 32 + lane_off : p.dummy + lq;
                    *dst = v;
                }
            }
        }
};
if (full) store_all(std::true_type{}); else store_all(std::false_type{});
