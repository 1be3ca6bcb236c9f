// Shared declarations for the gfx950 (MI355X / CDNA4) kernels of libmultipoint_hip.so.
// Internal header: the public C ABI is include/multipoint_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

#define MP_WAVE 64

// is v a finite double?  (one comparison; false for NaN.  The kernels and the entries that check their arguments share it)
__host__ __device__ __forceinline__ bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }

// activation tensor layouts of the fp32 F(4x4,3x3) launches (ConvParams::in_planar / out_planar)
enum { MP_LAYOUT_NHWC = 0, MP_LAYOUT_PLANAR = 1, MP_LAYOUT_XPLANAR = 2 };

// ---------------------------------------------------------------------------------------------
// conv (implicit GEMM on v_mfma_f32_32x32x2_f32)
// ---------------------------------------------------------------------------------------------
// Activations are NHWC fp32.  One workgroup (256 threads = 4 waves) produces a tile of 256 output
// pixels x 64 output channels; the 256 pixels are 8 "M-blocks" of 32 pixels, an M-block being
// (32/MBW) rows x MBW columns, stacked vertically:  tile = (256/MBW) rows x MBW cols.
// Wave w owns M-blocks 2w, 2w+1 and both 32-wide N-blocks of the 64-channel slice.
struct ConvParams {
    const float* in;      // [B][H][W][in_cstride], channels [in_coff, in_coff+cin) are read
    float* out;           // [B][Ho][Wo][out_cstride], channels [out_coff, out_coff+cout) written
    const float* wpack;   // packed weights, see pack_mfma_weights() in model_load.hip
    const float* bias;    // [nslices*64] conv bias (zero padded)
    const float* scale;   // [nslices*64] BN scale  s = gamma / sqrt(var + eps)
    const float* shift;   // [nslices*64] BN shift  t = beta - mean * s
    const int* img_list;  // optional: image ids this launch processes (nullptr = 0..B-1)
    // fused first encoder block (FUSE1 variants): the image and the Cin=1 layer's parameters
    const float* img;     // [B][H][W]
    const float *w1, *b1, *s1, *t1;   // [9][64] tap-major weights, bias, BN scale, BN shift
    int B, H, W;          // conv input == conv output spatial size (stride 1, 'same' padding)
    int in_cstride, in_coff, cin;
    int out_cstride, out_coff, cout;
    int nslices;          // ceil(cout / 64)
    int tiles_x, tiles_y; // tiles per image
    int pad_zero;         // 0: reflection pad (ReflectionPad2d(1)), 1: zero pad (ZeroPad2d(1))
    int bn_first;         // 0: conv -> ReLU -> BN (reference default), 1: conv -> BN -> ReLU
    int relu;             // 0: no ReLU (final 1x1 convs)
    long long total_px;   // TAPS==1 (flat) mode: number of pixels
    unsigned magic_slices, magic_tx, magic_ty;   // multiply-high division constants (filled in by the launcher)
    int nitems;           // work items (tile, slice) of the launch (filled in by the launcher)
    int persist;          // 0: per-tile kernel only; n > 0: persistent workgroups for launches with >= n items per CU
    // conv_wino43.hip only: channel-quad-planar tensors [B][C/4][H][W][4] instead of NHWC (a unit of 4 input channels is then
    // contiguous row by row: its patch DMA touches ~10 cache lines per instruction instead of 64), or -- MP_LAYOUT_XPLANAR, behind an
    // un-pooled conv_wino43_kernel launch -- column-interleaved planar [B][C/4][H][4 = x mod 4][W/4 = x div 4][4]: the tile columns
    // of an item are then consecutive 16-byte pieces, so an epilogue store instruction writes whole cache lines.  MP_LAYOUT_*
    // values; conv_wino43b.hip, the split-K reduction and conv_first.hip know the first two only
    int in_planar, out_planar;
    // machine shape (api.hip: mp_create derives it from the device, forward.hip: run_conv copies it into every launch): compute units of
    // the device = workgroups of a one-per-CU persistent grid, and log2 of its XCD count (workgroup b runs on XCD b mod nxcd;
    // each XCD has its own L2, so a persistent workgroup walks a contiguous share of ITS XCD's items)
    int ncu, xcd_shift;
    // conv_wino43.hip / conv_wino43b.hip, small launches (single-pair latency): the input channels of an item are cut into 2^ks_shift ranges that
    // run as separate items; their pre-bias output tiles meet in split_scratch, and split_reduce_kernel (conv_split.hip, the next
    // launch on the stream) sums them in range order and runs the rest of the epilogue.  ks_shift = 0: off.
    int ks_shift;
    float* split_scratch;     // [virtual item][32 or 64 values][512 or 256 threads] f32x2 (128 KiB per virtual item; mp_wino43.h: W43Share)
    // conv_wino43.hip, layers with many output slices (the 3x3 head convolutions): the input transform runs as a pass of its own
    // into vglobal [tile block][cin / 4][4][32][36] (conv_wino43_vglobal_floats()) and every slice's launch items DMA V from there
    // instead of transforming the same windows again.  nullptr: the transform runs inside the kernel, per slice.
    float* vglobal;
};

// persistent schedule shared by the persistent kernels: the items are cut into one contiguous range per XCD, and the
// workgroups of an XCD (blockIdx mod nxcd, gridDim a multiple of nxcd) walk that range with the stride of their number
struct XcdRange { int item, item_end, stride; };
__device__ __forceinline__ XcdRange xcd_range(int nitems, int xcd_shift)
{
    const int nxcd = 1 << xcd_shift;
    const int per_xcd = (nitems + nxcd - 1) >> xcd_shift;
    const int xcd = (int)blockIdx.x & (nxcd - 1);
    XcdRange r;
    r.stride = (int)gridDim.x >> xcd_shift;
    r.item_end = min((xcd + 1) * per_xcd, nitems);
    r.item = xcd * per_xcd + ((int)blockIdx.x >> xcd_shift);
    return r;
}
// host side: workgroups of a persistent launch with `per_cu` workgroups per CU -- never more than the items rounded up to a
// multiple of the XCD count (every XCD gets the same number of workgroups)
inline unsigned persistent_grid(long long nitems, int ncu, int xcd_shift, int per_cu = 1)
{
    const long long nxcd = 1ll << xcd_shift;
    const long long full = ((long long)ncu * per_cu) / nxcd * nxcd;
    const long long need = (nitems + nxcd - 1) / nxcd * nxcd;
    return (unsigned)(need < full ? need : full);
}

// first layer (Cin = 1, direct VALU conv, HBM-write bound)
struct Conv1Params {
    const float* in;      // [B][H][W]
    float* out;           // [B][H][W][channels]
    const float* w;       // [9][channels]  (tap-major, cout contiguous)
    const float* bias; const float* scale; const float* shift;   // [channels]
    const int* img_list;
    int B, H, W;
    int pad_zero, bn_first;
    int channels;         // output channels incl. zero padding: 64 (channel_version 0) or 32
    int out_planar;       // write [B][channels/4][H][W][4] (the consumer is conv_wino43.hip) instead of NHWC
    int pool;             // double_convolution: false (MultiPoint.py:147-148): MaxPool2d(2,2) follows the block -> out [B][H/2][W/2][channels]
};

// the conv launchers return 0, or 1 when the launch has more work items than the kernels' 32-bit magic-number tile decode
// can address (items * max divisor >= 2^32): nothing is launched and the caller reports MP_EINVAL
int launch_conv_mfma(const ConvParams& p, int taps, int mbw, bool pool, bool fuse1, hipStream_t s);
void launch_conv_first(const Conv1Params& p, hipStream_t s);
// the batch-statistics forward's un-pooled 3x3 convolution of bn_first models, and their first block: conv + bias, no activation
// (the BatchNorm that follows needs the pre-ReLU values)
int launch_conv_mfma_linear(const ConvParams& p, int mbw, hipStream_t s);
void launch_conv_first_linear(const Conv1Params& p, hipStream_t s);
// Winograd F(4x4,3x3) (conv_wino43.hip): p.wpack = pack_wino43_weights() output; supports() says whether the shape is covered
// Interpolation points of the F(4x4,3x3) transforms: {0, +-a, +-b, inf}.  The textbook choice a = 1, b = 2 (Lavin & Gray) has
// integer transform matrices but the worst conditioning of the family: its fp32 error is ~20x that of a direct fp32
// convolution.  The same set scaled by 3/4 -- a = 3/4, b = 3/2 -- keeps every transform coefficient an exact binary
// fraction (a^2 = 9/16, b^2 = 9/4, a^2 b^2 = 81/64, a^2 + b^2 = 45/16), keeps the even/odd structure (12 multiply-adds per
// 1-D input transform, as before) and cuts the maximum error 3.4x and the rms error 2x (CPU emulation over a grid of dyadic
// (a, b): the minimum is broad around a b ~ 1, b / a ~ 2; docs/HISTORY.md section 4).  Shared by the kernel and the host-side
// weight transform U = G g G^T (model_load.hip).
#ifndef MP_W43_A
#define MP_W43_A 0.75
#endif
#ifndef MP_W43_B
#define MP_W43_B 1.5
#endif
// Packed fp32 arithmetic as explicit instructions: hipcc scalarises a third of the input transform's packed multiply-adds (4
// v_fma_f32 for 2 v_pk_fma_f32 per pass), and next to an MFMA stream every vector instruction costs matrix-pipe time
// (docs/HISTORY.md A.3).  The transform coefficients come in scalar register pairs (VOP3P takes no literal on gfx950).
// Two coefficients share one scalar register pair (low / high half, picked by op_sel: the selected half feeds both lanes), so the
// six coefficients of the input transform occupy three pairs instead of six (SGPRs are what the fused-first-block instantiation
// of conv_wino43.hip is shortest of).
constexpr unsigned long long pk_const2(double lo, double hi)
{
    return (unsigned long long)__builtin_bit_cast(unsigned, (float)lo) | ((unsigned long long)__builtin_bit_cast(unsigned, (float)hi) << 32);
}
constexpr double W43A = MP_W43_A, W43B = MP_W43_B;                  // interpolation points {0, +-a, +-b, inf}
constexpr unsigned long long K_AB = pk_const2(W43A, W43B), K_BA = pk_const2(W43B, W43A), K_A2B2 = pk_const2(W43A * W43A, W43B * W43B),
                             K_B2A2 = pk_const2(W43B * W43B, W43A * W43A),
                             K_PS = pk_const2(W43A * W43A * W43B * W43B, W43A * W43A + W43B * W43B);
static_assert((double)(float)(W43A * W43A * W43B * W43B) == W43A * W43A * W43B * W43B && (double)(float)(W43A * W43A + W43B * W43B) ==
              W43A * W43A + W43B * W43B, "the transform coefficients must be exact in fp32");
// HI = 0: the low half of k, 1: the high half
template <int HI>
__device__ __forceinline__ f32x2 pk_fma_k(f32x2 a, unsigned long long k, f32x2 c)      // a * k + c
{
    f32x2 d;
    if (HI) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(d) : "v"(a), "s"(k), "v"(c));
    else asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,1]" : "=v"(d) : "v"(a), "s"(k), "v"(c));
    return d;
}
template <int HI>
__device__ __forceinline__ f32x2 pk_fnma_k(f32x2 a, unsigned long long k, f32x2 c)     // c - a * k
{
    f32x2 d;
    if (HI) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1] neg_lo:[1,0,0] neg_hi:[1,0,0]" : "=v"(d) : "v"(a), "s"(k), "v"(c));
    else asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0] neg_hi:[1,0,0]" : "=v"(d) : "v"(a), "s"(k), "v"(c));
    return d;
}
// 1-D input transform B^T d (6 -> 6) of the F(4x4,3x3) kernels, packed over two channels: 12 multiply-adds.  Row of point p = the
// coefficients of x (x^2 - a^2)(x^2 - b^2) / (x - p), last row the polynomial itself:
//   B^T = [a^2 b^2, 0, -(a^2+b^2), 0, 1, 0;  0, -+a b^2, -b^2, +-a, 1, 0 (p = +-a);  0, -+b a^2, -a^2, +-b, 1, 0 (p = +-b);
//          0, a^2 b^2, 0, -(a^2+b^2), 0, 1]
__device__ __forceinline__ void bt6(const f32x2 d[6], f32x2 r[6])
{
    const f32x2 t0 = pk_fnma_k<1>(d[2], K_A2B2, d[4]);      // d4 - b^2 d2      (even part of the +-a rows)
    const f32x2 t1 = pk_fnma_k<1>(d[1], K_A2B2, d[3]);      // d3 - b^2 d1      (odd part / a)
    const f32x2 t2 = pk_fnma_k<0>(d[2], K_A2B2, d[4]);      // d4 - a^2 d2      (+-b rows)
    const f32x2 t3 = pk_fnma_k<0>(d[1], K_A2B2, d[3]);      // d3 - a^2 d1
    r[0] = pk_fma_k<0>(d[0], K_PS, pk_fnma_k<1>(d[2], K_PS, d[4]));      // a^2 b^2 d0 + (d4 - (a^2+b^2) d2)
    r[1] = pk_fma_k<0>(t1, K_AB, t0);                          // t0 + a t1
    r[2] = pk_fnma_k<0>(t1, K_AB, t0);                         // t0 - a t1
    r[3] = pk_fma_k<1>(t3, K_AB, t2);                          // t2 + b t3
    r[4] = pk_fnma_k<1>(t3, K_AB, t2);                         // t2 - b t3
    r[5] = pk_fma_k<0>(d[1], K_PS, pk_fnma_k<1>(d[3], K_PS, d[5]));      // a^2 b^2 d1 + (d5 - (a^2+b^2) d3)
}
// 1-D output transform A^T m (6 -> 4) of the F(4x4,3x3) kernels, packed over two output channels, with the powers of `a` factored
// out of rows 1 and 2: A^T[i][p] = p^i over the points (0, a, -a, b, -b, inf) and b = 2a give
//   y0 = m0 + s1 + s2,  y1 = a (d1 + 2 d2),  y2 = a^2 (s1 + 4 s2),  y3 = a^3 (d1 + 8 d2) + m5     (s = sums, d = differences)
// so z = (y0, y1 / a, y2 / a^2, y3) takes 10 packed instructions instead of 13 (every bracket is ONE multiply-add with an exact
// coefficient), and the factor sigma_r sigma_c, sigma = (1, a, a^2, 1), of output (r, c) goes into the multiply-add that adds the
// bias anyway (w43_out_scale; 1, a .. a^4 are exact binary fractions).  Two roundings fewer per y1 / y2 than the plain form.
static_assert(MP_W43_B == 2 * MP_W43_A, "at6s() needs b = 2a");
__device__ __forceinline__ void at6s(const f32x2 m[6], f32x2 z[4])
{
    constexpr float a3 = (float)(MP_W43_A * MP_W43_A * MP_W43_A);
    const f32x2 s1 = m[1] + m[2], d1 = m[1] - m[2], s2 = m[3] + m[4], d2 = m[3] - m[4];
    z[0] = (m[0] + s1) + s2;
    z[1] = __builtin_elementwise_fma(d2, f32x2{2.f, 2.f}, d1);
    z[2] = __builtin_elementwise_fma(s2, f32x2{4.f, 4.f}, s1);
    z[3] = __builtin_elementwise_fma(__builtin_elementwise_fma(d2, f32x2{8.f, 8.f}, d1), f32x2{a3, a3}, m[5]);
}
constexpr float w43_sigma(int r) { return r == 1 ? (float)MP_W43_A : r == 2 ? (float)(MP_W43_A * MP_W43_A) : 1.f; }
constexpr float w43_out_scale(int r, int c) { return w43_sigma(r) * w43_sigma(c); }
// pre-bias output (r, c) of a tile from the scaled transform's value + the bias: ONE multiply-add (an add where the factor is 1)
__device__ __forceinline__ f32x2 w43_add_bias(f32x2 z, int r, int c, f32x2 bias)
{
    const float k = w43_out_scale(r, c);
    return k == 1.f ? z + bias : __builtin_elementwise_fma(z, f32x2{k, k}, bias);
}
bool conv_wino43_supports(const ConvParams& p);
long long conv_wino43_items(const ConvParams& p);      // work items the launch would have (B x tile blocks x slices)
long long conv_wino43_vglobal_floats(const ConvParams& p);      // size of ConvParams::vglobal for this layer
int launch_conv_wino43(const ConvParams& p, bool pool, hipStream_t s, bool fuse_first = false);
// second generation (conv_wino43b.hip): one wave per SIMD, whole-window input transform; any frame size
bool conv_wino43b_supports(const ConvParams& p);
int launch_conv_wino43b(const ConvParams& p, bool pool, hipStream_t s);
// the split small launches' second half (conv_split.hip): sums the ranges' shares, activation, [pool], store; gen 1 / 2 = which kernel wrote them
int launch_split_reduce(const ConvParams& p, int gen, bool pool, hipStream_t s);

// fp16 path (mixed_precision: activations and packed weights fp16, fp32 accumulate; conv_f16.hip).
// Same tiling as ConvParams; a chunk is 64 input channels, so cin must be a multiple of 64.
struct ConvParamsH {
    const _Float16* in;   // [B][H][W][in_cstride]
    _Float16* out;        // [B][Ho][Wo][out_cstride]
    const _Float16* wpack;
    const float* bias;    // fp16-representable values
    const float* scale;   // fp32 BN terms (BatchNorm runs in fp32 under autocast)
    const float* shift;
    const int* img_list;
    int B, H, W;
    int in_cstride, in_coff, cin;
    int out_cstride, out_coff, cout;
    int nslices, tiles_x, tiles_y;
    int pad_zero, bn_first;
    long long total_px;
    unsigned magic_slices, magic_tx, magic_ty;
    int nitems;           // work items (tile, slice) of the launch (filled in by the launcher)
    _Float16* dummy;      // >= 1 KiB scratch line that masked-off store lanes write to
    int ncu, xcd_shift;   // machine shape, as in ConvParams
    int res_groups;       // conv_f16_res.hip: independent four-wave groups per CU (3; 2 = MP_DEBUG=f16_res_groups=2; the fused-first-block launch always runs 2)
    // conv_f16_res.hip with the first encoder block fused in: the fp32 image [B][H][W] and the Cin = 1 layer's parameters
    // ([9][64] tap-major fp16-representable weights, bias, BN scale / shift); img == nullptr: p.in is read
    const float* img;
    const float *w1, *b1, *s1, *t1;
};
struct Conv1ParamsH {
    const float* in;      // [B][H][W] fp32 image (rounded to fp16 on load)
    _Float16* out;        // [B][H][W][64]
    const float* w;       // [9][64] fp16-representable values
    const float* bias; const float* scale; const float* shift;
    const int* img_list;
    int B, H, W;
    int pad_zero, bn_first;
    int pool;             // double_convolution: false (MultiPoint.py:147-148): MaxPool2d(2,2) follows the block -> out [B][H/2][W/2][64]
};
int launch_conv_f16(const ConvParamsH& p, int taps, int mbw, bool pool, hipStream_t s);
// 64 -> 64 3x3 layers with the packed weights resident in LDS (conv_f16_res.hip)
bool conv_f16_res_supports(const ConvParamsH& p, int taps);
int launch_conv_f16_res(const ConvParamsH& p, int mbw, bool pool, hipStream_t s);
void launch_conv_first_f16(const Conv1ParamsH& p, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// heads post-processing
// ---------------------------------------------------------------------------------------------
// logits [B*Hc*Wc][lstride] (65 valid) -> prob [B][Hc*8][Wc*8]  (softmax over 65, drop dustbin,
// depth-to-space 8) and/or logits_nchw [B][65][Hc][Wc]
// fused tail of both heads (head_tail.hip): 1x1 convolutions + BN + softmax/shuffle + L2 normalisation in one launch
struct HeadTailParams {
    const float* x;             // [npx][xstride] output of the 3x3 head convolution: detector channels [0,K), descriptor [K,2K)
    int xstride, K;             // K = head channels (multiple of 32)
    const float *wdet, *bdet, *sdet, *tdet;       // detector 1x1: pack_mfma_weights(taps = 1) fragments, bias / BN scale / shift.
                                                  // The kernel reads entries [0, 96) of bdet / sdet / tdet (three 32-channel blocks for the 65
                                                  // detector channels) and [0, D) of the descriptor arrays: model_load.hip's build_conv pads every
                                                  // per-channel array to nslices * 64 >= 128 entries (zeros / identity BatchNorm)
    const float *wdesc, *bdesc, *sdesc, *tdesc;   // descriptor 1x1 (unused when desc == nullptr)
    int D;                      // descriptor size (64, 128 or 256)
    long long npx;              // B * Hc * Wc
    int B, Hc, Wc;
    float* prob;                // [B][1][8Hc][8Wc] or nullptr
    float* logits_nchw;         // [B][65][Hc][Wc] or nullptr
    float* desc;                // [npx][D] or nullptr
    int softmax_mode;           // 0: Softmax2d, 1: SuperPointMagicLeap heat map
    int normalize;              // F.normalize the descriptors
    int ncu;                    // compute units of the device: one persistent workgroup each
};
int launch_head_tail(const HeadTailParams& p, hipStream_t s);      // 0: launched, 1: shape not covered (use the separate kernels)
// the same for the fp16 path (head_tail_f16.hip): x and the weight fragments are fp16 (conv_f16.hip's packing, taps = 1), the
// biases are the fp16-rounded ones, outputs stay fp32
struct HeadTailParamsH {
    const _Float16* x;          // [npx][xstride] fp16 output of the 3x3 head convolution: detector channels [0,K), descriptor [K,2K)
    int xstride, K;             // K = head channels (multiple of 128: two 64-channel chunks per pass of the double buffer)
    const _Float16 *wdet, *wdesc;
    const float *bdet, *sdet, *tdet, *bdesc, *sdesc, *tdesc;      // padded like HeadTailParams' (>= 96 / D entries)
    int D;
    long long npx;
    int B, Hc, Wc;
    float* prob; float* logits_nchw; float* desc;
    int softmax_mode, normalize, ncu;
};
int launch_head_tail_f16(const HeadTailParamsH& p, hipStream_t s); // 0: launched, 1: shape not covered
void launch_det_post(const float* logits, int lstride, int B, int Hc, int Wc, float* prob,
                     float* logits_nchw, int mode, hipStream_t s);
void launch_det_post_f16(const _Float16* logits, int lstride, int B, int Hc, int Wc, float* prob,
                         float* logits_nchw, int mode, hipStream_t s);
// raw [npx][D] -> out [npx][D] rows divided by max(||row||, 1e-12)   (D multiple of 4, <= 1024)
void launch_desc_l2norm(const float* raw, float* out, long long npx, int D, int normalize,
                        hipStream_t s);
void launch_desc_l2norm_f16(const _Float16* raw, float* out, long long npx, int D, int normalize,
                            hipStream_t s);

// ---------------------------------------------------------------------------------------------
// keypoint extraction
// ---------------------------------------------------------------------------------------------
#define MP_NMS_MAX_R 15  // footprint radius supported by the NMS kernels (box size <= 16: a row of the footprint is one 32-bit mask)
struct NmsFootprint {
    int R;                                   // radius
    unsigned rowmask[2 * MP_NMS_MAX_R + 1];  // bit (dx+R) of rowmask[dy+R] set <=> IoU > thr
};

// work map encoding: > 0 undecided candidate (its score), 0 dead / not a candidate, < 0 kept (-score)
void launch_nms_init(const float* prob, const uint8_t* mask, float min_prob, float* work,
                     long long n, hipStream_t s);
// tie_pairs (optional, int [B]): footprint tie guard -- += candidates that died to kept neighbours within tie_eps of their score only
void launch_nms_round(float* work, int B, int H, int W, const NmsFootprint& fp, int* remaining,
                      int round, hipStream_t s, float tie_eps = 0.f, int* tie_pairs = nullptr);
// W: width of the work map (a multiple of 4), Ws <= W: row stride (true width) of prob / mask
void launch_nms_round0(const float* prob, const uint8_t* mask, float min_prob, float* work, int B, int H, int W,
                       const NmsFootprint& fp, int* remaining, hipStream_t s, int Ws, float tie_eps = 0.f, int* tie_pairs = nullptr);
void launch_nms_accumulate(int* remaining, int B, int H, int W, int round, int* total, hipStream_t s);
// per image: ordered (row-major) list of kept pixels, top-k selection by (score desc, index asc),
// outputs kp_yx [B][K][2] int32, kp_score [B][K], kp_count [B]; optional dense map prob_nms
// Wout <= W: row stride of prob_nms (the caller's true width when the work map's rows are padded to a multiple of 4); kp_yx are
// true coordinates either way.  tie_pairs / pairs_min: the footprint tie guard's per-image counts (nms.hip; read and reset here)
void launch_select_keypoints(const float* work, int B, int H, int W, int topk, int K,
                             int* list_idx, float* list_score, int list_cap, int* kp_yx,
                             float* kp_score, int* kp_count, float* prob_nms, int* seg_scratch, hipStream_t s,
                             float tie_eps = 0.f, int tie_min = 0, int* tie_state = nullptr, int Wout = 0,
                             int* tie_pairs = nullptr, int pairs_min = 0);
// top-k tie guard state (device ints): [0] flagged images since the last read, [1 + b] flag of image b of the latest call
#define MP_TIE_MAX_IMAGES 1000
// ints of device scratch (segment counts + list totals) launch_select_keypoints / launch_extract_threshold need
size_t keypoint_scratch_ints(int B, int H, int W);
// plain threshold extraction: (map > thr) -> row-major list (torch.nonzero semantics)
void launch_extract_threshold(const float* map, const unsigned char* mask, int B, int H, int W, float thr, int K, int* kp_yx,
                              float* kp_score, int* kp_count, int* seg_scratch, hipStream_t s);

// spatially uniform top-k (keypoints_spread.hip): adaptive non-maximal suppression.  radius2 [B][K] uint32 of a keypoint list
// (kp_yx [B][K][2], kp_score [B][K], kp_count [B]): squared distance to the nearest entry j with s_i < robust * s_j (one fp32
// multiply), 0xFFFFFFFF without one; rows beyond min(kp_count[b], K) are not written
void launch_suppression_radii(const int* kp_yx, const float* kp_score, const int* kp_count, int B, int K, float robust,
                              unsigned* radius2, hipStream_t s);
// ... and the selection on the row-major survivor list launch_select_keypoints left behind (list_idx / list_score / list_count;
// list_r2 [B][list_cap] is scratch): the topk entries first by (radius desc, score desc, index asc), outputs as
// launch_select_keypoints' plus kp_radius2 [B][K] (may be NULL).  prob_nms must already be zero.
void launch_select_spread(int B, int H, int W, int topk, int K, const int* list_idx, const float* list_score, unsigned* list_r2,
                          int list_cap, const int* list_count, float robust, int* kp_yx, float* kp_score, unsigned* kp_radius2,
                          int* kp_count, float* prob_nms, int Wout, hipStream_t s);

// sub-pixel keypoints (keypoints_subpixel.hip): a separable log-parabola fit on the detector map around every list entry;
// kp_sub_yx [B][K][2] fp32 (y, x), rows beyond min(kp_count[b], K) zero
void launch_refine_keypoints(const float* prob, int B, int H, int W, const int* kp_yx, const int* kp_count, int K,
                             float* kp_sub_yx, hipStream_t s);

// bilinear sampling (grid_sample align_corners=True, zeros) + L2 normalise.
// desc [B][Hc][Wc][D] channels-last; kp_yx [B][K][2] int pixels or float sub-pixel positions; out [B][K][D]
template <class KP>
void launch_sample_desc(const float* desc, int B, int Hc, int Wc, int D, int H, int W,
                        const KP* kp_yx, const int* kp_count, int K, float* out, hipStream_t s);

// MFMA matchers (match_mfma.hip, unit rows, D in {64, 128, 256}); their scratch holds one array of packed keys per column share
constexpr int MATCH_SHARES = 2;     // column shares of the row passes (mp_match.h: column_share)
// mutual nearest neighbour matching of P pairs; rowbest/colbest: [MATCH_SHARES][P][K] packed scratch each
void launch_match_impl(const float* dA, const int* nA, const float* dB, const int* nB,
                       long long pair_stride, int count_stride, int P, int K, int D, float thr,
                       unsigned long long* rowbest, unsigned long long* colbest, int* match_idx,
                       float* match_dist, int* match_count, hipStream_t s);

// one-directional matching of P pairs on the same tile walk: nearest train row per query (ratio <= 0) or
// Lowe's ratio test on the two nearest (ratio > 0); best2: [MATCH_SHARES][P][K][2] packed scratch; second_* may be NULL
void launch_match_nearest(const float* dA, const int* nA, const float* dB, const int* nB, long long pair_stride,
                          int count_stride, int P, int K, int D, double ratio, unsigned long long* best2, int* match_idx,
                          float* match_dist, int* match_count, int* second_idx, float* second_dist, hipStream_t s);

// mutual nearest neighbours inside a geometric gate (match_guided.hip): a candidate pair (i, j) needs hom[p] to map optical
// keypoint i within `radius` of thermal keypoint j.  kp*_yx rows lie like the descriptor rows (pair p at + p * (pair_stride / D)
// rows); pos: [2][P][K][2] float scratch; rowbest/colbest as for launch_match_impl
void launch_match_guided(const float* dA, const int* nA, const float* dB, const int* nB, long long pair_stride,
                         int count_stride, int P, int K, int D, const int* kpA_yx, const int* kpB_yx, const double* hom,
                         float radius, float thr, float* pos, unsigned long long* rowbest, unsigned long long* colbest,
                         int* match_idx, float* match_dist, int* match_count, hipStream_t s);

// remaining get_matches modes (match_extra.hip): two nearest train rows per query (BFMatcher knnMatch / match without
// crossCheck), idx/dist [P][K][2]; all pairs closer than thr (ThresholdMatcher), list_count [P] pre-set to 0
void launch_match_knn2(const float* dA, const int* nA, const float* dB, const int* nB, long long pair_stride,
                       int count_stride, int P, int K, int D, int* idx, float* dist, hipStream_t s);
void launch_match_threshold(const float* dA, const int* nA, const float* dB, const int* nB, long long pair_stride,
                            int count_stride, int P, int K, int D, float thr, int capacity, int* list_ij,
                            float* list_dist, int* list_count, hipStream_t s);

// GPU-resident pair metrics (evaluation.py:287-328): hom [2P][9] double (slot 2p: optical->thermal ground-truth
// homography, 2p+1: its inverse), warped [2P][K][2] double scratch, inv_idx [P][K] scratch (pre-set to -1),
// tp [2P][K] (pre-set to 0), metrics [P][8] (pre-set to 0): n_gt_o, n_gt_t, matched_o, matched_t, N_o, N_t, n_matches
void launch_pair_metrics(const int* kp_yx, const int* kp_count, const int* match_idx, const double* hom, int P, int K,
                         int H, int W, float thr, double* warped, int* inv_idx, unsigned char* tp, int* metrics,
                         hipStream_t s);
// keypoint repeatability (evaluation.py:156-199): hom [2P][2][9] double (slot b: inverse of its own homography, then the
// other image's homography), warped [2P][K][2] int64 scratch, out [P][4] (pre-set to 0): count1, count2, N_thermal, N_optical
void launch_repeatability(const int* kp_yx, const int* kp_count, const double* hom, int P, int K, int H, int W, double thr,
                          long long* warped, int* out, hipStream_t s);
// batched RANSAC homography (predict_align_image_pair.py:205-216): best [P] scratch (pre-set to 0), H_out [P][9] double
// (x,y) optical -> (x,y) thermal, mask [P][K] uint8 per optical keypoint (pre-set to 0), n_inliers [P]
// KP (here and in the two launchers below): int for pixel keypoints, float for sub-pixel ones
template <class KP>
void launch_ransac_homography(const KP* kp_yx, const int* kp_count, const int* match_idx, int P, int K, int T, double thr,
                              unsigned long long seed, unsigned long long* best, double* H_out, unsigned char* mask,
                              int* n_inliers, hipStream_t s);

// Levenberg-Marquardt polish of hom [P][9] (in: estimate, out: polished, h22 = 1) over the matches within thr of the estimate;
// mask [P][K] zeroed by the caller, cost [P][2] (before / after) or NULL
template <class KP>
void launch_refine_homography(const KP* kp_yx, const int* kp_count, const int* match_idx, int P, int K, double thr, int iters,
                              double* H_io, unsigned char* mask, int* n_inliers, double* cost, hipStream_t s);

// pooled RANSAC homography (homography_pooled.hip): one model per group of pairs from their compacted matches
constexpr int MP_POOLED_CHUNK = 1024;        // points per staged LDS chunk of the scoring kernel
constexpr int MP_POOLED_MAX_SPLITS = 64;     // most workgroups that share the points of one (hypothesis block, group)
// pts [capacity][4] fp32 (16-byte aligned) / query_index [capacity]: the usable matches of all pairs, pair-major in query order;
// pair_offsets [P + 1], group_offsets [G + 1] (groups: device [P] non-decreasing ids or NULL = one group); pair_cnt [P] scratch
template <class KP>
void launch_pool_matches(const KP* kp_yx, const int* kp_count, const int* match_idx, const int* groups, int P, int K, int G,
                         float* pts, int* query_index, long long capacity, int* pair_offsets, int* group_offsets, int* pair_cnt,
                         hipStream_t s);
// counts [G][T] and mask [N] pre-set to 0; best [G] scratch; H_out [G][9], n_inliers [G]
void launch_find_homography_pooled(const float* pts, const int* group_offsets, int N, int G, int T, double thr,
                                   unsigned long long seed, unsigned int* counts, unsigned long long* best, double* H_out,
                                   unsigned char* mask, int* n_inliers, hipStream_t s);
// mask [N] pre-set to 0; cost [G][2] or NULL
void launch_refine_homography_pooled(const float* pts, const int* group_offsets, int N, int G, double thr, int iters, double* H_io,
                                     unsigned char* mask, int* n_inliers, double* cost, hipStream_t s);

// best [G] = the winning (count << 32) | (0x7fffffff - t) of counts [G][T] (the selection step of the pooled estimators)
void launch_pooled_select(const unsigned int* counts, int T, int G, unsigned long long* best, hipStream_t s);

// similarity / affine estimation (transform.hip, transform_f.hip, transform_pooled.hip): the homography launchers' arguments
// and buffers plus `model`, MP_MODEL_SIMILARITY or MP_MODEL_AFFINE (the C entries forward MP_MODEL_HOMOGRAPHY to the
// launchers above); `rounds` of local optimisation in the place of the polish's `iters`
template <class KP>
void launch_find_transform(int model, const KP* kp_yx, const int* kp_count, const int* match_idx, int P, int K, int T, double thr,
                           unsigned long long seed, unsigned long long* best, double* H_out, unsigned char* mask, int* n_inliers,
                           hipStream_t s);
template <class KP>
void launch_refine_transform(int model, const KP* kp_yx, const int* kp_count, const int* match_idx, int P, int K, double thr,
                             int rounds, double* H_io, unsigned char* mask, int* n_inliers, double* cost, hipStream_t s);
void launch_find_transform_pooled(int model, const float* pts, const int* group_offsets, int N, int G, int T, double thr,
                                  unsigned long long seed, unsigned int* counts, unsigned long long* best, double* H_out,
                                  unsigned char* mask, int* n_inliers, hipStream_t s);
void launch_refine_transform_pooled(int model, const float* pts, const int* group_offsets, int N, int G, double thr, int rounds,
                                    double* H_io, unsigned char* mask, int* n_inliers, double* cost, hipStream_t s);

// single-image detector metrics (detector_metrics.hip; evaluation.py:56-97): best [B][H][W] scratch, rec_count / n_gt [B]
// (all three pre-set to 0), records [B][H*W]
void launch_detector_metrics(const float* prob, const unsigned char* gt, int B, int H, int W, float zero_thr,
                             float distance_thr, unsigned long long* best, int* rec_index, float* rec_prob,
                             unsigned* rec_bits, int* rec_count, int* n_gt, hipStream_t s);

// homographic adaptation (homog_adapt.hip; reference multipoint/utils/homographies.py:38-189, 361-433).
// hom arrays are device double [n][9], row-major 3x3 acting on pixel (x, y, 1).
// warp: dst[n](x, y) = src[n % n_src] sampled at hom[n] * (x, y, 1); mode 0 bilinear / 1 nearest, padding 0 zeros / 1 reflection
void launch_warp_perspective(const float* src, int n_src, int H, int W, const double* hom, int n_out, int Ho, int Wo,
                             int mode, int padding, float* dst, hipStream_t s);
void launch_cv_warp_linear(const float* src, int n, int H, int W, const double* hom_inv, int border, float* dst,
                           hipStream_t s);
void launch_ha_valid_mask(const double* hom_inv, int G, int H, int W, int r, int mask_border, unsigned char* mask,
                          hipStream_t s);
void launch_ha_begin(const float* pa, const float* pb, long long n, int aggregation, float* prob, float* count,
                     hipStream_t s);
void launch_ha_accumulate(const float* pa, const float* pb, const unsigned char* mask, const double* hom, int G, int B,
                          int H, int W, int aggregation, float* prob, float* count, hipStream_t s);
void launch_ha_finalize(const float* prob, const float* count, long long n, int aggregation, float min_count, float* out,
                        hipStream_t s);
void launch_gaussian_filter(const float* in, int B, int H, int W, int k, const float* wgt, float* out, hipStream_t s);

// SuperPointLoss evaluation (losses.hip; reference multipoint/utils/losses.py:85-122, 207-272).  Label / mask maps uint8
// [B][H][W] (nonzero = set), logits fp32 [B][65][Hc][Wc], descriptors channels-last fp32 [B][Hc*Wc][D], homographies fp32
// [B][9].  `workspace` holds loss_workspace_bytes(B, H, W) bytes.
//   detector:   noise fp32 [B][64][Hc][Wc] or NULL (hash of (seed, b, c, h, w)); out double [B][2]: sum of loss * valid, count
//   descriptor: s_max = largest float s with sqrt_rn(s) <= threshold; out double [B][4]: lambda_d * positive sum, negative
//               sum, corresponding valid pairs, normalisation; warped fp32 [2][B][Hc*Wc][2] (y, x) or NULL
size_t loss_workspace_bytes(int B, int H, int W);
void launch_detector_loss(const float* logits, const unsigned char* kp, const unsigned char* valid, const float* noise,
                          unsigned long long seed, int B, int H, int W, int use_ce, void* workspace, double* out,
                          hipStream_t s);
void launch_descriptor_loss(const float* desc1, const float* desc2, const float* hom1, const float* hom2,
                            const unsigned char* valid1, const unsigned char* valid2, int B, int H, int W, int D,
                            float s_max, float pos_margin, float neg_margin, double lambda_d, int use_mask,
                            void* workspace, double* out, float* warped, hipStream_t s);
// backward: fwd_out the forward's out array of the same call; coef device doubles, the upstream coefficients
//   detector:   coef[0] = gamma; grad fp32 [B][65][Hc][Wc]
//   descriptor: coef[0] = alpha (positive terms), coef[1] = beta (negative terms); grad1 / grad2 channels-last fp32
//               [B][Hc*Wc][D], either may be NULL (that side is skipped); recomputes the prologue into the workspace
void launch_detector_loss_backward(const float* logits, const unsigned char* kp, const unsigned char* valid,
                                   const float* noise, unsigned long long seed, int B, int H, int W, int use_ce,
                                   const double* fwd_out, const double* coef, float* grad, hipStream_t s);
void launch_descriptor_loss_backward(const float* desc1, const float* desc2, const float* hom1, const float* hom2,
                                     const unsigned char* valid1, const unsigned char* valid2, int B, int H, int W, int D,
                                     float s_max, float pos_margin, float neg_margin, float lambda_d, int use_mask,
                                     const double* fwd_out, const double* coef, void* workspace, float* grad1,
                                     float* grad2, hipStream_t s);

// BatchNorm2d with the statistics of the batch (batchnorm_stats.hip).  Activations NHWC fp32 [npx][cstride], C (a multiple of 4,
// 8..1024) channels per pixel; part: double [bn_stats_parts(npx, C)][2][C] scratch (at most MP_BN_MAX_PARTS slots)
#define MP_BN_MAX_PARTS 2048
int bn_stats_parts(long long npx, int C);
// images [*][H][W] -> out [nb][H][W]: image list[b] to place b (H * W a multiple of 4)
void launch_bn_gather(const float* img, const int* list, int nb, int H, int W, float* out, hipStream_t s);
void launch_bn_stats(const float* x, long long npx, int C, int cstride, double* part, hipStream_t s);
// channels [c0, c0 + nc) of the launch's C: scale / shift [C] (indexed by the tensor channel), gamma / beta / mean_out / var_out
// indexed from c0; channels c0 + c with c >= c_real are padding (scale = shift = 0).  mean_out / var_out may be NULL
void launch_bn_finalize(const double* part, long long npx, int C, const float* x, int c0, int nc, int c_real, const float* gamma,
                        const float* beta, float* scale, float* shift, float* mean_out, float* var_out, hipStream_t s);
// x [B][H][W][C] -> y [B][H or H/2][W or W/2][C], image b to out_list[b] (NULL: b); x == y allowed without pool and list
void launch_bn_apply(const float* x, float* y, int B, int H, int W, int C, const float* scale, const float* shift, bool relu,
                     bool pool, const int* out_list, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// photometric augmentation (photometric.hip).  plans / ellipses are host arrays (copied into the workspace on the
// stream); `workspace` holds photometric_workspace_bytes(n, H, W, n_ellipses) bytes.
// ---------------------------------------------------------------------------------------------
struct mp_photometric_plan;
size_t photometric_workspace_bytes(int n, int H, int W, int n_ellipses);
size_t photometric_lds_bytes(const mp_photometric_plan* plans, int n, int H, int W);
void launch_photometric(const float* in, float* out, int n, int H, int W, const mp_photometric_plan* plans,
                        const int* ellipses, int n_ellipses, const double* normal, const double* uniform, void* workspace,
                        hipStream_t s);
// cv2.GaussianBlur(frame, (k, k), 0) of n fp32 frames in place with ksizes[img] (device array; 0: frame left alone), the
// sepFilter2D restatement of the shade masks: weights [n][MP_PHOTO_MAX_BLUR] and tmp [n][H][W] are device scratch, kmax the
// largest size (host); the caller checks gaussian_blur_lds_bytes(kmax, W) against the device limit
size_t gaussian_blur_lds_bytes(int k, int W);
void launch_gaussian_blur_frames(float* img, float* tmp, float* weights, const int* ksizes, int kmax, int n, int H, int W,
                                 hipStream_t s);
void launch_photometric_shade_mask(int n, int H, int W, const mp_photometric_plan* plans, const int* ellipses,
                                   int n_ellipses, int op_index, int blurred, float* out, void* workspace, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// mutual-information alignment (mutual_info.hip; reference create_dataset/helper_functions/align.py:13-215).
// An evaluation is (pair, bins, transform); its n x 2n counters start at counts + off.  G consecutive evaluations form a
// group of which the first nact[group] run (nact NULL: all of them): the candidate slots of one Nelder-Mead problem.
// ---------------------------------------------------------------------------------------------
#define MI_PARTS 16            // row blocks of the score's first pass
#define MI_MAX_RADIUS 64       // of the smoothing kernel: int(4 sigma + 0.5)
#define MI_SLOTS 10            // candidate slots of a Nelder-Mead problem: the 9 + 1 vertices of its largest simplex
#define MI_PARAMS_MAX 9        // parameters of the largest motion model (the homography's nine entries)
struct MiEval { int pair, bins, tslot, pad; long long off; };
struct MiNmOptions { int maxiter, maxfun; double xatol, fatol; };
// a simplex of n + 1 vertices over the n parameters of the refinement's motion model: rows and columns beyond stay unused
struct MiNmState {
    double sim[MI_SLOTS][MI_PARAMS_MAX], fsim[MI_SLOTS];
    MiNmOptions opt;
    int iterations, fcalls, phase, done, status, pad;
};
struct MiLaunch {
    const float* optical;      // [B][Ho][Wo]
    int Ho, Wo, H, W, E, G;
    int lds_bins;              // largest bin count <= 64 among the evaluations (0: none): sizes hist_kernel's LDS
    const MiEval* ev;          // [E]
    const int* nact;           // [E / G] or NULL
    const double* T;           // [E][9]
    double* M;                 // [E][9]: cv_invert3(cv_invert3(T))
    unsigned* keys;            // [E][2]: ordered keys of the warped frame's min / max
    const unsigned short* tmap;   // [S][H W]: thermal bins per distinct (pair, bins)
    double *part, *rowsum, *colpart;   // [E][MI_PARTS], [E][256], [E][MI_PARTS][512]
};
// tkeys [B][2], tmap [S][H W] for the S slots (pair, bins)
void launch_mi_thermal(const float* thermal, int B, int HW, const int2* slots, int S, unsigned* tkeys, unsigned short* tmap,
                       hipStream_t s);
// counts (zeroed here), warped [E][H][W]; minmax [E][2] or NULL; strategy 0 by bin count, 1 LDS copies, 2 global atomics
void launch_mi_histograms(const MiLaunch& L, unsigned* counts, float* warped, float* minmax, int strategy, hipStream_t s);
// values [E] = -MI (+ |Tinit[e / tg] - T[e]|_F when Tinit); smooth_a / smooth_b [E][smooth_stride] doubles when sigma > 0
void launch_mi_score(const MiLaunch& L, const unsigned* counts, double sigma, int normalized, const double* Tinit, int tg,
                     long long smooth_stride, double* smooth_a, double* smooth_b, double* values, hipStream_t s);
// The motion model of a refinement (MP_MODEL_*): n parameters per point (mi_model_params: 9, 4 or 6; 0 for an unknown
// model) and the map from a parameter vector to the 3x3 matrix the objective reads.  A problem's candidate points lie in
// candp [P][MI_SLOTS][MI_PARAMS_MAX] (n used per row); their matrices in cand [P][MI_SLOTS][9], which is MiLaunch::T.
int mi_model_params(int model);
// transforms [rows][9] = map(params [rows][n])
void launch_mi_model_transform(int model, const double* params, int rows, double* transforms, hipStream_t s);
// x0 [P][n]: the start parameters; tinit [P][9] receives their matrices (what the regulariser measures from)
void launch_mi_nm_begin(MiNmState* state, const MiNmOptions* opt, int model, const double* x0, int P, double* candp, double* cand,
                        double* tinit, int* nact, hipStream_t s);
void launch_mi_nm_decide(MiNmState* state, int model, int P, double* candp, double* cand, const double* values, int* nact,
                         int* live, hipStream_t s);
// T [P][9]: the matrix of the best vertex; params [P][n]: the vertex itself, or NULL
void launch_mi_nm_result(const MiNmState* state, int model, int P, double* T, double* params, double* value, int* iterations,
                         int* fcalls, int* success, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// 2-D FFT (fft.hip) and the LGHD baseline (lghd.hip; reference multipoint/models/ClassicDetectors.py, class LGHD).
// Complex arrays are interleaved fp32 (re, im).  tw_rows / tw_cols: the tables fft_twiddles() fills for W and H, on the device.
// ---------------------------------------------------------------------------------------------
void fft_twiddles(int n, float* table);       // host: table [n][2] = exp(-2 pi i t / n), computed in double and rounded once
// axes: 1 rows (length W), 2 columns (length H), 3 both; in == out allowed
void launch_fft2d(const float* in, float* out, int planes, int H, int W, int inverse, int axes, const float* tw_rows,
                  const float* tw_cols, hipStream_t s);
// orientation u8 [nb][4][H][W]; spectrum: nb complex frames, tmp: nb * 24 complex frames
void launch_lghd_orientation(const unsigned char* u8, const float* bank, int nb, int H, int W, float* spectrum, float* tmp,
                             unsigned char* orientation, const float* tw_rows, const float* tw_cols, hipStream_t s);
void launch_lghd_quantize(const float* image, unsigned char* u8, long long n, hipStream_t s);
// score / corners u8 [B][H][W], prob fp32 [B][H][W] or NULL
void launch_lghd_detect(const unsigned char* u8, int B, int H, int W, unsigned char* score, unsigned char* corners, float* prob,
                        hipStream_t s);
// raw / unit fp32 [B][K][384], either may be NULL
void launch_lghd_describe(const unsigned char* ori, int B, int H, int W, const int* kp_yx, const int* kp_count, int K, float* raw,
                          float* unit, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// The RIFT baseline (fft.hip, rift.hip, lghd.hip).
// ---------------------------------------------------------------------------------------------
// FAST-9/16 of lghd.hip with its threshold and validity border as arguments; scored: prob = score / 255 instead of 1
void launch_fast_detect(const unsigned char* u8, int B, int H, int W, int threshold, int half, int scored, unsigned char* score,
                        unsigned char* corners, float* prob, hipStream_t s);
// M, m fp32 and mim u8 [nb][H][W], T fp32 [nb][6]; spectrum: nb complex frames, tmp: nb * 24 complex frames, amp: nb * 6 real frames
void launch_rift_phase_congruency(const unsigned char* u8, const float* bank, int nb, int H, int W, float k, float g, float cutoff,
                                  float* spectrum, float* tmp, float* amp, float* T, float* M, float* m, unsigned char* mim,
                                  const float* tw_rows, const float* tw_cols, hipStream_t s);
// T[p] from the exact median of amp[p][0 .. HW), p < planes
void launch_rift_noise_threshold(const float* amp, int planes, long long HW, float k, float* T, hipStream_t s);
// u8m [B][H][W] from M, range fp32 [B][2] = (min, max) of M, then FAST on u8m
void launch_rift_detect(const float* M, int B, int H, int W, int threshold, int patch, unsigned char* u8m, float* range,
                        unsigned char* score, unsigned char* corners, float* prob, hipStream_t s);
// raw / unit fp32 [B][K][256]: 216 counts of the 6 x 6 cells of patch / 6 pixels, then zeros; either may be NULL
void launch_rift_describe(const unsigned char* mim, int B, int H, int W, int patch, const int* kp_yx, const int* kp_count, int K,
                          float* raw, float* unit, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Fourier-Mellin registration (register.hip).  Complex planes are interleaved fp32, as the FFT takes them.
// ---------------------------------------------------------------------------------------------
#define MP_REGISTER_PEAK_CHUNK 16384      // plane values one workgroup of the peak search reduces
// frames [n][H][W] -> out complex [n][N][N]; cs [n][2] or NULL; wy [H], wx [W]
void launch_register_prepare(const float* frames, const float* cs, const float* wy, const float* wx, int n, int H, int W, int N,
                             float* out, hipStream_t s);
// spectrum complex [n][N][N] -> out complex [n][A][R]; ca, sa [A]; rho, wr [R]
void launch_register_logpolar(const float* spectrum, int n, int N, const float* ca, const float* sa, const float* rho,
                              const float* wr, int A, int R, float* out, hipStream_t s);
// a, b complex [P][h][w], group_offsets [G+1] -> out complex [G][h][w] (accumulate: the sums start from out)
void launch_register_cross_power(const float* a, const float* b, const int* group_offsets, int P, int G, int h, int w,
                                 int accumulate, float* out, hipStream_t s);
// the chunks' results in the caller's workspace: carved from `partial`, or from nullptr for the bytes a call needs
struct RegisterPeakWorkspace { float* part_v; int* part_i; int chunks; size_t bytes; };
RegisterPeakWorkspace register_peak_workspace(void* partial, int G, int h, int w);
// planes [G][h][w] values `stride` floats apart -> out_i [G][2], out_f [G][6]; partial: G * chunks (float, int) pairs
void launch_register_peak(const float* planes, int G, int h, int w, int stride, int* out_i, float* out_f, void* partial,
                          hipStream_t s);

// ---------------------------------------------------------------------------------------------
// ECC direct alignment (ecc.hip): Gauss-Newton maximisation of the enhanced correlation coefficient.
// ---------------------------------------------------------------------------------------------
#define MP_ECC_CHUNK 4096                 // template pixels one workgroup of the sums pass reduces
#define MP_ECC_MAX_SUMS 66                // 6 + K + K (K + 1) / 2 + 2 K at K = 8
#define MP_ECC_RUNNING (-1)               // EccState::status of a problem whose iterations go on
// one problem of a running refinement
struct EccState {
    double T[9];                          // the current iterate (T22 == 1)
    double rho, rho_prev;                 // the correlation at T, and at the iterate before (NaN: none)
    int pair, nit, status, converged;     // status: MP_ECC_RUNNING or an MP_ECC_* result code
};
struct EccOptions { double eps, min_valid; int maxiter, pad; };
// parameters of a motion model (MP_MODEL_*): 8, 4, 6, 2; 0 for an unknown one.  ecc_sum_count: the sums of one problem
int ecc_model_params(int model);
int ecc_sum_count(int K);
int ecc_chunks(int H, int W);
// blurred [n][H][W] -> feat [n][H][W] (gradient != 0: the magnitude of the central differences, else a copy)
void launch_ecc_feature(const float* blurred, int n, int H, int W, int gradient, float* feat, hipStream_t s);
// feat [n][H][W] -> packed [n][H][W][4]: (f, gx, gy, 0)
void launch_ecc_pack(const float* feat, int n, int H, int W, float* packed, hipStream_t s);
// One sums pass: partial [P][chunks][sums].  T != NULL: the transforms [P][9] and pair [P] of a diagnostic call; else those of
// `state`, whose finished problems are skipped.
void launch_ecc_sums(int K, const float* packed, int Ho, int Wo, const float* thermal, int H, int W, const int* pair,
                     const double* T, const EccState* state, int P, double* partial, hipStream_t s);
// partial [P][chunks][sums] -> sums [P][sums], added in chunk order
void launch_ecc_reduce(int K, const double* partial, int P, int chunks, double* sums, hipStream_t s);
void launch_ecc_begin(const int* pair, const double* T0, int P, EccState* state, hipStream_t s);
// one Gauss-Newton decision per running problem from its partial sums
void launch_ecc_solve(int K, const double* partial, int P, int chunks, int HW, EccOptions o, EccState* state, hipStream_t s);
void launch_ecc_live(const EccState* state, int P, int* live, hipStream_t s);
void launch_ecc_result(const EccState* state, int P, double* T, double* rho, int* nit, int* status, int* converged, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Pooled ECC (ecc_pooled.hip): one transform per group of pairs, static masks.
// ---------------------------------------------------------------------------------------------
#define MP_ECC_POOLED_MAX_Q 55            // centred quantities of one pair: ww, rr, corr, A (K (K + 1) / 2), ip (K), tp (K) at K = 8
// one group of a running pooled refinement
struct EccGroup {
    EccState s;                           // the group's iterate and stop state (s.pair: the group's index)
    int M;                                // template pixels the group's thermal mask keeps (H W without one)
    int n_included;                       // pairs included at the latest evaluation
};
// one pair at the latest evaluation of its group
struct EccPairRec { double rho, n; int included, pad; };
// use-masks in [n][H][W] (nonzero: use) -> out: 0 within Chebyshev distance R of a zero of `in`, else 1; tmp [n][H][W]
void launch_ecc_mask_grow(const unsigned char* in, int n, int H, int W, int R, unsigned char* tmp, unsigned char* out, hipStream_t s);
// running minimum and maximum per pixel over frames [n][HW]; first != 0 starts them from the first frame
void launch_ecc_static_update(const float* frames, int n, int HW, int first, float* lo, float* hi, hipStream_t s);
// mask = lo == hi ? 0 : 1
void launch_ecc_static_finish(const float* lo, const float* hi, int HW, unsigned char* mask, hipStream_t s);
// packed [n][HW][4]: .w = 1.0f where mask [HW] is 0 (the same mask for the n frames)
void launch_ecc_flag_packed(float* packed, int n, int HW, const unsigned char* mask, hipStream_t s);
// One pooled sums pass: partial [P][chunks][sums] of pair p at the transform of its group.  T != NULL: the transforms [G][9] of a
// diagnostic call; else those of `groups`, whose finished groups and inactive pairs are skipped.  tmasks [.][H][W] use-masks of
// the template, tmask [G] the plane of every group (-1: none).
void launch_ecc_pooled_sums(int K, const float* packed, int Ho, int Wo, const float* thermal, int H, int W,
                            const unsigned char* tmasks, const int* tmask, const int* group, const int* active, const double* T,
                            const EccGroup* groups, int P, double* partial, hipStream_t s);
void launch_ecc_pooled_begin(const double* T0, const unsigned char* tmasks, const int* tmask, int HW, int G, int P, EccGroup* groups,
                             EccPairRec* recs, hipStream_t s);
// per pair: the chunks added in order, the centred quantities quant [P][MP_ECC_POOLED_MAX_Q], the inclusion decision, recs
void launch_ecc_pooled_pair(int K, const double* partial, int P, int chunks, const int* group, const int* active, EccOptions o,
                            const EccGroup* groups, EccPairRec* recs, double* quant, hipStream_t s);
// per group: the included pairs' quantities added in list order (offsets [G + 1], list [P]), then the decision of 3.21
void launch_ecc_pooled_solve(int K, const int* offsets, const int* list, const EccPairRec* recs, const double* quant, int G,
                             EccOptions o, EccGroup* groups, hipStream_t s);
void launch_ecc_pooled_live(const EccGroup* groups, int G, int* live, hipStream_t s);
void launch_ecc_pooled_result(const EccGroup* groups, int G, const EccPairRec* recs, int P, double* T, double* rho, int* nit,
                              int* status, int* converged, int* n_included, double* rho_pair, double* n_pair, int* included,
                              hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Local residual field (residual.hip): windowed zero-mean normalised cross-correlation of two feature frames.
// ---------------------------------------------------------------------------------------------
// status of a window (include/multipoint_hip.h repeats them for the callers)
#define MP_RES_OK 0                       // a best displacement inside the search border
#define MP_RES_FEW_VALID 1                // the mask leaves displacement 0 fewer than min_valid w^2 pixels
#define MP_RES_FLAT 2                     // no displacement has a defined score
#define MP_RES_AT_EDGE 3                  // a best displacement that touches the search border on some axis
#define MP_RES_MAX_RADIUS 8
struct ResidualParams {
    const float* fo;                      // [B][H][W] optical feature frames (the search side)
    const float* ft;                      // [B][H][W] thermal feature frames (the template side)
    const unsigned char* mask;            // [mask_frames][H][W] on the optical side, nonzero = use, or NULL
    int mask_frames;                      // 1: one plane for every frame, else B
    int H, W, w, s, r, gy, gx;            // window edge, stride, search radius, windows per column / row
    double min_valid, var_floor;
    double* out_d;                        // [B][gy gx][5]: dy, dx, rho, rho0, second
    int* out_i;                           // [B][gy gx][2]: n, status
};
size_t residual_lds_bytes(int w, int r);
void launch_residual_field(const ResidualParams& p, int B, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Local alignment correction (field.hip): a smooth displacement field fitted to a lattice of measured
// displacements, and frames sampled through such a field.
// ---------------------------------------------------------------------------------------------
// status of a fitted frame (include/multipoint_hip.h repeats them for the callers)
#define MP_FIELD_OK 0                     // the last solve met its stopping rule
#define MP_FIELD_NO_DATA 1                // no node has a positive weight: u = 0
#define MP_FIELD_ALL_REJECTED 2           // a robust round left no weight: the solution before it is kept
#define MP_FIELD_MAX_ITER 3               // the last solve ended at max_iter
#define MP_FIELD_MAX_SIDE 256
#define MP_FIELD_MAX_ROUNDS 16
#define MP_FIELD_INFO_INTS 4              // status, iterations of the last solve, nodes with a non-zero final weight, non-finite d
#define MP_FIELD_WS_DOUBLES 7             // per node of the workspace: the weight, and r, p, A p of both axes
struct FieldFitParams {
    const double* d;                      // [B][gy][gx][2]
    const double* weight;                 // [B][gy][gx]
    double* ws;                           // [B][MP_FIELD_WS_DOUBLES gy gx]
    double* out_u;                        // [B][gy][gx][2]
    int* out_info;                        // [B][MP_FIELD_INFO_INTS]
    double* out_res;                      // [B]: the last solve's final relative residual, the larger of the two axes
    double* out_w;                        // [B][gy][gx] the final weights, or NULL
    int gy, gx, rounds, max_iter, p_in_lds;
    double lambda, robust_px, tol;
};
size_t field_fit_lds_bytes(int nodes);    // 0: the search direction does not fit and stays in the workspace
hipError_t launch_field_fit(const FieldFitParams& p, int B, hipStream_t s);   // an error: the LDS attribute was refused, nothing launched

struct FieldWarpParams {
    const float* src;                     // [n_src][Hs][Ws]
    const double* u;                      // [B][gy][gx][2]
    const double* hom;                    // [B][9] or NULL
    float* dst;                           // [B][H][W]
    unsigned char* valid;                 // [B][H][W] or NULL
    int n_src, Hs, Ws, H, W, gy, gx, extrapolate;
    double y0, x0, step;
};
void launch_field_warp(const FieldWarpParams& p, int B, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// Frame preparation (frames.hip; reference create_dataset/extract_images.py:167-242).
// ---------------------------------------------------------------------------------------------
struct FramesCamera {
    double fx, fy, cx, cy;          // K of the source frame
    double k1, k2, p1, p2, k3;      // radial-tangential distortion
    double nfx, nfy, ncx, ncy;      // K_new of the destination frame
};
// np.percentile's linear method on H W values: the ranks the 1 % and the 99 % bound interpolate between and their weights
struct FramesRanks {
    long long rank[4];              // lower previous / next, upper previous / next
    double gamma[2];
};
// src / dst: uint8 [n][H][W][3] (u16 = 0) or uint16 [n][H][W] (u16 = 1); dst 4-byte aligned, not src
void launch_undistort(const void* src, int u16, int n, int H, int W, const FramesCamera& cam, int rotate180, void* dst, hipStream_t s);
void launch_resize_bgr8(const unsigned char* src, int n, int H, int W, int oh, int ow, unsigned char* dst, hipStream_t s);
size_t thermal_rescale_workspace_bytes(int n);
// workspace: thermal_rescale_workspace_bytes(n) zeroed bytes on s; clipped (may be `in`) and saved may be NULL
void launch_thermal_rescale(const unsigned short* in, int n, int H, int W, const FramesRanks& rk, unsigned short* clipped,
                            float* rescaled, unsigned short* saved, void* workspace, hipStream_t s);

// ---------------------------------------------------------------------------------------------
// SIFT baseline (sift.hip; Lowe 2004 with the constants of opencv-contrib 4.2's sift.cpp).  Every buffer lies
// in one caller-provided workspace; SiftLayout says where (sift_api.hip: sift_layout()).
// ---------------------------------------------------------------------------------------------
#define MP_SIFT_MAX_OCTAVES 16
#define MP_SIFT_LAYERS 6           // Gaussian layers per octave (nOctaveLayers + 3); 5 difference layers
#define MP_SIFT_MAX_TAPS 27        // widest Gaussian of the chain: round(8 sigma + 1) | 1 at sigma = 3.09
#define MP_SIFT_MAX_ORI 18         // strict peaks of a circular 36-bin histogram
#define MP_SIFT_BORDER 5
#define MP_SIFT_FLAG_CANDIDATES 1  // flags: more candidates than the capacity (dropped from the end)
#define MP_SIFT_FLAG_KEYPOINTS 2   // ... more oriented keypoints than the capacity
struct SiftLayout {
    int B, H, W, noct, cap;
    int h[MP_SIFT_MAX_OCTAVES], w[MP_SIFT_MAX_OCTAVES];
    long long gauss[MP_SIFT_MAX_OCTAVES];      // float offset of [B][6][h][w]
    long long dog[MP_SIFT_MAX_OCTAVES];        // float offset of [B][5][h][w]
    long long flat[MP_SIFT_MAX_OCTAVES + 1];   // candidate positions (3 layers x h x w) of the octaves before o
    long long tmp;                             // float offset of [B][2H][2W]: the row pass of a blur
    int nblk;                                  // candidate workgroups per image (1024 positions each)
    // byte offsets
    long long cmask, seg_count, seg_base, cand, cand_count, crec, cn, cang, cinfo, list, list_count, dup, bytes;
};
struct SiftTaps { int n; float w[MP_SIFT_MAX_TAPS]; };
// the Gaussian and difference pyramids of u8 [B][H][W]
void launch_sift_scale_space(const unsigned char* u8, const SiftLayout& L, void* ws, hipStream_t s);
// candidates -> refinement + orientation -> ordered list [B][cap][6] (doubled-base coordinates) in the workspace; flags |= MP_SIFT_FLAG_*
void launch_sift_detect(const SiftLayout& L, void* ws, int* flags, hipStream_t s);
// records [B][M][6] -> duplicates removed, the nfeatures largest responses in list order, x / y / size halved: keypoints [B][N][6]
// (rows beyond count zero); dup: B * M bytes of scratch
void launch_sift_select(const float* records, const int* rec_count, int B, int M, int nfeatures, int N, float* keypoints,
                        int* count, unsigned char* dup, hipStream_t s);
void launch_sift_describe(const SiftLayout& L, const void* ws, const float* keypoints, const int* count, int N, float* desc,
                          hipStream_t s);
void launch_sift_scatter(const float* keypoints, const int* count, int B, int N, int H, int W, float* prob, int* owner,
                         hipStream_t s);
