// fp16 vector types and the activation shared by the fp16 kernels (conv_f16.hip, conv_f16_res.hip, head_tail_f16.hip,
// heads_post.hip).  Internal header.
#pragma once
#include "mp_common.h"

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));

// conv result pair (fp32 accumulators) -> activation as autocast produces it: fp16(acc + bias); ReLU; the BatchNorm affine in
// fp32 on the fp16 value -> fp16 (BNF: BatchNorm first, then ReLU).  Written on a pair so that hipcc emits packed instructions
// (v_pk_add_f32, v_cvt_pk_f16_f32, v_pk_max_f16, v_pk_fma_f32): ReLU commutes with the rounding, so it runs on the packed halves
template <bool RELU, bool BNF>
__device__ __forceinline__ h2 act_h2(float a0, float a1, f32x2 bias, f32x2 scale, f32x2 shift)
{
    const f32x2 x = f32x2{a0, a1} + bias;
    h2 h = __builtin_convertvector(x, h2);
    const h2 zero = {0, 0};
    if (RELU && !BNF) h = __builtin_elementwise_max(h, zero);
    f32x2 y = __builtin_convertvector(h, f32x2) * scale + shift;
    asm volatile("" : "+v"(y));      // y exists as an fp32 pair (autocast: BatchNorm result in fp32, THEN fp16): no v_fma_mixlo_f16, which rounds once
    h2 o = __builtin_convertvector(y, h2);
    if (RELU && BNF) o = __builtin_elementwise_max(o, zero);
    return o;
}
