// Sub-pixel keypoint positions (mp_refine_keypoints; an extension -- the reference keeps torch.nonzero's integer pixels): a
// separable log-parabola fit on the detector map around every entry of a keypoint list.
// Per axis, with p0 = prob[y][x], p-, p+ its two neighbours on that axis and l = logf(p):
//     den = l- - 2 l0 + l+,      delta = 0.5 (l- - l+) / den
// The axis is refined only if both neighbours lie inside the frame, all three values are finite and > 0, p0 >= p-, p0 >= p+ and
// den < 0; those conditions give |delta| <= 0.5.  Otherwise delta = 0 and the output is exactly (float)y / (float)x.  The fit
// is exact for an isotropic Gaussian peak of any width (its log is a parabola on each axis), where a window centroid is biased
// by the window's cut.
// One thread per list slot: five scattered loads, three of them shared between the axes.  Rows k >= min(kp_count[b], K) are
// written as zeros, so the output is always fully written.  Any H x W.
#include "mp_common.h"

namespace {

__device__ __forceinline__ bool usable(float p) { return p > 0.f && p < __builtin_inff(); }      // finite and positive (NaN: false)

// the vertex offset of the parabola through (-1, log pm), (0, log p0), (1, log pp), or 0 where the axis is not refined
__device__ __forceinline__ float parabola_offset(bool inside, float pm, float p0, float pp)
{
    if (!inside || !usable(pm) || !usable(p0) || !usable(pp) || !(p0 >= pm) || !(p0 >= pp)) return 0.f;
    const float lm = logf(pm), l0 = logf(p0), lp = logf(pp);
    const float den = lm - 2.f * l0 + lp;
    if (!(den < 0.f)) return 0.f;
    return 0.5f * (lm - lp) / den;
}

__global__ __launch_bounds__(256) void refine_keypoints_kernel(const float* __restrict__ prob, int B, int H, int W,
                                                              const int* __restrict__ kp_yx, const int* __restrict__ kp_count, int K,
                                                              float* __restrict__ kp_sub_yx)
{
    const long long slot = (long long)blockIdx.x * 256 + threadIdx.x;
    if (slot >= (long long)B * K) return;
    const int b = (int)(slot / K), k = (int)(slot % K);
    if (k >= min(kp_count[b], K)) {                   // (a count beyond K is clamped, as in sample_desc_kernel)
        kp_sub_yx[slot * 2] = 0.f; kp_sub_yx[slot * 2 + 1] = 0.f;
        return;
    }
    const int y = kp_yx[slot * 2], x = kp_yx[slot * 2 + 1];
    float dy = 0.f, dx = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {         // (list entries are device data: nothing they hold may lead outside the map)
        const float* img = prob + (long long)b * H * W;
        const float* c = img + (long long)y * W + x;
        const bool in_y = y >= 1 && y + 1 < H, in_x = x >= 1 && x + 1 < W;
        const float p0 = *c;
        dy = parabola_offset(in_y, in_y ? c[-W] : 0.f, p0, in_y ? c[W] : 0.f);
        dx = parabola_offset(in_x, in_x ? c[-1] : 0.f, p0, in_x ? c[1] : 0.f);
    }
    kp_sub_yx[slot * 2] = (float)y + dy;
    kp_sub_yx[slot * 2 + 1] = (float)x + dx;
}

}  // namespace

void launch_refine_keypoints(const float* prob, int B, int H, int W, const int* kp_yx, const int* kp_count, int K,
                             float* kp_sub_yx, hipStream_t s)
{
    const long long slots = (long long)B * K;
    if (slots <= 0) return;
    hipLaunchKernelGGL(refine_keypoints_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, s, prob, B, H, W, kp_yx,
                       kp_count, K, kp_sub_yx);
}
