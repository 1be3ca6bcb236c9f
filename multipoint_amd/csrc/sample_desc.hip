// Descriptor sampling: utils.interpolate_descriptors (reference multipoint/utils/utils.py:159-167):
//     g = kp / (S * 0.5) - 1  ->  F.grid_sample(bilinear, zeros padding, align_corners=True)
//     -> F.normalize(p=2, dim=1).  One wave per keypoint, lane = channel; the coarse descriptor
//     map is channels-last, so each of the 4 bilinear taps is one coalesced 256-byte load.
#include "mp_common.h"

namespace {

// KP: int (pixel keypoints) or float (sub-pixel positions, what the reference's keypoints.float() admits); one body from the cast on
template <class KP>
__global__ __launch_bounds__(256) void sample_desc_kernel(const float* __restrict__ desc, int B, int Hc,
                                                         int Wc, int D, int H, int W,
                                                         const KP* __restrict__ kp_yx,
                                                         const int* __restrict__ kp_count, int K,
                                                         float* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const long long wid = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wid >= (long long)B * K) return;
    const int b = (int)(wid / K), k = (int)(wid % K);
    const int cnt = min(kp_count[b], K);
    if (k >= cnt) {                                   // rows beyond the image's keypoint count: zeros (the output is fully written)
        for (int r = 0; r < (D >> 6); ++r) out[wid * D + r * 64 + lane] = 0.f;
        return;
    }
    const KP y = kp_yx[wid * 2], x = kp_yx[wid * 2 + 1];
    // utils.py:162-163 (fp32) then ATen grid_sampler unnormalize, align_corners=True
    const float gy = (float)y / ((float)H * 0.5f) - 1.0f;
    const float gx = (float)x / ((float)W * 0.5f) - 1.0f;
    const float iy = ((gy + 1.f) / 2.f) * (float)(Hc - 1);
    const float ix = ((gx + 1.f) / 2.f) * (float)(Wc - 1);
    const float y0f = floorf(iy), x0f = floorf(ix);
    const float y1f = y0f + 1.f, x1f = x0f + 1.f;
    const float w_nw = (x1f - ix) * (y1f - iy), w_ne = (ix - x0f) * (y1f - iy);
    const float w_sw = (x1f - ix) * (iy - y0f), w_se = (ix - x0f) * (iy - y0f);
    const int y0 = (int)y0f, x0 = (int)x0f, y1 = y0 + 1, x1 = x0 + 1;
    const bool vy0 = y0 >= 0 && y0 < Hc, vy1 = y1 >= 0 && y1 < Hc;
    const bool vx0 = x0 >= 0 && x0 < Wc, vx1 = x1 >= 0 && x1 < Wc;
    const float* base = desc + (long long)b * Hc * Wc * D;
    float ss = 0.f;
    float vals[6];                      // D <= 384
    const int nrep = D >> 6;
    for (int r = 0; r < nrep; ++r) {
        const int c = r * 64 + lane;
        const float nw = (vy0 && vx0) ? base[((long long)y0 * Wc + x0) * D + c] : 0.f;
        const float ne = (vy0 && vx1) ? base[((long long)y0 * Wc + x1) * D + c] : 0.f;
        const float sw = (vy1 && vx0) ? base[((long long)y1 * Wc + x0) * D + c] : 0.f;
        const float se = (vy1 && vx1) ? base[((long long)y1 * Wc + x1) * D + c] : 0.f;
        const float v = nw * w_nw + ne * w_ne + sw * w_sw + se * w_se;
        vals[r] = v;
        ss += v * v;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) ss += __shfl_xor(ss, off);
    const float denom = fmaxf(sqrtf(ss), 1e-12f);          // F.normalize eps
    for (int r = 0; r < nrep; ++r) out[wid * D + r * 64 + lane] = vals[r] / denom;
}

}  // namespace

template <class KP>
void launch_sample_desc(const float* desc, int B, int Hc, int Wc, int D, int H, int W,
                        const KP* kp_yx, const int* kp_count, int K, float* out, hipStream_t s)
{
    const long long waves = (long long)B * K;
    if (waves <= 0) return;
    hipLaunchKernelGGL(sample_desc_kernel<KP>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, desc, B,
                       Hc, Wc, D, H, W, kp_yx, kp_count, K, out);
}

template void launch_sample_desc<int>(const float*, int, int, int, int, int, int, const int*, const int*, int, float*, hipStream_t);
template void launch_sample_desc<float>(const float*, int, int, int, int, int, int, const float*, const int*, int, float*, hipStream_t);
