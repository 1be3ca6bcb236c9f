// LGHD baseline (reference multipoint/models/ClassicDetectors.py, class LGHD): image quantisation, the FAST-9/16
// detector and the patch-histogram descriptor.  The log-Gabor orientation maps come from fft.hip.  Integer arithmetic throughout:
// every output here is bit-exact.  The FAST kernels and the patch histogram take the threshold, the validity border and the patch
// geometry as arguments: rift.hip runs the same bodies on its own maps.
#include "mp_common.h"

namespace {

constexpr int FAST_THRESHOLD = 10;
constexpr int LGHD_HALF = 20;       // patch 40 x 40, cells 10 x 10, 4 scales x 16 cells x 6 orientations = 384
constexpr int LGHD_D = 384;

// (image * 255.0).astype(np.uint8): one fp32 multiply, then truncation
__global__ __launch_bounds__(256) void quantize_kernel(const float* __restrict__ image, unsigned char* __restrict__ u8, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) u8[i] = (unsigned char)(int)(image[i] * 255.0f);
}

// score(p) = the largest t for which 9 contiguous circle pixels are all > p + t or all < p - t; 0 below the threshold and
// outside 3 <= y <= H - 4, 3 <= x <= W - 4
__global__ __launch_bounds__(256) void fast_score_kernel(const unsigned char* __restrict__ u8, int H, int W, int threshold,
                                                        unsigned char* __restrict__ score)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const long long plane = (long long)blockIdx.z * H * W;
    int sc = 0;
    if (y >= 3 && y <= H - 4 && x >= 3 && x <= W - 4) {
        const unsigned char* im = u8 + plane;
        const int p = im[(long long)y * W + x];
        const int dx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
        const int dy[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
        int d[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) d[i] = (int)im[(long long)(y + dy[i]) * W + (x + dx[i])] - p;
        int best = -256;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            int mn = d[s], mx = d[s];
#pragma unroll
            for (int k = 1; k < 9; ++k) { mn = min(mn, d[(s + k) & 15]); mx = max(mx, d[(s + k) & 15]); }
            best = max(best, max(mn - 1, -mx - 1));
        }
        sc = best >= threshold ? best : 0;
    }
    score[plane + (long long)y * W + x] = (unsigned char)sc;
}

// corner: score strictly above all 8 neighbours; prob = 1 (scored: score / 255) at corners whose patch of 2 half x 2 half lies
// inside the frame
__global__ __launch_bounds__(256) void fast_nms_kernel(const unsigned char* __restrict__ score, int H, int W, int half, int scored,
                                                      unsigned char* __restrict__ corners, float* __restrict__ prob)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const long long plane = (long long)blockIdx.z * H * W, at = plane + (long long)y * W + x;
    const int s = score[at];
    bool keep = s > 0;
    if (keep) {
        for (int j = -1; j <= 1; ++j)
            for (int i = -1; i <= 1; ++i) {
                const int yy = y + j, xx = x + i;
                if ((i || j) && yy >= 0 && yy < H && xx >= 0 && xx < W && (int)score[plane + (long long)yy * W + xx] >= s) keep = false;
            }
    }
    corners[at] = keep ? 1 : 0;
    if (prob) prob[at] = (keep && y >= half && y <= H - half && x >= half && x <= W - half) ? (scored ? __fdiv_rn((float)s, 255.f) : 1.f) : 0.f;
}

// one workgroup per keypoint slot: the patch of S planes of orientation indices in G x G cells of cell x cell pixels -> S G G 6
// counts in LDS (LGHD: 4 scales x 40 x 40 -> 384; RIFT: the one maximum index map, 6 x 6 cells -> 216).  CELL = 0: the cell edge
// is the argument.  Rows are `width` floats apart and zero behind the counts.
template <int S, int G, int CELL>
__global__ __launch_bounds__(256) void patch_describe_kernel(const unsigned char* __restrict__ ori, int H, int W, int cell_arg,
                                                            int width, const int* __restrict__ kp_yx,
                                                            const int* __restrict__ kp_count, int K, float* __restrict__ raw,
                                                            float* __restrict__ unit)
{
    constexpr int D = S * G * G * 6;
    const int cell = CELL ? CELL : cell_arg, P = G * cell, half = P / 2;
    __shared__ int hist[D];
    __shared__ int wsum[4];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const long long row = ((long long)b * K + k) * width;
    for (int i = D + tid; i < width; i += 256) { if (raw) raw[row + i] = 0.f; if (unit) unit[row + i] = 0.f; }
    const int cnt = min(kp_count[b], K);
    int y = 0, x = 0;
    bool live = k < cnt;
    if (live) {
        y = kp_yx[((long long)b * K + k) * 2]; x = kp_yx[((long long)b * K + k) * 2 + 1];
        live = y >= half && y <= H - half && x >= half && x <= W - half;     // a patch outside the frame: zeros
    }
    if (!live) {                // (uniform over the workgroup)
        for (int i = tid; i < D; i += 256) { if (raw) raw[row + i] = 0.f; if (unit) unit[row + i] = 0.f; }
        return;
    }
    for (int i = tid; i < D; i += 256) hist[i] = 0;
    __syncthreads();
    const unsigned char* base = ori + (long long)b * S * H * W;
    for (int i = tid; i < S * P * P; i += 256) {
        const int s = i / (P * P), r = i - s * (P * P), py = r / P, px = r - py * P;
        const int o = base[((long long)s * H + (y - half + py)) * W + (x - half + px)];
        if (o < 6) atomicAdd(&hist[((s * G + py / cell) * G + px / cell) * 6 + o], 1);
    }
    __syncthreads();
    int ss = 0;
    for (int i = tid; i < D; i += 256) ss += hist[i] * hist[i];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) ss += __shfl_xor(ss, off);
    if ((tid & 63) == 0) wsum[tid >> 6] = ss;
    __syncthreads();
    const float norm = sqrtf((float)(wsum[0] + wsum[1] + wsum[2] + wsum[3]));      // the sum of squares is an exact integer < 2^24
    for (int i = tid; i < D; i += 256) {
        const float v = (float)hist[i];
        if (raw) raw[row + i] = v;
        if (unit) unit[row + i] = v / norm;
    }
}

}  // namespace

void launch_lghd_quantize(const float* image, unsigned char* u8, long long n, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(quantize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, image, u8, n);
}

void launch_fast_detect(const unsigned char* u8, int B, int H, int W, int threshold, int half, int scored, unsigned char* score,
                        unsigned char* corners, float* prob, hipStream_t s)
{
    const dim3 g((W + 63) / 64, (H + 3) / 4, B);
    hipLaunchKernelGGL(fast_score_kernel, g, dim3(256), 0, s, u8, H, W, threshold, score);
    hipLaunchKernelGGL(fast_nms_kernel, g, dim3(256), 0, s, score, H, W, half, scored, corners, prob);
}

void launch_lghd_detect(const unsigned char* u8, int B, int H, int W, unsigned char* score, unsigned char* corners, float* prob,
                        hipStream_t s)
{
    launch_fast_detect(u8, B, H, W, FAST_THRESHOLD, LGHD_HALF, 0, score, corners, prob, s);
}

void launch_lghd_describe(const unsigned char* ori, int B, int H, int W, const int* kp_yx, const int* kp_count, int K, float* raw,
                          float* unit, hipStream_t s)
{
    hipLaunchKernelGGL((patch_describe_kernel<4, 4, 10>), dim3(K, B), dim3(256), 0, s, ori, H, W, 10, LGHD_D, kp_yx, kp_count, K, raw,
                       unit);
}

void launch_rift_describe(const unsigned char* mim, int B, int H, int W, int patch, const int* kp_yx, const int* kp_count, int K,
                          float* raw, float* unit, hipStream_t s)
{
    hipLaunchKernelGGL((patch_describe_kernel<1, 6, 0>), dim3(K, B), dim3(256), 0, s, mim, H, W, patch / 6, 256, kp_yx, kp_count, K,
                       raw, unit);
}
