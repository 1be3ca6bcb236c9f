// The image pyramid of the staged mutual-information alignment (reference create_dataset/align_images.py:163-171 and
// helper_functions/align.py:485-489): cv2.GaussianBlur(frame, (k, k), 0) on fp32 frames with the reference's
// [::2, ::2] fused into it, and the conversion of 8- / 16-bit frames to fp32.
//
//   pyr_blur_kernel<DEC, KT>   one workgroup per tile of 64 input columns and 16 output rows of one frame.  The tile and its
//                              halo of k/2 pixels (BORDER_REFLECT_101) go to LDS -- along a row the lanes read the 128-byte
//                              runs the tile's columns lie in, so every global access is a whole aligned run where W is a
//                              multiple of 32 --, the row filter of sepFilter2D writes a second LDS array (taps summed left to
//                              right), the symmetric column filter (centre tap, then ky[r+j] (S[+j] + S[-j])) reads that and
//                              stores the output rows.  DEC = 1 keeps the even rows and columns only: the row filter runs at
//                              the even columns, the column filter at the even rows, with the arithmetic of the full-size
//                              blur, so its output is bit for bit the undecimated one's [::2, ::2].  KT > 0 fixes k at compile
//                              time (weights in registers), KT = 0 takes any odd k <= 31.
//   frames_to_float_kernel     one thread per pixel: u8 / 255, u8 BGR / 255 then COLOR_BGR2GRAY, u16 / 65535.
//
// The weights are getGaussianKernel(k, 0, CV_32F), computed on the host: OpenCV's fixed tables up to k = 7, above that exp in
// double, stored as float and normalised.  All pixel arithmetic is fp32 with every step rounded (no contraction into FMA), so
// that a numpy float32 restatement matches bit for bit.
#include "host.h"
#include "mp_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int MAX_K = 31;
constexpr int TILE_W = 64;          // input columns of a tile: 64 output columns, or 32 (one 128-byte run) with decimation
constexpr int OUT_H = 16;           // output rows of a tile
constexpr int THREADS = 256;

struct BlurWeights {
    float w[MAX_K];
};

// (the border is reflect101 of mp_device.h; k/2 < n keeps every pixel an output needs within one reflection)

// dynamic LDS: 32 floats of weights | the input rows [nrows][PW] | the row-filtered rows [nrows][OW]
template <int DEC, int KT>
__global__ __launch_bounds__(THREADS) void pyr_blur_kernel(const float* __restrict__ in, int H, int W, int Ho, int Wo, int k_any,
                                                           BlurWeights wt, float* __restrict__ out)
{
    constexpr int S = DEC ? 2 : 1;
    constexpr int OW = TILE_W / S;
    const int k = KT ? KT : k_any, r = k / 2;
    const int halo = (r + 31) & ~31;                   // the halo's columns, in whole 128-byte runs: 0 or 32
    const int PW = TILE_W + 2 * halo;
    const int nrows = (OUT_H - 1) * S + 1 + 2 * r;
    extern __shared__ float lds[];
    float* wl = lds;
    float* tin = lds + 32;
    float* trow = tin + nrows * PW;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * OUT_H * S;        // the tile's first input column and row
    const float* src = in + (long long)blockIdx.z * H * W;

#pragma unroll
    for (int i = 0; i < MAX_K; ++i)
        if (tid == i) wl[i] = wt.w[i];
    for (int idx = tid; idx < nrows * PW; idx += THREADS) {
        const int row = idx / PW, c = idx - row * PW;
        if (c < halo - r || c >= halo + TILE_W + r) continue;
        tin[idx] = src[(long long)reflect101(y0 - r + row, H) * W + reflect101(x0 - halo + c, W)];
    }
    __syncthreads();

    float wr[KT ? KT : 1];
    if (KT) {
#pragma unroll
        for (int j = 0; j < KT; ++j) wr[j] = wl[j];
    }
    for (int idx = tid; idx < nrows * OW; idx += THREADS) {
        const int row = idx / OW, ox = idx - row * OW;
        const float* e = tin + row * PW + halo - r + ox * S;
        float s;
        if (KT) {
            s = wr[0] * e[0];
#pragma unroll
            for (int j = 1; j < KT; ++j) s = s + wr[j] * e[j];
        } else {
            s = wl[0] * e[0];
            for (int j = 1; j < k; ++j) s = s + wl[j] * e[j];
        }
        trow[idx] = s;
    }
    __syncthreads();

    float* dst = out + (long long)blockIdx.z * Ho * Wo;
    for (int idx = tid; idx < OUT_H * OW; idx += THREADS) {
        const int oy = idx / OW, ox = idx - oy * OW;
        const int gy = blockIdx.y * OUT_H + oy, gx = blockIdx.x * OW + ox;
        if (gy >= Ho || gx >= Wo) continue;
        const float* c = trow + (oy * S + r) * OW + ox;
        float s;
        if (KT) {
            s = wr[KT / 2] * c[0];
#pragma unroll
            for (int j = 1; j <= KT / 2; ++j) s = s + wr[KT / 2 + j] * (c[j * OW] + c[-j * OW]);
        } else {
            s = wl[r] * c[0];
            for (int j = 1; j <= r; ++j) s = s + wl[r + j] * (c[j * OW] + c[-j * OW]);
        }
        dst[(long long)gy * Wo + gx] = s;
    }
}

__global__ __launch_bounds__(THREADS) void frames_to_float_kernel(const void* __restrict__ in, int mode, long long total,
                                                                  float* __restrict__ out)
{
    const long long p = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (p >= total) return;
    if (mode == MP_FRAMES_U8) {
        out[p] = (float)((const unsigned char*)in)[p] / 255.0f;
    } else if (mode == MP_FRAMES_U16) {
        out[p] = (float)((const unsigned short*)in)[p] / 65535.0f;
    } else {
        const unsigned char* px = (const unsigned char*)in + 3 * p;
        const float b = (float)px[0] / 255.0f, g = (float)px[1] / 255.0f, r = (float)px[2] / 255.0f;
        out[p] = (0.114f * b + 0.587f * g) + 0.299f * r;
    }
}

// getGaussianKernel(k, 0, CV_32F)
void gaussian_weights(int k, float* w)
{
    static const float tab[4][7] = {{1.f},
                                    {0.25f, 0.5f, 0.25f},
                                    {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f},
                                    {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f}};
    if (k <= 7) {
        for (int i = 0; i < k; ++i) w[i] = tab[k / 2][i];
        return;
    }
    const double sigma = ((k - 1) * 0.5 - 1) * 0.3 + 0.8;
    const double scale2x = -0.5 / (sigma * sigma);
    double sum = 0.0;
    for (int i = 0; i < k; ++i) {
        const double x = i - (k - 1) * 0.5;
        w[i] = (float)std::exp(scale2x * x * x);
        sum += (double)w[i];
    }
    sum = 1.0 / sum;
    for (int i = 0; i < k; ++i) w[i] = (float)((double)w[i] * sum);
}

template <int DEC>
void launch_blur(const float* in, int n, int H, int W, int Ho, int Wo, int k, const BlurWeights& wt, float* out, hipStream_t s)
{
    constexpr int S = DEC ? 2 : 1;
    const int r = k / 2, halo = (r + 31) & ~31;
    const int nrows = (OUT_H - 1) * S + 1 + 2 * r;
    const size_t lds = sizeof(float) * (32 + (size_t)nrows * (TILE_W + 2 * halo) + (size_t)nrows * (TILE_W / S));
    const dim3 grid((W + TILE_W - 1) / TILE_W, (Ho + OUT_H - 1) / OUT_H, n);
    switch (k) {
    case 3: pyr_blur_kernel<DEC, 3><<<grid, THREADS, lds, s>>>(in, H, W, Ho, Wo, k, wt, out); break;
    case 5: pyr_blur_kernel<DEC, 5><<<grid, THREADS, lds, s>>>(in, H, W, Ho, Wo, k, wt, out); break;
    case 7: pyr_blur_kernel<DEC, 7><<<grid, THREADS, lds, s>>>(in, H, W, Ho, Wo, k, wt, out); break;
    case 9: pyr_blur_kernel<DEC, 9><<<grid, THREADS, lds, s>>>(in, H, W, Ho, Wo, k, wt, out); break;
    default: pyr_blur_kernel<DEC, 0><<<grid, THREADS, lds, s>>>(in, H, W, Ho, Wo, k, wt, out); break;
    }
}

}  // namespace

using namespace mp_host;

extern "C" {

int mp_gaussian_weights(int ksize, float* weights)
{
    if (!weights || ksize < 1 || ksize > MAX_K || ksize % 2 == 0) return MP_EINVAL;
    gaussian_weights(ksize, weights);
    return MP_OK;
}

int mp_gaussian_blur(mp_handle* h, const float* in, int n, int H, int W, int ksize, int decimate, float* out, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!in || !out) return fail(h, MP_EINVAL, "mp_gaussian_blur: NULL tensor");
    if (in == out) return fail(h, MP_EINVAL, "mp_gaussian_blur: in and out must be different buffers (the filter is not in place)");
    if (ksize < 1 || ksize > MAX_K || ksize % 2 == 0)
        return fail(h, MP_EINVAL, "mp_gaussian_blur: ksize must be odd and in [1, " + std::to_string(MAX_K) + "], got " +
                                      std::to_string(ksize));
    if (!frames_ok(n, H, W, 1, 32767))
        return fail(h, MP_EINVAL, "mp_gaussian_blur: 1 to 65535 frames of 1 x 1 to 32767 x 32767 pixels");
    if (ksize / 2 >= (H < W ? H : W))
        return fail(h, MP_EINVAL, "mp_gaussian_blur: ksize / 2 = " + std::to_string(ksize / 2) + " must be below the frame's "
                                      "smaller side (" + std::to_string(H < W ? H : W) + "): BORDER_REFLECT_101 reflects once");
    MP_HIP(hipSetDevice(h->device));
    BlurWeights wt{};
    gaussian_weights(ksize, wt.w);
    if (decimate)
        launch_blur<1>(in, n, H, W, (H + 1) / 2, (W + 1) / 2, ksize, wt, out, (hipStream_t)stream);
    else
        launch_blur<0>(in, n, H, W, H, W, ksize, wt, out, (hipStream_t)stream);
    return launch_status(h);
}

int mp_frames_to_float(mp_handle* h, const void* in, int mode, int n, int H, int W, float* out, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!in || !out) return fail(h, MP_EINVAL, "mp_frames_to_float: NULL tensor");
    if (mode != MP_FRAMES_U8 && mode != MP_FRAMES_BGR8 && mode != MP_FRAMES_U16)
        return fail(h, MP_EINVAL, "mp_frames_to_float: mode must be MP_FRAMES_U8, MP_FRAMES_BGR8 or MP_FRAMES_U16");
    if (!frames_ok(n, H, W, 1, 32767))
        return fail(h, MP_EINVAL, "mp_frames_to_float: 1 to 65535 frames of 1 x 1 to 32767 x 32767 pixels");
    const long long total = (long long)n * H * W;
    if (total > (1LL << 38)) return fail(h, MP_EINVAL, "mp_frames_to_float: at most 2^38 pixels per call");
    MP_HIP(hipSetDevice(h->device));
    frames_to_float_kernel<<<(unsigned)((total + THREADS - 1) / THREADS), THREADS, 0, (hipStream_t)stream>>>(in, mode, total, out);
    return launch_status(h);
}

}  // extern "C"
