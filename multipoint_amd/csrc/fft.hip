// 2-D complex FFT in fp32 for line lengths 2^a 3^b 5^c in [8, 4096], batched over planes, and the log-Gabor stage of LGHD built
// on it.  No vendor library.
//
// A workgroup owns a BUNDLE of C lines, loads it into LDS once, runs every Stockham pass (mp_fft.h) between two LDS buffers and
// stores the bundle once.  Twiddles come from a table of exp(-2 pi i t / N) the host computed in double (fft_twiddles()).
//   row pass      C = 1: one line per workgroup, consecutive threads on consecutive elements
//   column pass   C = 16 adjacent columns (fewer above N = 512, where two buffers of 16 columns no longer fit 128 KiB of LDS):
//                 every global access is a run of 16 complex = 128 bytes of one image row; LDS holds buf[n * C + c]
// What a workgroup loads and stores is the MODE:
//   PLAIN   complex in, complex out (mp_fft2d; in == out is allowed: a bundle is read completely before it is written)
//   U8      the row pass of the forward transform of a uint8 image (real input)
//   BANK    the column pass of the inverse transform of spectrum * bank[plane], the real filter multiplied at the load: the
//           24 filtered spectra are never written
//   ARGMAX  the row pass of the inverse transform of the 6 orientation planes of one scale, one after the other through the same
//           LDS buffers; each thread keeps the running maximum of |response| of its pixels in registers and the row's index of the
//           FIRST maximum is all that is stored: the responses are never written
//   AMP     the row pass of the inverse transform that stores |response| * scale as one float per pixel (RIFT's noise planes)
// pc_rows_kernel is the row pass of RIFT's phase congruency: all 24 planes of a row through the same buffers,
// orientation-major, the per-pixel sums in registers; M, m and the maximum index map are all that is stored.
#include "mp_common.h"
#include "mp_fft.h"

namespace {

enum { PLAIN = 0, U8 = 1, BANK = 2, ARGMAX = 3, AMP = 4 };

struct FftArgs {
    FftPlan plan;
    const float2* tw;
    const void* in;
    void* out;
    const float* bank;     // BANK: [planes][H][W]
    float scale;           // AMP: the factor on |response|
    int H, W;
    int cshift;            // log2 C
    int cols;              // 1: lines are columns (N = H), 0: rows (N = W)
    int inverse;
    long long in_image_stride, in_plane_stride;     // elements of the input type between images (blockIdx.z) and planes (blockIdx.y)
    long long out_image_stride, out_plane_stride;
};

constexpr int ARGMAX_SLOTS = MP_FFT_MAX_N / 256;     // pixels of a row a thread of the 256 owns

// |E + iO| as both RIFT row passes compute it: the same instructions, so the same bits
__device__ __forceinline__ float pc_amplitude(float E, float O) { return __fsqrt_rn(__fmaf_rn(E, E, __fmul_rn(O, O))); }

template <int MODE>
__global__ __launch_bounds__(512) void fft_lines_kernel(const FftArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float2 fft_lds[];
    const int N = a.plan.N, cshift = a.cshift, C = 1 << cshift, tid = threadIdx.x, nthr = blockDim.x;
    float2 *cur = fft_lds, *oth = fft_lds + ((size_t)N << cshift);
    const int W = a.W;
    // element n of line c of this bundle lies at n * es + c * ls + first (in elements), lines c < nvalid exist
    const long long es = a.cols ? W : 1;
    const long long first = a.cols ? ((long long)blockIdx.x << cshift) : (long long)blockIdx.x * W;
    const int nvalid = a.cols ? min(C, W - (int)(blockIdx.x << cshift)) : 1;
    constexpr int REPS = MODE == ARGMAX ? 6 : 1;
    float best[ARGMAX_SLOTS];
    int besti[ARGMAX_SLOTS];
    if (MODE == ARGMAX) {
#pragma unroll
        for (int i = 0; i < ARGMAX_SLOTS; ++i) { best[i] = -1.f; besti[i] = 0; }
    }
    for (int rep = 0; rep < REPS; ++rep) {
        const long long plane = MODE == ARGMAX ? (long long)blockIdx.y * 6 + rep : blockIdx.y;
        const long long ibase = blockIdx.z * a.in_image_stride + (MODE == BANK ? 0 : plane * a.in_plane_stride) + first;
        for (int w = tid; w < (N << cshift); w += nthr) {
            const int n = w >> cshift, c = w & (C - 1);
            float2 v = float2{0.f, 0.f};
            if (c < nvalid) {
                const long long at = ibase + n * es + c;
                if (MODE == U8) v.x = (float)static_cast<const unsigned char*>(a.in)[at];
                else v = static_cast<const float2*>(a.in)[at];
                if (MODE == BANK) {
                    const float f = a.bank[plane * a.H * W + first + n * es + c];
                    v.x *= f; v.y *= f;
                }
            }
            cur[w] = v;
        }
        __syncthreads();
        int Ns = 1;
        for (int p = 0; p < a.plan.npass; ++p) {
            const int r = a.plan.radix[p];
            fft_pass(cur, oth, N, cshift, r, Ns, a.tw, a.inverse != 0, tid, nthr);
            Ns *= r;
            float2* t = cur; cur = oth; oth = t;
            __syncthreads();
        }
        if (MODE == ARGMAX) {
#pragma unroll
            for (int i = 0; i < ARGMAX_SLOTS; ++i) {
                const int n = tid + i * 256;
                if (n < N) {
                    const float2 v = cur[n];
                    const float m = sqrtf(v.x * v.x + v.y * v.y);
                    if (m > best[i]) { best[i] = m; besti[i] = rep; }       // strictly larger: the first maximum stays
                }
            }
            __syncthreads();        // the next plane's load overwrites a buffer this epilogue read
        } else if (MODE == AMP) {
            float* o = static_cast<float*>(a.out) + blockIdx.z * a.out_image_stride + plane * a.out_plane_stride + first;
            for (int n = tid; n < N; n += nthr) o[n] = pc_amplitude(cur[n].x * a.scale, cur[n].y * a.scale);
        } else {
            const long long obase = blockIdx.z * a.out_image_stride + plane * a.out_plane_stride + first;
            for (int w = tid; w < (N << cshift); w += nthr) {
                const int n = w >> cshift, c = w & (C - 1);
                if (c < nvalid) static_cast<float2*>(a.out)[obase + n * es + c] = cur[w];
            }
        }
    }
    if (MODE == ARGMAX) {
        unsigned char* o = static_cast<unsigned char*>(a.out) + blockIdx.z * a.out_image_stride + blockIdx.y * a.out_plane_stride + first;
#pragma unroll
        for (int i = 0; i < ARGMAX_SLOTS; ++i) {
            const int n = tid + i * 256;
            if (n < N) o[n] = (unsigned char)besti[i];
        }
    }
}

struct PcArgs {
    FftPlan plan;
    const float2* tw;
    const float2* in;      // [images][24][H][W]: the column-transformed planes, scale-major
    const float* T;        // [images][6] noise thresholds
    float *M, *m;          // [images][H][W]
    unsigned char* mim;    // [images][H][W]
    int W;
    long long HW;
    float scale;           // 1 / (H W)
    float g, cutoff;
    float ct[6], st[6];    // cos / sin of o pi / 6
};

constexpr float PC_EPS = 1e-4f;

// One row of one image per workgroup; thread t owns the pixels t + i * blockDim.x, i < SLOTS.  Orientation-major: the four scales
// of orientation o go through the LDS buffers one after the other, their (E, O) pairs stay in registers until the orientation is
// closed (mean phase direction, energy, noise threshold, frequency-spread weight), and the covariance sums and the running
// arg-max of sumA carry over the six orientations.  Every sum runs s = 0..3 inside o = 0..5: a pixel's bits do not depend on the
// launch.
template <int SLOTS>
__global__ __launch_bounds__(512) void pc_rows_kernel(const PcArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float2 fft_lds[];
    const int N = a.plan.N, tid = threadIdx.x, nthr = blockDim.x;
    float2 *cur = fft_lds, *oth = fft_lds + N;
    const float2* img = a.in + blockIdx.z * 24 * a.HW + (long long)blockIdx.x * a.W;
    float cx2[SLOTS], cy2[SLOTS], cxy[SLOTS], bestA[SLOTS];
    int besti[SLOTS];
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) { cx2[i] = cy2[i] = cxy[i] = 0.f; bestA[i] = -1.f; besti[i] = 0; }
    for (int o = 0; o < 6; ++o) {
        float E[SLOTS][4], O[SLOTS][4], sumA[SLOTS], maxA[SLOTS];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float2* line = img + (long long)(s * 6 + o) * a.HW;
            for (int n = tid; n < N; n += nthr) cur[n] = line[n];
            __syncthreads();
            int Ns = 1;
            for (int p = 0; p < a.plan.npass; ++p) {
                const int r = a.plan.radix[p];
                fft_pass(cur, oth, N, 0, r, Ns, a.tw, true, tid, nthr);
                Ns *= r;
                float2* t = cur; cur = oth; oth = t;
                __syncthreads();
            }
#pragma unroll
            for (int i = 0; i < SLOTS; ++i) {
                const int n = tid + i * nthr;
                const float2 v = n < N ? cur[n] : float2{0.f, 0.f};
                E[i][s] = v.x * a.scale; O[i][s] = v.y * a.scale;
                const float A = pc_amplitude(E[i][s], O[i][s]);
                sumA[i] = s ? sumA[i] + A : A;
                maxA[i] = s ? fmaxf(maxA[i], A) : A;
            }
            __syncthreads();        // the next plane's load overwrites a buffer this epilogue read
        }
        const float T = a.T[blockIdx.z * 6 + o];
#pragma unroll
        for (int i = 0; i < SLOTS; ++i) {
            const float sumE = ((E[i][0] + E[i][1]) + E[i][2]) + E[i][3], sumO = ((O[i][0] + O[i][1]) + O[i][2]) + O[i][3];
            const float X = sqrtf(sumE * sumE + sumO * sumO) + PC_EPS, mE = sumE / X, mO = sumO / X;
            float En = 0.f;
#pragma unroll
            for (int s = 0; s < 4; ++s) En += E[i][s] * mE + O[i][s] * mO - fabsf(E[i][s] * mO - O[i][s] * mE);
            En = fmaxf(En - T, 0.f);
            const float width = (sumA[i] / (maxA[i] + PC_EPS) - 1.f) / 3.f;
            const float weight = 1.f / (1.f + expf((a.cutoff - width) * a.g));
            const float pc = weight * En / (sumA[i] + PC_EPS);
            const float cx = pc * a.ct[o], cy = pc * a.st[o];
            cx2[i] += cx * cx; cy2[i] += cy * cy; cxy[i] += cx * cy;
            if (sumA[i] > bestA[i]) { bestA[i] = sumA[i]; besti[i] = o; }       // strictly larger: the first maximum stays
        }
    }
    const long long at = blockIdx.z * a.HW + (long long)blockIdx.x * a.W;
#pragma unroll
    for (int i = 0; i < SLOTS; ++i) {
        const int n = tid + i * nthr;
        if (n < N) {
            const float x2 = cx2[i] / 3.f, y2 = cy2[i] / 3.f, xy = cxy[i] * (4.f / 6.f);
            const float d = sqrtf(xy * xy + (x2 - y2) * (x2 - y2)) + PC_EPS;
            a.M[at + n] = (y2 + x2 + d) / 2.f;
            a.m[at + n] = (y2 + x2 - d) / 2.f;
            a.mim[at + n] = (unsigned char)besti[i];
        }
    }
}

constexpr size_t FFT_LDS_CAP = 128 * 1024;

template <int MODE>
void launch_lines(FftArgs a, int planes, int images, hipStream_t s)
{
    const int N = a.plan.N;
    int cshift = 0;
    if (a.cols) {
        cshift = 4;
        while (cshift > 0 && ((size_t)2 * sizeof(float2) * N << cshift) > FFT_LDS_CAP) --cshift;
    }
    a.cshift = cshift;
    const size_t lds = (size_t)2 * sizeof(float2) * N << cshift;
    const int bundles = a.cols ? (a.W + (1 << cshift) - 1) >> cshift : a.H;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fft_lines_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)FFT_LDS_CAP);
    // a bundle above 64 KiB has a CU to itself: 8 waves instead of 4 hide the passes' LDS latency.  (Rows stay at 256 threads:
    // the ARGMAX epilogue assigns pixels to threads by 256.)
    hipLaunchKernelGGL(fft_lines_kernel<MODE>, dim3(bundles, planes, images), dim3(lds > 64 * 1024 ? 512 : 256), lds, s, a);
}

}  // namespace

void fft_twiddles(int n, float* table)
{
    for (int t = 0; t < n; ++t) {
        const double w = -2.0 * 3.14159265358979323846 * (double)t / (double)n;
        table[2 * t] = (float)cos(w);
        table[2 * t + 1] = (float)sin(w);
    }
}

void launch_fft2d(const float* in, float* out, int planes, int H, int W, int inverse, int axes, const float* tw_rows,
                  const float* tw_cols, hipStream_t s)
{
    FftArgs a{};
    a.H = H; a.W = W; a.inverse = inverse;
    a.in_plane_stride = a.out_plane_stride = (long long)H * W;
    a.in = in; a.out = out;
    if (axes & 1) {
        fft_plan(W, a.plan);
        a.tw = reinterpret_cast<const float2*>(tw_rows); a.cols = 0;
        launch_lines<PLAIN>(a, planes, 1, s);
        a.in = out;
    }
    if (axes & 2) {
        fft_plan(H, a.plan);
        a.tw = reinterpret_cast<const float2*>(tw_cols); a.cols = 1;
        launch_lines<PLAIN>(a, planes, 1, s);
    }
}

// orientation[b][sc][y][x] = the first o in [0, 6) with the largest | ifft2(fft2(u8[b]) * bank[sc * 6 + o]) |[y][x];
// spectrum: nb complex frames, tmp: nb * 24 complex frames (the one round trip between the inverse column and row passes)
void launch_lghd_orientation(const unsigned char* u8, const float* bank, int nb, int H, int W, float* spectrum, float* tmp,
                             unsigned char* orientation, const float* tw_rows, const float* tw_cols, hipStream_t s)
{
    const long long HW = (long long)H * W;
    FftPlan rows, cols;
    fft_plan(W, rows); fft_plan(H, cols);
    FftArgs a{};
    a.H = H; a.W = W;
    // forward: rows of the image, then columns in place
    a.plan = rows; a.tw = reinterpret_cast<const float2*>(tw_rows); a.cols = 0; a.inverse = 0;
    a.in = u8; a.in_image_stride = HW; a.out = spectrum; a.out_image_stride = HW;
    launch_lines<U8>(a, 1, nb, s);
    a.plan = cols; a.tw = reinterpret_cast<const float2*>(tw_cols); a.cols = 1;
    a.in = spectrum; a.in_image_stride = HW;
    launch_lines<PLAIN>(a, 1, nb, s);
    // inverse: columns of spectrum * bank, then rows with the arg-max
    a.inverse = 1; a.bank = bank;
    a.out = tmp; a.out_image_stride = 24 * HW; a.out_plane_stride = HW;
    launch_lines<BANK>(a, 24, nb, s);
    a.plan = rows; a.tw = reinterpret_cast<const float2*>(tw_rows); a.cols = 0; a.bank = nullptr;
    a.in = tmp; a.in_image_stride = 24 * HW; a.in_plane_stride = HW;
    a.out = orientation; a.out_image_stride = 4 * HW; a.out_plane_stride = HW;
    launch_lines<ARGMAX>(a, 4, nb, s);
}

// RIFT's phase congruency of nb images: the transforms of launch_lghd_orientation up to the 24 half-transformed
// planes in tmp, then   amp[b][o] = |response of scale 0, orientation o| / (H W)   (nb * 6 real frames),
// T[b][o] from their exact medians (rift.hip), and the row pass that leaves M, m and the maximum index map.
void launch_rift_phase_congruency(const unsigned char* u8, const float* bank, int nb, int H, int W, float k, float g, float cutoff,
                                  float* spectrum, float* tmp, float* amp, float* T, float* M, float* m, unsigned char* mim,
                                  const float* tw_rows, const float* tw_cols, hipStream_t s)
{
    const long long HW = (long long)H * W;
    FftPlan rows, cols;
    fft_plan(W, rows); fft_plan(H, cols);
    FftArgs a{};
    a.H = H; a.W = W;
    a.plan = rows; a.tw = reinterpret_cast<const float2*>(tw_rows); a.cols = 0; a.inverse = 0;
    a.in = u8; a.in_image_stride = HW; a.out = spectrum; a.out_image_stride = HW;
    launch_lines<U8>(a, 1, nb, s);
    a.plan = cols; a.tw = reinterpret_cast<const float2*>(tw_cols); a.cols = 1;
    a.in = spectrum; a.in_image_stride = HW;
    launch_lines<PLAIN>(a, 1, nb, s);
    a.inverse = 1; a.bank = bank;
    a.out = tmp; a.out_image_stride = 24 * HW; a.out_plane_stride = HW;
    launch_lines<BANK>(a, 24, nb, s);
    // the six planes of scale 0 once more than the others: their amplitudes have to exist before any pixel can be thresholded
    a.plan = rows; a.tw = reinterpret_cast<const float2*>(tw_rows); a.cols = 0; a.bank = nullptr;
    a.in = tmp; a.in_image_stride = 24 * HW; a.in_plane_stride = HW;
    a.out = amp; a.out_image_stride = 6 * HW; a.out_plane_stride = HW;
    a.scale = 1.0f / (float)HW;
    launch_lines<AMP>(a, 6, nb, s);
    launch_rift_noise_threshold(amp, nb * 6, HW, k, T, s);
    PcArgs p{};
    p.plan = rows; p.tw = reinterpret_cast<const float2*>(tw_rows);
    p.in = reinterpret_cast<const float2*>(tmp); p.T = T; p.M = M; p.m = m; p.mim = mim;
    p.W = W; p.HW = HW; p.scale = a.scale; p.g = g; p.cutoff = cutoff;
    for (int o = 0; o < 6; ++o) {
        p.ct[o] = (float)cos(o * 3.14159265358979323846 / 6.0);
        p.st[o] = (float)sin(o * 3.14159265358979323846 / 6.0);
    }
    // 2, 4 or 8 pixels per thread of 256 (512 above 2048): the smallest that covers the row, so that a 640-wide frame does not
    // carry the registers of a 4096-wide one
    const size_t lds = (size_t)2 * sizeof(float2) * W;
    const dim3 grid(H, 1, nb);
    if (W <= 512) hipLaunchKernelGGL(pc_rows_kernel<2>, grid, dim3(256), lds, s, p);
    else if (W <= 1024) hipLaunchKernelGGL(pc_rows_kernel<4>, grid, dim3(256), lds, s, p);
    else hipLaunchKernelGGL(pc_rows_kernel<8>, grid, dim3(W <= 2048 ? 256 : 512), lds, s, p);
}
