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
#include "mp_common.h"
#include "mp_fft.h"

namespace {

enum { PLAIN = 0, U8 = 1, BANK = 2, ARGMAX = 3 };

struct FftArgs {
    FftPlan plan;
    const float2* tw;
    const void* in;
    void* out;
    const float* bank;     // BANK: [planes][H][W]
    int H, W;
    int cshift;            // log2 C
    int cols;              // 1: lines are columns (N = H), 0: rows (N = W)
    int inverse;
    long long in_image_stride, in_plane_stride;     // elements of the input type between images (blockIdx.z) and planes (blockIdx.y)
    long long out_image_stride, out_plane_stride;
};

constexpr int ARGMAX_SLOTS = MP_FFT_MAX_N / 256;     // pixels of a row a thread of the 256 owns

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
