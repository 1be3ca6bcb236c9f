// Host emulation of fft_lines_kernel (multipoint_amd/csrc/fft.hip) for tests/test_lghd_shapes_host.py: the passes of
// multipoint_amd/csrc/mp_fft.h over one bundle of C = 1 << cshift lines, compiled by a plain C++ compiler and loaded with ctypes.
// Everything but the loads and stores of global memory is the kernel's: two ping-pong buffers laid out as buf[n * C + c], the
// twiddle table of fft_twiddles() (computed in double, rounded once), and every pass run by each thread `tid` of `nthr` before
// the next pass starts (the kernel's __syncthreads()).
#include <cmath>
#include <vector>

#include "mp_fft.h"

extern "C" {

// fft_plan(n): returns its verdict, *npass and radix[0 .. *npass) as it left them (radix holds MP_FFT_MAX_PASSES ints)
int fft_host_plan(int n, int* npass, int* radix)
{
    FftPlan p;
    const bool ok = fft_plan(n, p);
    *npass = p.npass;
    for (int i = 0; i < p.npass; ++i) radix[i] = p.radix[i];
    return ok ? 1 : 0;
}

// in, out: (n << cshift) complex numbers as interleaved floats, element n of line c at [n * C + c].  0, -1 for a length
// without a plan or a bad argument, -2 if a pass wrote behind a buffer (each has a guard of its own size behind it: a store index
// of a pass with a wrong k stays below 2 n).
int fft_host_lines(const float* in, float* out, int n, int cshift, int inverse, int nthr)
{
    FftPlan plan;
    if (!in || !out || cshift < 0 || cshift > 4 || nthr < 1 || !fft_plan(n, plan)) return -1;
    std::vector<float2> tw((size_t)n);
    for (int t = 0; t < n; ++t) {
        const double w = -2.0 * 3.14159265358979323846 * (double)t / (double)n;
        tw[t] = float2{(float)cos(w), (float)sin(w)};
    }
    const size_t total = (size_t)n << cshift;
    const float guard = -12345.f;
    std::vector<float2> a(2 * total, float2{guard, guard}), b(2 * total, float2{guard, guard});
    for (size_t i = 0; i < total; ++i) a[i] = float2{in[2 * i], in[2 * i + 1]};
    float2 *cur = a.data(), *oth = b.data();
    int Ns = 1;
    for (int p = 0; p < plan.npass; ++p) {
        const int r = plan.radix[p];
        for (int tid = 0; tid < nthr; ++tid) fft_pass(cur, oth, n, cshift, r, Ns, tw.data(), inverse != 0, tid, nthr);
        Ns *= r;
        float2* t = cur; cur = oth; oth = t;
    }
    for (size_t i = total; i < 2 * total; ++i)
        if (a[i].x != guard || a[i].y != guard || b[i].x != guard || b[i].y != guard) return -2;
    for (size_t i = 0; i < total; ++i) { out[2 * i] = cur[i].x; out[2 * i + 1] = cur[i].y; }
    return 0;
}

}  // extern "C"
