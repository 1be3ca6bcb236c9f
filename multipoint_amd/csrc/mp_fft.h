// The Stockham pass of the 2-D FFT (fft.hip): radix 2, 3, 4 and 5 butterflies over a bundle of C lines held in LDS as
// buf[n * C + c].  Host-compilable so that the pass can be checked without a device.  Internal header.
//
// A length N = r_0 r_1 ... r_{p-1}.  Pass i (radix r, Ns = r_0 ... r_{i-1}) does, for every j in [0, N / r):
//     k = j mod Ns,  v[q] = in[j + q N / r] * w^(q k N / (Ns r)),  w = exp(-/+ 2 pi i / N)   (table: forward, conjugated for the inverse)
//     out[(j - k) r + k + q Ns] = DFT_r(v)[q]
// after the last pass the line is in natural order (autosort: no bit reversal).
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MP_FFT_HD __host__ __device__ __forceinline__
#define MP_FFT_UNROLL _Pragma("unroll")
#else
struct float2 { float x, y; };
#define MP_FFT_HD inline
#define MP_FFT_UNROLL               // (a plain C++ compiler does not know the pragma)
#endif

#define MP_FFT_MAX_PASSES 12
#define MP_FFT_MIN_N 8
#define MP_FFT_MAX_N 4096

struct FftPlan {
    int N, npass;
    int radix[MP_FFT_MAX_PASSES];
};

// radices of n = 2^a 3^b 5^c in [8, 4096] (4 first: fewest passes); false for any other n
inline bool fft_plan(int n, FftPlan& p)
{
    p.N = n; p.npass = 0;
    if (n < MP_FFT_MIN_N || n > MP_FFT_MAX_N) return false;
    const int cand[4] = {4, 2, 3, 5};
    for (int r : cand)
        while (n % r == 0) {
            if (p.npass == MP_FFT_MAX_PASSES) return false;
            p.radix[p.npass++] = r;
            n /= r;
        }
    return n == 1;
}

MP_FFT_HD float2 fft_cmul(float2 a, float2 b) { return float2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
MP_FFT_HD float2 fft_add(float2 a, float2 b) { return float2{a.x + b.x, a.y + b.y}; }
MP_FFT_HD float2 fft_sub(float2 a, float2 b) { return float2{a.x - b.x, a.y - b.y}; }
// a + i s b
MP_FFT_HD float2 fft_add_i(float2 a, float2 b, float s) { return float2{a.x - s * b.y, a.y + s * b.x}; }

// v = DFT_r(v) with the kernel exp(sg 2 pi i q m / r), sg = -1 (forward) or +1 (inverse)
MP_FFT_HD void fft_butterfly(float2* v, int r, float sg)
{
    if (r == 2) {
        const float2 a = v[0], b = v[1];
        v[0] = fft_add(a, b); v[1] = fft_sub(a, b);
    } else if (r == 4) {
        const float2 a = fft_add(v[0], v[2]), b = fft_sub(v[0], v[2]), c = fft_add(v[1], v[3]), d = fft_sub(v[1], v[3]);
        v[0] = fft_add(a, c); v[2] = fft_sub(a, c);
        v[1] = fft_add_i(b, d, sg); v[3] = fft_add_i(b, d, -sg);
    } else if (r == 3) {
        const float s3 = 0.86602540378443864676f;
        const float2 t = fft_add(v[1], v[2]), d = fft_sub(v[1], v[2]);
        const float2 m = float2{v[0].x - 0.5f * t.x, v[0].y - 0.5f * t.y};
        const float2 e = float2{s3 * d.x, s3 * d.y};
        v[0] = fft_add(v[0], t);
        v[1] = fft_add_i(m, e, sg); v[2] = fft_add_i(m, e, -sg);
    } else {
        const float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f;
        const float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;
        const float2 a1 = fft_add(v[1], v[4]), b1 = fft_sub(v[1], v[4]), a2 = fft_add(v[2], v[3]), b2 = fft_sub(v[2], v[3]);
        const float2 m1 = float2{v[0].x + c1 * a1.x + c2 * a2.x, v[0].y + c1 * a1.y + c2 * a2.y};
        const float2 m2 = float2{v[0].x + c2 * a1.x + c1 * a2.x, v[0].y + c2 * a1.y + c1 * a2.y};
        const float2 e1 = float2{s1 * b1.x + s2 * b2.x, s1 * b1.y + s2 * b2.y};
        const float2 e2 = float2{s2 * b1.x - s1 * b2.x, s2 * b1.y - s1 * b2.y};
        v[0] = float2{v[0].x + a1.x + a2.x, v[0].y + a1.y + a2.y};
        v[1] = fft_add_i(m1, e1, sg); v[4] = fft_add_i(m1, e1, -sg);
        v[2] = fft_add_i(m2, e2, sg); v[3] = fft_add_i(m2, e2, -sg);
    }
}

// one pass over a bundle of C lines (C a power of two, log2 = cshift) by thread `tid` of `nthr`
MP_FFT_HD void fft_pass(const float2* in, float2* out, int N, int cshift, int r, int Ns, const float2* tw, bool inverse,
                        int tid, int nthr)
{
    const int M = N / r, total = M << cshift, cmask = (1 << cshift) - 1, tstep = N / (Ns * r);
    const float sg = inverse ? 1.f : -1.f;
    const bool pow2 = (Ns & (Ns - 1)) == 0;          // (the radices 4 and 2 come first: most passes)
    for (int w = tid; w < total; w += nthr) {
        const int j = w >> cshift, c = w & cmask;
        const int k = pow2 ? (j & (Ns - 1)) : j % Ns;
        float2 v[5];
        MP_FFT_UNROLL
        for (int q = 0; q < 5; ++q)
            if (q < r) v[q] = in[((j + q * M) << cshift) + c];
        if (Ns > 1) {
            MP_FFT_UNROLL
            for (int q = 1; q < 5; ++q)
                if (q < r) {
                    float2 t = tw[q * k * tstep];
                    if (inverse) t.y = -t.y;
                    v[q] = fft_cmul(v[q], t);
                }
        }
        fft_butterfly(v, r, sg);
        const int o = (j - k) * r + k;
        MP_FFT_UNROLL
        for (int q = 0; q < 5; ++q)
            if (q < r) out[((o + q * Ns) << cshift) + c] = v[q];
    }
}
