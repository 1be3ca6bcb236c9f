// Device code the per-pair ECC kernels (ecc.hip) and the pooled ones (ecc_pooled.hip, 3.22) share, so that the two
// cannot drift: the layout of the sums, the per-pixel terms and their accumulation, the workgroup's reduction, and the
// Gauss-Newton step from centred quantities.
#pragma once
#include "mp_common.h"
#include "mp_device.h"

#include <type_traits>

namespace mp_ecc {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;

template <int K> struct Sums {
    static constexpr int G = 6, GG = 6 + K, GW = GG + K * (K + 1) / 2, GR = GW + K, N = GR + K;
};
static_assert(Sums<8>::N == MP_ECC_MAX_SUMS, "the sums of the homography");

// launch(std::integral_constant<int, K>{}) for the parameter count of a model: 2, 4, 6, or 8 for the homography
template <class Launch>
void for_params(int K, Launch launch)
{
    if (K == 2) launch(std::integral_constant<int, 2>{});
    else if (K == 4) launch(std::integral_constant<int, 4>{});
    else if (K == 6) launch(std::integral_constant<int, 6>{});
    else launch(std::integral_constant<int, 8>{});
}

__device__ __forceinline__ float lerp2(float p00, float p01, float p10, float p11, float fx, float fy)
{
    const float top = fmaf(fx, p01 - p00, p00);
    const float bot = fmaf(fx, p11 - p10, p10);
    return fmaf(fy, bot - top, top);
}

// The sums of one chunk of MP_ECC_CHUNK template pixels into the calling lane's accumulators: lane t takes the pixels t, t + 256,
// ... of the chunk in that order.  MASKED: a template pixel whose `keep` byte is 0 (keep may be NULL) and an image sample with a
// flagged tap (packed .w != 0) are skipped like invalid ones.
template <int K, bool MASKED>
__device__ __forceinline__ void chunk_sums(const float4* __restrict__ img, int Ho, int Wo, const float* __restrict__ tpl,
                                           const unsigned char* __restrict__ keep, int HW, int W, const float (&m)[9], int chunk,
                                           double (&acc)[Sums<K>::N])
{
    using S = Sums<K>;
    const float xmax = (float)(Wo - 2), ymax = (float)(Ho - 2);
    const int base = chunk * MP_ECC_CHUNK;
    for (int i = threadIdx.x; i < MP_ECC_CHUNK; i += THREADS) {
        const int idx = base + i;
        if (idx >= HW) break;
        const int y = idx / W, x = idx - y * W;
        const float xf = (float)x, yf = (float)y;
        const float X = fmaf(m[0], xf, fmaf(m[1], yf, m[2]));
        const float Y = fmaf(m[3], xf, fmaf(m[4], yf, m[5]));
        const float D = fmaf(m[6], xf, fmaf(m[7], yf, m[8]));
        const float xs = X / D, ys = Y / D;
        const float x0f = floorf(xs), y0f = floorf(ys);
        if (!(x0f >= 0.f && y0f >= 0.f && x0f <= xmax && y0f <= ymax)) continue;     // (a NaN or an infinity fails here)
        if constexpr (MASKED) {
            if (keep && keep[idx] == 0) continue;
        }
        const float fx = xs - x0f, fy = ys - y0f;                                    // exact
        const float4* p = img + (size_t)(int)y0f * Wo + (int)x0f;
        const float4 p00 = p[0], p01 = p[1], p10 = p[Wo], p11 = p[Wo + 1];
        if constexpr (MASKED) {
            if (p00.w + p01.w + p10.w + p11.w != 0.f) continue;
        }
        const float w = lerp2(p00.x, p01.x, p10.x, p11.x, fx, fy);
        const float gx = lerp2(p00.y, p01.y, p10.y, p11.y, fx, fy);
        const float gy = lerp2(p00.z, p01.z, p10.z, p11.z, fx, fy);
        const float r = tpl[idx];
        float G[K];
        if constexpr (K == 2) {
            G[0] = gx; G[1] = gy;
        } else if constexpr (K == 4) {
            G[0] = fmaf(gx, xf, gy * yf);
            G[1] = fmaf(gy, xf, -(gx * yf));
            G[2] = gx; G[3] = gy;
        } else if constexpr (K == 6) {
            G[0] = gx * xf; G[1] = gx * yf; G[2] = gx;
            G[3] = gy * xf; G[4] = gy * yf; G[5] = gy;
        } else {
            const float id = 1.0f / D;
            const float a = gx * id, c = gy * id;
            const float t = -fmaf(a, xs, c * ys);
            G[0] = a * xf; G[1] = a * yf; G[2] = a;
            G[3] = c * xf; G[4] = c * yf; G[5] = c;
            G[6] = t * xf; G[7] = t * yf;
        }
        const double wd = (double)w, rd = (double)r;
        double gd[K];
#pragma unroll
        for (int k = 0; k < K; ++k) gd[k] = (double)G[k];
        acc[0] += 1.0;
        acc[1] += wd;
        acc[2] += rd;
        acc[3] = fma(wd, wd, acc[3]);
        acc[4] = fma(rd, rd, acc[4]);
        acc[5] = fma(wd, rd, acc[5]);
        int at = S::GG;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            acc[S::G + k] += gd[k];
#pragma unroll
            for (int l = k; l < K; ++l, ++at) acc[at] = fma(gd[k], gd[l], acc[at]);
            acc[S::GW + k] = fma(gd[k], wd, acc[S::GW + k]);
            acc[S::GR + k] = fma(gd[k], rd, acc[S::GR + k]);
        }
    }
}

// The workgroup's sums from its lanes' accumulators: butterflies inside a wave, (w0 + w1) + (w2 + w3) across the four waves, into
// partial [q][chunk][sum] of a grid (chunks, problems).
template <int K>
__device__ __forceinline__ void block_sums(const double (&acc)[Sums<K>::N], double (&lds)[WAVES][Sums<K>::N],
                                           double* __restrict__ partial, int q, int chunk)
{
    using S = Sums<K>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < S::N; ++i) {
        double v = acc[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) lds[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < S::N) {
        const int i = threadIdx.x;
        const double v = (lds[0][i] + lds[1][i]) + (lds[2][i] + lds[3][i]);
        partial[((size_t)q * gridDim.x + chunk) * S::N + i] = v;
    }
}

// The stop rule at a finite rho: true when the iteration ends here.
__device__ __forceinline__ bool converged(double rho, const EccOptions& o, EccState& st)
{
    st.rho = rho;
    if (fabs(rho - st.rho_prev) < o.eps) { st.status = MP_ECC_OK; st.converged = 1; return true; }
    return false;
}

// The Gauss-Newton step behind the stop rule: the Cholesky factorisation of A (its lower triangle is filled), lambda, the
// additive update of st.T, maxiter.  ww, corr, ip, tp are centred.  Every index is a compile-time constant.
template <int K>
__device__ __forceinline__ void step(double ww, double corr, double rho, double (&A)[K][K], double (&ip)[K], double (&tp)[K],
                                     const EccOptions& o, EccState& st)
{
    // Cholesky A = L L^T in place (lower triangle), y = L^-1 ip, z = L^-1 tp
    bool positive = true;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
        positive = positive && d > 0.0;
        const double l = sqrt(d);
        A[j][j] = l;
#pragma unroll
        for (int i = j + 1; i < K; ++i) {
            double v = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= A[i][k] * A[j][k];
            A[i][j] = v / l;
        }
    }
    if (!positive) { st.status = MP_ECC_NOT_POSITIVE; return; }
    double yy = 0.0, zy = 0.0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        double a = ip[i], b = tp[i];
#pragma unroll
        for (int k = 0; k < i; ++k) { a -= A[i][k] * ip[k]; b -= A[i][k] * tp[k]; }
        ip[i] = a / A[i][i];
        tp[i] = b / A[i][i];
        yy += ip[i] * ip[i];
        zy += tp[i] * ip[i];
    }
    const double lam_n = ww - yy, lam_d = corr - zy;
    if (!(finite64(lam_n) && finite64(lam_d))) { st.status = MP_ECC_NONFINITE; return; }
    if (lam_d <= 0.0) { st.status = MP_ECC_LAMBDA; return; }
    const double lam = lam_n / lam_d;
    // dp = L^-T (lam z - y)
    double dp[K];
#pragma unroll
    for (int i = K - 1; i >= 0; --i) {
        double v = lam * tp[i] - ip[i];
#pragma unroll
        for (int k = i + 1; k < K; ++k) v -= A[k][i] * dp[k];
        dp[i] = v / A[i][i];
    }
    double T[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) T[i] = st.T[i];
    if constexpr (K == 2) {
        T[2] += dp[0]; T[5] += dp[1];
    } else if constexpr (K == 4) {
        const double a = T[0] + dp[0], b = T[3] + dp[1];
        T[0] = a; T[1] = -b; T[3] = b; T[4] = a;
        T[2] += dp[2]; T[5] += dp[3];
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) T[k] += dp[k];
    }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) ok = ok && finite64(T[i]);
    if (!ok) { st.status = MP_ECC_NONFINITE; return; }
#pragma unroll
    for (int i = 0; i < 9; ++i) st.T[i] = T[i];
    st.rho_prev = rho;
    st.nit += 1;
    if (st.nit >= o.maxiter) st.status = MP_ECC_OK;
}

// A start matrix divided by its last entry into a fresh state; a non-finite one fails at once.
__device__ __forceinline__ void start_state(const double* __restrict__ T0, int pair, EccState& st)
{
    const double d = T0[8];
    for (int i = 0; i < 9; ++i) st.T[i] = T0[i] / d;
    st.T[8] = 1.0;
    st.rho = st.rho_prev = __longlong_as_double(0x7ff8000000000000LL);
    st.pair = pair;
    st.nit = 0;
    st.status = MP_ECC_RUNNING;
    st.converged = 0;
    bool ok = true;
    for (int i = 0; i < 9; ++i) ok = ok && finite64(st.T[i]);
    if (!ok) st.status = MP_ECC_NONFINITE;
}

}  // namespace mp_ecc
