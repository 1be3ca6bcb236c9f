// ECC direct alignment: Gauss-Newton maximisation of the enhanced correlation coefficient between a template
// (thermal feature frame) and an image (optical feature frame) under a translation, similarity, affine map or homography.
//
//   ecc_feature_kernel   one lane per pixel: the magnitude of the central differences of a blurred frame (or a copy of it).
//   ecc_pack_kernel      one lane per pixel: (f, gx, gy, 0) of a feature frame as one float4, so that a bilinear tap of the
//                        sums pass is one 16-byte load (4 per template pixel instead of 12).
//   ecc_sums_kernel<K>   the hot path, one launch per iteration over (pixel chunk, problem).  A workgroup owns MP_ECC_CHUNK
//                        consecutive template pixels, lane t the pixels t, t + 256, ... of them in that order.  Coordinates are
//                        fp32 fmafs of the float64 matrix rounded once; the sample, its gradient and the Jacobian columns G_k
//                        are fp32; every sum is a float64 accumulator in a register (K is a template parameter so that all of
//                        them have compile-time indices), fed with the exact float64 products of the fp32 factors.  Lanes
//                        reduce by butterflies, the four waves through LDS, and the workgroup writes its [problem][chunk][sum]
//                        partials.  No atomics: the order of every addition is fixed by (problem, pixel index) alone, so a
//                        problem has the same bits alone, in any batch and from run to run.
//   ecc_solve_kernel<K>  one wave per problem: its lanes add the chunks' partials in chunk order (coalesced over the sums),
//                        lane 0 centres them, factorises G^T G (Cholesky), forms lambda and the update, applies the stop and
//                        failure rules and writes the next iterate.  All float64, all loops unrolled over K.
//   A finished problem's workgroups and wave leave at once.
#include "../../include/multipoint_hip.h"
#include "mp_common.h"
#include "mp_device.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;

template <int K> struct Sums {
    static constexpr int G = 6, GG = 6 + K, GW = GG + K * (K + 1) / 2, GR = GW + K, N = GR + K;
};
static_assert(Sums<8>::N == MP_ECC_MAX_SUMS, "the sums of the homography");

__global__ __launch_bounds__(THREADS) void ecc_feature_kernel(const float* __restrict__ in, int H, int W, int gradient,
                                                              float* __restrict__ out)
{
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= H * W) return;
    const float* f = in + (size_t)blockIdx.y * H * W;
    float v = f[idx];
    if (gradient) {
        const int y = idx / W, x = idx - y * W;
        const float gx = 0.5f * (f[y * W + reflect101(x + 1, W)] - f[y * W + reflect101(x - 1, W)]);
        const float gy = 0.5f * (f[reflect101(y + 1, H) * W + x] - f[reflect101(y - 1, H) * W + x]);
        v = sqrtf(fmaf(gx, gx, gy * gy));
    }
    out[(size_t)blockIdx.y * H * W + idx] = v;
}

__global__ __launch_bounds__(THREADS) void ecc_pack_kernel(const float* __restrict__ in, int H, int W, float4* __restrict__ out)
{
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= H * W) return;
    const float* f = in + (size_t)blockIdx.y * H * W;
    const int y = idx / W, x = idx - y * W;
    const float gx = 0.5f * (f[y * W + reflect101(x + 1, W)] - f[y * W + reflect101(x - 1, W)]);
    const float gy = 0.5f * (f[reflect101(y + 1, H) * W + x] - f[reflect101(y - 1, H) * W + x]);
    out[(size_t)blockIdx.y * H * W + idx] = make_float4(f[idx], gx, gy, 0.f);
}

__device__ __forceinline__ float lerp2(float p00, float p01, float p10, float p11, float fx, float fy)
{
    const float top = fmaf(fx, p01 - p00, p00);
    const float bot = fmaf(fx, p11 - p10, p10);
    return fmaf(fy, bot - top, top);
}

template <int K>
__global__ __launch_bounds__(THREADS) void ecc_sums_kernel(const float4* __restrict__ packed, int Ho, int Wo,
                                                           const float* __restrict__ thermal, int H, int W,
                                                           const int* __restrict__ pair, const double* __restrict__ T,
                                                           const EccState* __restrict__ state, double* __restrict__ partial)
{
    using S = Sums<K>;
    __shared__ double lds[WAVES][S::N];
    const int q = blockIdx.y, chunk = blockIdx.x;
    const double* Tq;
    int b;
    if (T) {
        Tq = T + 9 * (size_t)q;
        b = pair[q];
    } else {
        if (state[q].status != MP_ECC_RUNNING) return;
        Tq = state[q].T;
        b = state[q].pair;
    }
    float m[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = (float)Tq[i];
    const int HW = H * W;
    const float4* img = packed + (size_t)b * Ho * Wo;
    const float* tpl = thermal + (size_t)b * HW;
    const float xmax = (float)(Wo - 2), ymax = (float)(Ho - 2);

    double acc[S::N];
#pragma unroll
    for (int i = 0; i < S::N; ++i) acc[i] = 0.0;

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
        const float fx = xs - x0f, fy = ys - y0f;                                    // exact
        const float4* p = img + (size_t)(int)y0f * Wo + (int)x0f;
        const float4 p00 = p[0], p01 = p[1], p10 = p[Wo], p11 = p[Wo + 1];
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

template <int K>
__global__ __launch_bounds__(THREADS) void ecc_reduce_kernel(const double* __restrict__ partial, int P, int chunks,
                                                             double* __restrict__ sums)
{
    constexpr int N = Sums<K>::N;
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= P * N) return;
    const int q = idx / N, i = idx - q * N;
    double v = 0.0;
    for (int c = 0; c < chunks; ++c) v += partial[((size_t)q * chunks + c) * N + i];
    sums[idx] = v;
}

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }

// The decision of one problem from its sums s (LDS): DESIGN.md 3.21.  Every index is a compile-time constant.
template <int K>
__device__ void ecc_decide(const double* s, int HW, const EccOptions& o, EccState& st)
{
    using S = Sums<K>;
    const double n = s[0];
    if (n < o.min_valid * (double)HW) { st.status = MP_ECC_FEW_VALID; return; }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < S::N; ++i) ok = ok && finite_d(s[i]);
    if (!ok) { st.status = MP_ECC_NONFINITE; return; }
    const double mw = s[1] / n, mr = s[2] / n;
    const double ww = s[3] - n * mw * mw, rr = s[4] - n * mr * mr, corr = s[5] - n * mw * mr;
    const double rho = corr / (sqrt(ww) * sqrt(rr));
    if (!finite_d(rho)) { st.status = MP_ECC_NONFINITE; return; }
    st.rho = rho;
    if (fabs(rho - st.rho_prev) < o.eps) { st.status = MP_ECC_OK; st.converged = 1; return; }

    double A[K][K], ip[K], tp[K];
    {
        int at = S::GG;
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int l = k; l < K; ++l, ++at) A[l][k] = s[at];
            ip[k] = s[S::GW + k] - mw * s[S::G + k];
            tp[k] = s[S::GR + k] - mr * s[S::G + k];
        }
    }
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
    if (!(finite_d(lam_n) && finite_d(lam_d))) { st.status = MP_ECC_NONFINITE; return; }
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
    ok = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) ok = ok && finite_d(T[i]);
    if (!ok) { st.status = MP_ECC_NONFINITE; return; }
#pragma unroll
    for (int i = 0; i < 9; ++i) st.T[i] = T[i];
    st.rho_prev = rho;
    st.nit += 1;
    if (st.nit >= o.maxiter) st.status = MP_ECC_OK;
}

template <int K>
__global__ __launch_bounds__(THREADS) void ecc_solve_kernel(const double* __restrict__ partial, int P, int chunks, int HW,
                                                            EccOptions o, EccState* __restrict__ state)
{
    constexpr int N = Sums<K>::N;
    __shared__ double lds[WAVES][N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * WAVES + wave;
    const bool live = q < P && state[q].status == MP_ECC_RUNNING;
    if (live) {
        for (int i = lane; i < N; i += 64) {
            double v = 0.0;
            for (int c = 0; c < chunks; ++c) v += partial[((size_t)q * chunks + c) * N + i];
            lds[wave][i] = v;
        }
    }
    __syncthreads();
    if (live && lane == 0) ecc_decide<K>(lds[wave], HW, o, state[q]);
}

__global__ __launch_bounds__(THREADS) void ecc_begin_kernel(const int* __restrict__ pair, const double* __restrict__ T0, int P,
                                                            EccState* __restrict__ state)
{
    const int q = blockIdx.x * THREADS + threadIdx.x;
    if (q >= P) return;
    EccState st;
    const double d = T0[9 * q + 8];
    for (int i = 0; i < 9; ++i) st.T[i] = T0[9 * q + i] / d;
    st.T[8] = 1.0;
    st.rho = st.rho_prev = __longlong_as_double(0x7ff8000000000000LL);
    st.pair = pair[q];
    st.nit = 0;
    st.status = MP_ECC_RUNNING;
    st.converged = 0;
    bool ok = true;
    for (int i = 0; i < 9; ++i) ok = ok && finite_d(st.T[i]);
    if (!ok) st.status = MP_ECC_NONFINITE;
    state[q] = st;
}

__global__ __launch_bounds__(THREADS) void ecc_live_kernel(const EccState* __restrict__ state, int P, int* __restrict__ live)
{
    int total = 0;
    for (int base = 0; base < P; base += THREADS) {
        const int q = base + threadIdx.x;
        total += __syncthreads_count(q < P && state[q].status == MP_ECC_RUNNING);
    }
    if (threadIdx.x == 0) *live = total;
}

__global__ __launch_bounds__(THREADS) void ecc_result_kernel(const EccState* __restrict__ state, int P, double* __restrict__ T,
                                                             double* __restrict__ rho, int* __restrict__ nit,
                                                             int* __restrict__ status, int* __restrict__ converged)
{
    const int q = blockIdx.x * THREADS + threadIdx.x;
    if (q >= P) return;
    for (int i = 0; i < 9; ++i) T[9 * q + i] = state[q].T[i];
    rho[q] = state[q].rho;
    nit[q] = state[q].nit;
    status[q] = state[q].status;
    converged[q] = state[q].converged;
}

}  // namespace

int ecc_model_params(int model)
{
    switch (model) {
    case MP_MODEL_HOMOGRAPHY: return 8;
    case MP_MODEL_SIMILARITY: return 4;
    case MP_MODEL_AFFINE: return 6;
    case MP_MODEL_TRANSLATION: return 2;
    default: return 0;
    }
}

int ecc_sum_count(int K) { return 6 + K + K * (K + 1) / 2 + 2 * K; }

int ecc_chunks(int H, int W) { return (H * W + MP_ECC_CHUNK - 1) / MP_ECC_CHUNK; }

void launch_ecc_feature(const float* blurred, int n, int H, int W, int gradient, float* feat, hipStream_t s)
{
    const dim3 grid((unsigned)((H * W + THREADS - 1) / THREADS), (unsigned)n);
    hipLaunchKernelGGL(ecc_feature_kernel, grid, dim3(THREADS), 0, s, blurred, H, W, gradient, feat);
}

void launch_ecc_pack(const float* feat, int n, int H, int W, float* packed, hipStream_t s)
{
    const dim3 grid((unsigned)((H * W + THREADS - 1) / THREADS), (unsigned)n);
    hipLaunchKernelGGL(ecc_pack_kernel, grid, dim3(THREADS), 0, s, feat, H, W, reinterpret_cast<float4*>(packed));
}

#define MP_ECC_BY_K(K, CALL)            \
    switch (K) {                        \
    case 2: { CALL(2); break; }         \
    case 4: { CALL(4); break; }         \
    case 6: { CALL(6); break; }         \
    default: { CALL(8); break; }        \
    }

void launch_ecc_sums(int K, const float* packed, int Ho, int Wo, const float* thermal, int H, int W, const int* pair,
                     const double* T, const EccState* state, int P, double* partial, hipStream_t s)
{
    const dim3 grid((unsigned)ecc_chunks(H, W), (unsigned)P);
    const float4* img = reinterpret_cast<const float4*>(packed);
#define MP_ECC_CALL(KK) \
    hipLaunchKernelGGL(ecc_sums_kernel<KK>, grid, dim3(THREADS), 0, s, img, Ho, Wo, thermal, H, W, pair, T, state, partial)
    MP_ECC_BY_K(K, MP_ECC_CALL)
#undef MP_ECC_CALL
}

void launch_ecc_reduce(int K, const double* partial, int P, int chunks, double* sums, hipStream_t s)
{
    const dim3 grid((unsigned)((P * ecc_sum_count(K) + THREADS - 1) / THREADS));
#define MP_ECC_CALL(KK) hipLaunchKernelGGL(ecc_reduce_kernel<KK>, grid, dim3(THREADS), 0, s, partial, P, chunks, sums)
    MP_ECC_BY_K(K, MP_ECC_CALL)
#undef MP_ECC_CALL
}

void launch_ecc_begin(const int* pair, const double* T0, int P, EccState* state, hipStream_t s)
{
    hipLaunchKernelGGL(ecc_begin_kernel, dim3((unsigned)((P + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, pair, T0, P, state);
}

void launch_ecc_solve(int K, const double* partial, int P, int chunks, int HW, EccOptions o, EccState* state, hipStream_t s)
{
    const dim3 grid((unsigned)((P + WAVES - 1) / WAVES));
#define MP_ECC_CALL(KK) hipLaunchKernelGGL(ecc_solve_kernel<KK>, grid, dim3(THREADS), 0, s, partial, P, chunks, HW, o, state)
    MP_ECC_BY_K(K, MP_ECC_CALL)
#undef MP_ECC_CALL
}

void launch_ecc_live(const EccState* state, int P, int* live, hipStream_t s)
{
    hipLaunchKernelGGL(ecc_live_kernel, dim3(1), dim3(THREADS), 0, s, state, P, live);
}

void launch_ecc_result(const EccState* state, int P, double* T, double* rho, int* nit, int* status, int* converged, hipStream_t s)
{
    hipLaunchKernelGGL(ecc_result_kernel, dim3((unsigned)((P + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, state, P, T, rho,
                       nit, status, converged);
}
