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
//   The per-pixel body, the workgroup's reduction and the Gauss-Newton step are in mp_ecc.h, shared with ecc_pooled.hip (3.22).
#include "../../include/multipoint_hip.h"
#include "mp_ecc.h"

namespace {

using namespace mp_ecc;

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

    double acc[S::N];
#pragma unroll
    for (int i = 0; i < S::N; ++i) acc[i] = 0.0;
    chunk_sums<K, false>(img, Ho, Wo, tpl, nullptr, HW, W, m, chunk, acc);
    block_sums<K>(acc, lds, partial, q, chunk);
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

// The decision of one problem from its sums s (LDS): DESIGN.md 3.21.  Every index is a compile-time constant.
template <int K>
__device__ void ecc_decide(const double* s, int HW, const EccOptions& o, EccState& st)
{
    using S = Sums<K>;
    const double n = s[0];
    if (n < o.min_valid * (double)HW) { st.status = MP_ECC_FEW_VALID; return; }
    bool ok = true;
#pragma unroll
    for (int i = 0; i < S::N; ++i) ok = ok && finite64(s[i]);
    if (!ok) { st.status = MP_ECC_NONFINITE; return; }
    const double mw = s[1] / n, mr = s[2] / n;
    const double ww = s[3] - n * mw * mw, rr = s[4] - n * mr * mr, corr = s[5] - n * mw * mr;
    const double rho = corr / (sqrt(ww) * sqrt(rr));
    if (!finite64(rho)) { st.status = MP_ECC_NONFINITE; return; }
    if (converged(rho, o, st)) return;

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
    step<K>(ww, corr, rho, A, ip, tp, o, st);
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
    start_state(T0 + 9 * q, pair[q], st);
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

void launch_ecc_sums(int K, const float* packed, int Ho, int Wo, const float* thermal, int H, int W, const int* pair,
                     const double* T, const EccState* state, int P, double* partial, hipStream_t s)
{
    const dim3 grid((unsigned)ecc_chunks(H, W), (unsigned)P);
    const float4* img = reinterpret_cast<const float4*>(packed);
    for_params(K, [&](auto k) {
        hipLaunchKernelGGL(ecc_sums_kernel<decltype(k)::value>, grid, dim3(THREADS), 0, s, img, Ho, Wo, thermal, H, W, pair, T, state,
                           partial);
    });
}

void launch_ecc_reduce(int K, const double* partial, int P, int chunks, double* sums, hipStream_t s)
{
    const dim3 grid((unsigned)((P * ecc_sum_count(K) + THREADS - 1) / THREADS));
    for_params(K, [&](auto k) {
        hipLaunchKernelGGL(ecc_reduce_kernel<decltype(k)::value>, grid, dim3(THREADS), 0, s, partial, P, chunks, sums);
    });
}

void launch_ecc_begin(const int* pair, const double* T0, int P, EccState* state, hipStream_t s)
{
    hipLaunchKernelGGL(ecc_begin_kernel, dim3((unsigned)((P + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, pair, T0, P, state);
}

void launch_ecc_solve(int K, const double* partial, int P, int chunks, int HW, EccOptions o, EccState* state, hipStream_t s)
{
    const dim3 grid((unsigned)((P + WAVES - 1) / WAVES));
    for_params(K, [&](auto k) {
        hipLaunchKernelGGL(ecc_solve_kernel<decltype(k)::value>, grid, dim3(THREADS), 0, s, partial, P, chunks, HW, o, state);
    });
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
