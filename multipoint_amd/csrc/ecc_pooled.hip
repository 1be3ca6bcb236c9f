// Pooled ECC: the Gauss-Newton maximisation of ecc.hip with ONE transform per group of pairs -- the correlation
// coefficient of the concatenation of the group's centred per-pair feature vectors -- and static masks.
//
//   ecc_grow_rows / _cols   one lane per pixel: a use-mask with its excluded set grown by a Chebyshev radius R (a box, so rows
//                           first, then columns), clipped at the frame.
//   ecc_static_update       running minimum and maximum per pixel over a batch of frames; ecc_static_finish: min == max -> 0.
//   ecc_flag_kernel         1.0f into .w of the packed plane where a use-mask is 0: a bilinear tap of the sums pass then carries
//                           its own flag.
//   ecc_pooled_sums<K>      the hot path, one launch per iteration over (pixel chunk, pair): the per-pixel body, the ownership and
//                           the order of additions of ecc_sums_kernel (mp_ecc.h), at the transform of the pair's GROUP, with
//                           the two mask tests.  The workgroups of a finished group or an inactive pair leave at once; every
//                           other workgroup writes its partials, zeros when each of its pixels was skipped.
//   ecc_pooled_pair<K>      one wave per pair: adds the chunks in chunk order, centres, decides the pair's inclusion, writes its
//                           centred quantities and its record (rho_i, n_i, included).
//   ecc_pooled_solve<K>     one wave per group: its lanes add the included pairs' quantities in ascending pair index (coalesced
//                           over the entries), lane 0 takes the step of 3.21 (mp_ecc.h) and writes the next T_g.
//   No atomics: a group's bits depend on its own ordered pair list alone.
#include "../../include/multipoint_hip.h"
#include "mp_ecc.h"

namespace {

using namespace mp_ecc;

template <int K> struct Quant {
    static constexpr int A = 3, IP = 3 + K * (K + 1) / 2, TP = IP + K, N = TP + K;
};
static_assert(Quant<8>::N == MP_ECC_POOLED_MAX_Q, "the centred quantities of the homography");

// dir 0: along a row, 1: along a column.  out = 1 iff no pixel within R of this one along the line is 0 in `in`.
__global__ __launch_bounds__(THREADS) void ecc_grow_kernel(const unsigned char* __restrict__ in, int H, int W, int R, int dir,
                                                           unsigned char* __restrict__ out)
{
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= H * W) return;
    const unsigned char* f = in + (size_t)blockIdx.y * H * W;
    const int y = idx / W, x = idx - y * W;
    const int at = dir ? y : x, len = dir ? H : W, stride = dir ? W : 1;
    const int lo = max(at - min(R, len), 0), hi = min(at + min(R, len), len - 1);      // (min: R may exceed the frame)
    const unsigned char* line = f + (dir ? x : y * W);
    int keep = 1;
    for (int i = lo; i <= hi; ++i) keep &= line[(size_t)i * stride] != 0;
    out[(size_t)blockIdx.y * H * W + idx] = (unsigned char)keep;
}

__global__ __launch_bounds__(THREADS) void ecc_static_update_kernel(const float* __restrict__ frames, int n, int HW, int first,
                                                                    float* __restrict__ lo, float* __restrict__ hi)
{
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= HW) return;
    float a = first ? frames[idx] : lo[idx], b = first ? frames[idx] : hi[idx];
    for (int i = first ? 1 : 0; i < n; ++i) {
        const float v = frames[(size_t)i * HW + idx];
        a = v < a ? v : a;
        b = v > b ? v : b;
    }
    lo[idx] = a;
    hi[idx] = b;
}

__global__ __launch_bounds__(THREADS) void ecc_static_finish_kernel(const float* __restrict__ lo, const float* __restrict__ hi, int HW,
                                                                    unsigned char* __restrict__ mask)
{
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= HW) return;
    mask[idx] = lo[idx] == hi[idx] ? 0 : 1;
}

__global__ __launch_bounds__(THREADS) void ecc_flag_kernel(float4* __restrict__ packed, int HW, const unsigned char* __restrict__ mask)
{
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= HW) return;
    if (mask[idx] == 0) packed[(size_t)blockIdx.y * HW + idx].w = 1.0f;
}

template <int K>
__global__ __launch_bounds__(THREADS) void ecc_pooled_sums_kernel(const float4* __restrict__ packed, int Ho, int Wo,
                                                                  const float* __restrict__ thermal, int H, int W,
                                                                  const unsigned char* __restrict__ tmasks,
                                                                  const int* __restrict__ tmask, const int* __restrict__ group,
                                                                  const int* __restrict__ active, const double* __restrict__ T,
                                                                  const EccGroup* __restrict__ groups, double* __restrict__ partial)
{
    using S = Sums<K>;
    __shared__ double lds[WAVES][S::N];
    const int p = blockIdx.y, chunk = blockIdx.x;
    const int g = group[p];
    const double* Tg;
    if (T) {
        Tg = T + 9 * (size_t)g;
    } else {
        if (!active[p] || groups[g].s.status != MP_ECC_RUNNING) return;
        Tg = groups[g].s.T;
    }
    float m[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = (float)Tg[i];
    const int plane = tmask[g];
    const unsigned char* keep = plane >= 0 ? tmasks + (size_t)plane * H * W : nullptr;
    const int HW = H * W;
    const float4* img = packed + (size_t)p * Ho * Wo;
    const float* tpl = thermal + (size_t)p * HW;

    double acc[S::N];
#pragma unroll
    for (int i = 0; i < S::N; ++i) acc[i] = 0.0;
    chunk_sums<K, true>(img, Ho, Wo, tpl, keep, HW, W, m, chunk, acc);
    block_sums<K>(acc, lds, partial, p, chunk);
}

// one block per group: the start state, and how many template pixels the group's mask keeps
__global__ __launch_bounds__(THREADS) void ecc_pooled_begin_kernel(const double* __restrict__ T0, const unsigned char* __restrict__ tmasks,
                                                                   const int* __restrict__ tmask, int HW, EccGroup* __restrict__ groups)
{
    const int g = blockIdx.x;
    const int plane = tmask[g];
    int kept = 0;
    if (plane >= 0) {
        const unsigned char* keep = tmasks + (size_t)plane * HW;
        for (int base = 0; base < HW; base += THREADS) {
            const int i = base + threadIdx.x;
            kept += __syncthreads_count(i < HW && keep[i] != 0);
        }
    } else {
        kept = HW;
    }
    if (threadIdx.x == 0) {
        EccGroup gr;
        start_state(T0 + 9 * (size_t)g, g, gr.s);
        gr.M = kept;
        gr.n_included = 0;
        groups[g] = gr;
    }
}

__global__ __launch_bounds__(THREADS) void ecc_pooled_clear_kernel(EccPairRec* __restrict__ recs, int P)
{
    const int p = blockIdx.x * THREADS + threadIdx.x;
    if (p >= P) return;
    EccPairRec r;
    r.rho = __longlong_as_double(0x7ff8000000000000LL);
    r.n = 0.0;
    r.included = 0;
    r.pad = 0;
    recs[p] = r;
}

template <int K>
__global__ __launch_bounds__(THREADS) void ecc_pooled_pair_kernel(const double* __restrict__ partial, int P, int chunks,
                                                                  const int* __restrict__ group, const int* __restrict__ active,
                                                                  EccOptions o, const EccGroup* __restrict__ groups,
                                                                  EccPairRec* __restrict__ recs, double* __restrict__ quant)
{
    using S = Sums<K>;
    using Q = Quant<K>;
    __shared__ double lds[WAVES][S::N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.x * WAVES + wave;
    bool live = false;
    int M = 0;
    if (p < P && active[p]) {
        const EccGroup& gr = groups[group[p]];
        live = gr.s.status == MP_ECC_RUNNING;
        M = gr.M;
    }
    if (live) {
        for (int i = lane; i < S::N; i += 64) {
            const double* src = partial + (size_t)p * chunks * S::N + i;
            double v = 0.0;
            int c = 0;
            for (; c + 8 <= chunks; c += 8) {                  // eight loads in flight, added in chunk order
                double t[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) t[u] = src[(size_t)(c + u) * S::N];
#pragma unroll
                for (int u = 0; u < 8; ++u) v += t[u];
            }
            for (; c < chunks; ++c) v += src[(size_t)c * S::N];
            lds[wave][i] = v;
        }
    }
    __syncthreads();
    if (!live) return;
    const double* s = lds[wave];
    bool ok = true;
    for (int i = lane; i < S::N; i += 64) ok = ok && finite64(s[i]);
    ok = __all(ok);
    const double n = s[0];
    const double mw = s[1] / n, mr = s[2] / n;                                     // (n == 0: never used, the pair is out)
    const double ww = s[3] - n * mw * mw, rr = s[4] - n * mr * mr, corr = s[5] - n * mw * mr;
    const bool in = ok && n > 0.0 && n >= o.min_valid * (double)M && ww > 0.0 && rr > 0.0;
    double* q = quant + (size_t)p * MP_ECC_POOLED_MAX_Q;
    if (in) {
        for (int i = lane; i < Q::N; i += 64) {
            double v;
            if (i == 0) v = ww;
            else if (i == 1) v = rr;
            else if (i == 2) v = corr;
            else if (i < Q::IP) v = s[S::GG + (i - Q::A)];
            else if (i < Q::TP) v = s[S::GW + (i - Q::IP)] - mw * s[S::G + (i - Q::IP)];
            else v = s[S::GR + (i - Q::TP)] - mr * s[S::G + (i - Q::TP)];
            q[i] = v;
        }
    }
    if (lane == 0) {
        EccPairRec r;
        r.rho = in ? corr / (sqrt(ww) * sqrt(rr)) : __longlong_as_double(0x7ff8000000000000LL);
        r.n = ok ? n : 0.0;
        r.included = in ? 1 : 0;
        r.pad = 0;
        recs[p] = r;
    }
}

template <int K>
__global__ __launch_bounds__(THREADS) void ecc_pooled_solve_kernel(const int* __restrict__ offsets, const int* __restrict__ list,
                                                                   const EccPairRec* __restrict__ recs,
                                                                   const double* __restrict__ quant, int G, EccOptions o,
                                                                   EccGroup* __restrict__ groups)
{
    using Q = Quant<K>;
    __shared__ double lds[WAVES][Q::N];
    __shared__ int count[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = blockIdx.x * WAVES + wave;
    const bool live = g < G && groups[g].s.status == MP_ECC_RUNNING;
    if (live) {
        const int first = offsets[g], last = offsets[g + 1];
        double v = 0.0;
        int n = 0;
        // 64 pairs at a time: lane l looks up pair l of the batch, then every lane adds its entry of the included ones in list
        // order, eight loads in flight.  An excluded pair contributes a literal 0.0, which leaves v (never -0.0) as it is.
        for (int base = first; base < last; base += 64) {
            const int j = base + lane;
            const int p = j < last ? list[j] : 0;
            const int inc = j < last ? recs[p].included : 0;
            n += __popcll(__ballot(inc));
            const int cnt = min(64, last - base);
            for (int u0 = 0; u0 < cnt; u0 += 8) {
                double t[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int pu = __shfl(p, u0 + u, 64), iu = __shfl(inc, u0 + u, 64);
                    t[u] = (iu && lane < Q::N) ? quant[(size_t)pu * MP_ECC_POOLED_MAX_Q + lane] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) v += t[u];
            }
        }
        if (lane < Q::N) lds[wave][lane] = v;
        if (lane == 0) count[wave] = n;
    }
    __syncthreads();
    if (!(live && lane == 0)) return;
    EccState& st = groups[g].s;
    groups[g].n_included = count[wave];
    if (count[wave] == 0) { st.status = MP_ECC_FEW_VALID; return; }
    const double* s = lds[wave];
    const double ww = s[0], rr = s[1], corr = s[2];
    const double rho = corr / (sqrt(ww) * sqrt(rr));
    if (!finite64(rho)) { st.status = MP_ECC_NONFINITE; return; }
    if (converged(rho, o, st)) return;
    double A[K][K], ip[K], tp[K];
    {
        int at = Q::A;
#pragma unroll
        for (int k = 0; k < K; ++k) {
#pragma unroll
            for (int l = k; l < K; ++l, ++at) A[l][k] = s[at];
            ip[k] = s[Q::IP + k];
            tp[k] = s[Q::TP + k];
        }
    }
    step<K>(ww, corr, rho, A, ip, tp, o, st);
}

__global__ __launch_bounds__(THREADS) void ecc_pooled_live_kernel(const EccGroup* __restrict__ groups, int G, int* __restrict__ live)
{
    int total = 0;
    for (int base = 0; base < G; base += THREADS) {
        const int g = base + threadIdx.x;
        total += __syncthreads_count(g < G && groups[g].s.status == MP_ECC_RUNNING);
    }
    if (threadIdx.x == 0) *live = total;
}

__global__ __launch_bounds__(THREADS) void ecc_pooled_result_kernel(const EccGroup* __restrict__ groups, int G,
                                                                    const EccPairRec* __restrict__ recs, int P, double* __restrict__ T,
                                                                    double* __restrict__ rho, int* __restrict__ nit,
                                                                    int* __restrict__ status, int* __restrict__ converged,
                                                                    int* __restrict__ n_included, double* __restrict__ rho_pair,
                                                                    double* __restrict__ n_pair, int* __restrict__ included)
{
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i < G) {
        const EccGroup& gr = groups[i];
        for (int k = 0; k < 9; ++k) T[9 * i + k] = gr.s.T[k];
        rho[i] = gr.s.rho;
        nit[i] = gr.s.nit;
        status[i] = gr.s.status;
        converged[i] = gr.s.converged;
        n_included[i] = gr.n_included;
    }
    if (i < P) {
        rho_pair[i] = recs[i].rho;
        n_pair[i] = recs[i].n;
        included[i] = recs[i].included;
    }
}

unsigned blocks(long long n) { return (unsigned)((n + THREADS - 1) / THREADS); }

}  // namespace

void launch_ecc_mask_grow(const unsigned char* in, int n, int H, int W, int R, unsigned char* tmp, unsigned char* out, hipStream_t s)
{
    const dim3 grid(blocks((long long)H * W), (unsigned)n);
    hipLaunchKernelGGL(ecc_grow_kernel, grid, dim3(THREADS), 0, s, in, H, W, R, 0, tmp);
    hipLaunchKernelGGL(ecc_grow_kernel, grid, dim3(THREADS), 0, s, (const unsigned char*)tmp, H, W, R, 1, out);
}

void launch_ecc_static_update(const float* frames, int n, int HW, int first, float* lo, float* hi, hipStream_t s)
{
    hipLaunchKernelGGL(ecc_static_update_kernel, dim3(blocks(HW)), dim3(THREADS), 0, s, frames, n, HW, first, lo, hi);
}

void launch_ecc_static_finish(const float* lo, const float* hi, int HW, unsigned char* mask, hipStream_t s)
{
    hipLaunchKernelGGL(ecc_static_finish_kernel, dim3(blocks(HW)), dim3(THREADS), 0, s, lo, hi, HW, mask);
}

void launch_ecc_flag_packed(float* packed, int n, int HW, const unsigned char* mask, hipStream_t s)
{
    hipLaunchKernelGGL(ecc_flag_kernel, dim3(blocks(HW), (unsigned)n), dim3(THREADS), 0, s, reinterpret_cast<float4*>(packed), HW, mask);
}

void launch_ecc_pooled_sums(int K, const float* packed, int Ho, int Wo, const float* thermal, int H, int W,
                            const unsigned char* tmasks, const int* tmask, const int* group, const int* active, const double* T,
                            const EccGroup* groups, int P, double* partial, hipStream_t s)
{
    const dim3 grid((unsigned)ecc_chunks(H, W), (unsigned)P);
    const float4* img = reinterpret_cast<const float4*>(packed);
    for_params(K, [&](auto k) {
        hipLaunchKernelGGL(ecc_pooled_sums_kernel<decltype(k)::value>, grid, dim3(THREADS), 0, s, img, Ho, Wo, thermal, H, W, tmasks,
                           tmask, group, active, T, groups, partial);
    });
}

void launch_ecc_pooled_begin(const double* T0, const unsigned char* tmasks, const int* tmask, int HW, int G, int P, EccGroup* groups,
                             EccPairRec* recs, hipStream_t s)
{
    hipLaunchKernelGGL(ecc_pooled_begin_kernel, dim3((unsigned)G), dim3(THREADS), 0, s, T0, tmasks, tmask, HW, groups);
    hipLaunchKernelGGL(ecc_pooled_clear_kernel, dim3(blocks(P)), dim3(THREADS), 0, s, recs, P);
}

void launch_ecc_pooled_pair(int K, const double* partial, int P, int chunks, const int* group, const int* active, EccOptions o,
                            const EccGroup* groups, EccPairRec* recs, double* quant, hipStream_t s)
{
    const dim3 grid((unsigned)((P + WAVES - 1) / WAVES));
    for_params(K, [&](auto k) {
        hipLaunchKernelGGL(ecc_pooled_pair_kernel<decltype(k)::value>, grid, dim3(THREADS), 0, s, partial, P, chunks, group, active, o,
                           groups, recs, quant);
    });
}

void launch_ecc_pooled_solve(int K, const int* offsets, const int* list, const EccPairRec* recs, const double* quant, int G,
                             EccOptions o, EccGroup* groups, hipStream_t s)
{
    const dim3 grid((unsigned)((G + WAVES - 1) / WAVES));
    for_params(K, [&](auto k) {
        hipLaunchKernelGGL(ecc_pooled_solve_kernel<decltype(k)::value>, grid, dim3(THREADS), 0, s, offsets, list, recs, quant, G, o,
                           groups);
    });
}

void launch_ecc_pooled_live(const EccGroup* groups, int G, int* live, hipStream_t s)
{
    hipLaunchKernelGGL(ecc_pooled_live_kernel, dim3(1), dim3(THREADS), 0, s, groups, G, live);
}

void launch_ecc_pooled_result(const EccGroup* groups, int G, const EccPairRec* recs, int P, double* T, double* rho, int* nit,
                              int* status, int* converged, int* n_included, double* rho_pair, double* n_pair, int* included,
                              hipStream_t s)
{
    hipLaunchKernelGGL(ecc_pooled_result_kernel, dim3(blocks(P > G ? P : G)), dim3(THREADS), 0, s, groups, G, recs, P, T, rho, nit,
                       status, converged, n_included, rho_pair, n_pair, included);
}
