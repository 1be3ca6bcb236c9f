// Mutual-information alignment scoring and refinement (reference create_dataset/helper_functions/align.py:13-215).
// An EVALUATION is (pair p, bin count n, transform T): the optical frame of pair p is warped onto the thermal frame by
// cv2.warpPerspective(optical, inv(T), (W, H), borderValue=-1), the joint histogram of the warped against the thermal
// frame is taken as np.histogram2d(..., bins=(n, 2n)) takes it, optionally smoothed like scipy.ndimage.gaussian_filter,
// and turned into the negative (normalised) mutual information.  Evaluations are independent of each other: every kernel
// below has the evaluation on a grid axis, every sum has a fixed order and every atomic is an integer one, so the value of
// an evaluation has the same bits alone, inside any batch and from run to run.
//
//  * setup_kernel        M = cv_invert3(cv_invert3(T)) in double without contraction, min/max keys cleared
//  * zero_kernel         the evaluation's n x 2n counters
//  * warp_kernel         cv_warp_linear_kernel (homog_adapt.hip) with a source of another size and border value -1; stores the
//                        warped frame and folds its min / max into two ordered-integer keys (atomicMax on u32)
//  * minmax_kernel       the thermal frames' min / max, once per call
//  * thermal_map_kernel  the thermal bin (of 2n) of every pixel per distinct (pair, n), once per call, uint16
//  * hist_kernel         counts[xbin][ybin] += 1: n <= 64 in an LDS copy per workgroup (dynamic LDS, sized by the launch's
//                        largest such n; none when every evaluation has n > 64) whose non-zero counters are added to
//                        global memory at the end, larger n straight with global u32 atomics -- the same counts either way
//  * smooth_kernel       one axis of gaussian_filter(mode='constant') in double
//  * partial_kernel      per block of rows: sum x log x, the row sums, the block's column sums  (x = count + 2^-52)
//  * final_kernel        S, sum r log r, sum c log c -> the score (see below), negated, plus |T_init - T|_F
//  * nm_begin / nm_decide / nm_result   scipy's Nelder-Mead, one thread per problem, on the values the kernels above
//                        wrote for the problem's candidate points: over the n parameters of a motion model (9 matrix
//                        entries, 4 of a similarity, 6 of an affine transform), mapped to matrices by model_matrix
//  * model_transform_kernel             that map alone
//
// The score without a second pass over the histogram: with x the un-normalised entries and S their sum,
//     sum (x/S) log (x/S) = (sum x log x) / S - log S,
// and the same for the marginals, whose un-normalised sums r_i, c_j add up to S as well.
//
// Binning (numpy >= 2 on float32 samples: the edges are float32): a = min, b = max (a -= 0.5, b += 0.5 when equal),
// step = (b - a) / n, e[i] = fl(fl(i * step) + a), e[n] = b; bin = (number of edges <= v) - 1, v == e[n] in bin n - 1.
// The bin is guessed by a multiply and a truncation and then walked to where the edges put it.
#include "mp_common.h"
#include "mp_device.h"
#include "../../include/multipoint_hip.h"

namespace {

// ---- ordered keys: float -> u32 whose unsigned order is the float order (no NaN in a frame) ----
__device__ __forceinline__ unsigned f2key(float v)
{
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// keys[0] = ~key(min), keys[1] = key(max): both grow, both start at 0
__device__ __forceinline__ void fold_minmax(float lo, float hi, unsigned* keys)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o));
        hi = fmaxf(hi, __shfl_xor(hi, o));
    }
    if ((threadIdx.x & 63) == 0 && lo <= hi) {
        atomicMax(keys, ~f2key(lo));
        atomicMax(keys + 1, f2key(hi));
    }
}

struct Axis { float a, b, step, inv; };

// (every product and sum rounded separately, as numpy does: plain operators with contraction switched off -- hipcc's
// __fmul_rn / __fadd_rn wrappers are inline operators that carry their own `contract` flag)
__device__ __forceinline__ Axis make_axis(const unsigned* keys, int n)
{
#pragma clang fp contract(off)
    Axis x;
    x.a = key2f(~keys[0]);
    x.b = key2f(keys[1]);
    if (x.a == x.b) { x.a = x.a - 0.5f; x.b = x.b + 0.5f; }
    const float d = x.b - x.a;
    x.step = d / (float)n;
    x.inv = 1.f / x.step;
    return x;
}

__device__ __forceinline__ float edge(const Axis& x, int i)
{
#pragma clang fp contract(off)
    const float m = (float)i * x.step;
    return m + x.a;
}

// v in [a, b].  Only the inner edges 1 .. n-1 are looked at: e[0] = a <= v, and v == e[n] = b belongs to bin n - 1
__device__ __forceinline__ int bin_of(const Axis& x, int n, float v)
{
#pragma clang fp contract(off)
    const float g = (v - x.a) * x.inv;
    int k = g >= (float)(n - 1) ? n - 1 : (g > 0.f ? (int)g : 0);
    while (k > 0 && v < edge(x, k)) --k;
    while (k < n - 1 && v >= edge(x, k + 1)) ++k;
    return k;
}

__device__ __forceinline__ bool active(const int* nact, int G, int e) { return !nact || (e % G) < nact[e / G]; }

// cv::invert of a 3x3 double matrix: the closed-form adjugate path DECOMP_LU takes for n <= 3; singular -> zeros
__device__ __forceinline__ void cv_invert3(const double* S, double* t)
{
#pragma clang fp contract(off)
    double d = (S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6])) + S[2] * (S[3] * S[7] - S[4] * S[6]);
    if (d == 0.0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) t[i] = 0.0;
        return;
    }
    d = 1.0 / d;
    t[0] = (S[4] * S[8] - S[5] * S[7]) * d; t[1] = (S[2] * S[7] - S[1] * S[8]) * d; t[2] = (S[1] * S[5] - S[2] * S[4]) * d;
    t[3] = (S[5] * S[6] - S[3] * S[8]) * d; t[4] = (S[0] * S[8] - S[2] * S[6]) * d; t[5] = (S[2] * S[3] - S[0] * S[5]) * d;
    t[6] = (S[3] * S[7] - S[4] * S[6]) * d; t[7] = (S[1] * S[6] - S[0] * S[7]) * d; t[8] = (S[0] * S[4] - S[1] * S[3]) * d;
}

__global__ __launch_bounds__(64) void setup_kernel(const double* __restrict__ T, int E, const int* __restrict__ nact, int G,
                                                   double* __restrict__ M, unsigned* __restrict__ keys)
{
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E || !active(nact, G, e)) return;
    double t[9], a[9], m[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) t[i] = T[(size_t)e * 9 + i];
    cv_invert3(t, a);
    cv_invert3(a, m);
#pragma unroll
    for (int i = 0; i < 9; ++i) M[(size_t)e * 9 + i] = m[i];
    keys[2 * e] = 0u; keys[2 * e + 1] = 0u;
}

__global__ __launch_bounds__(256) void zero_kernel(const MiEval* __restrict__ ev, const int* __restrict__ nact, int G,
                                                   unsigned* __restrict__ counts)
{
    const int e = blockIdx.y;
    if (!active(nact, G, e)) return;
    const int n = ev[e].bins, total = 2 * n * n;
    unsigned* c = counts + ev[e].off;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) c[i] = 0u;
}

// src [B][Ho][Wo] -> dst [E][H][W]; bw0 is OpenCV's block width for the DESTINATION size
__global__ __launch_bounds__(256) void warp_kernel(const float* __restrict__ src, int Ho, int Wo, const MiEval* __restrict__ ev,
                                                   const int* __restrict__ nact, int G, const double* __restrict__ M, int H,
                                                   int W, int bw0, float* __restrict__ dst, unsigned* __restrict__ keys)
{
#pragma clang fp contract(off)
    const int e = blockIdx.z;
    if (!active(nact, G, e)) return;                    // (the whole workgroup)
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    float lo = INFINITY, hi = -INFINITY;
    if (x < W && y < H) {
        const float* img = src + (size_t)ev[e].pair * Ho * Wo;
        const CvWarpSource c = cv_warp_source(M + (size_t)e * 9, x, y, bw0);
        const int sx = c.sx, sy = c.sy;
        const bool xa = (unsigned)sx < (unsigned)Wo, xc = (unsigned)(sx + 1) < (unsigned)Wo;
        const bool ya = (unsigned)sy < (unsigned)Ho, yc = (unsigned)(sy + 1) < (unsigned)Ho;
        const float v0 = (ya && xa) ? img[(size_t)sy * Wo + sx] : -1.f;
        const float v1 = (ya && xc) ? img[(size_t)sy * Wo + sx + 1] : -1.f;
        const float v2 = (yc && xa) ? img[(size_t)(sy + 1) * Wo + sx] : -1.f;
        const float v3 = (yc && xc) ? img[(size_t)(sy + 1) * Wo + sx + 1] : -1.f;
        const float p0 = v0 * c.w0, p1 = v1 * c.w1, p2 = v2 * c.w2, p3 = v3 * c.w3;
        const float out = ((p0 + p1) + p2) + p3;
        dst[((size_t)e * H + y) * W + x] = out;
        lo = hi = out;
    }
    fold_minmax(lo, hi, keys + 2 * e);
}

// frames [B][HW] -> keys [B][2] (zeroed by the caller)
__global__ __launch_bounds__(256) void minmax_kernel(const float* __restrict__ img, int HW, unsigned* __restrict__ keys)
{
    const float* p = img + (size_t)blockIdx.y * HW;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
        const float v = p[i];
        lo = fminf(lo, v); hi = fmaxf(hi, v);
    }
    fold_minmax(lo, hi, keys + 2 * blockIdx.y);
}

// slot s = (pair, n): tmap [S][HW] = bin of 2n of the thermal pixel
__global__ __launch_bounds__(256) void thermal_map_kernel(const float* __restrict__ thermal, int HW, const int2* __restrict__ slots,
                                                          const unsigned* __restrict__ tkeys, unsigned short* __restrict__ tmap)
{
    const int2 sl = slots[blockIdx.y];
    const float* p = thermal + (size_t)sl.x * HW;
    const int n2 = 2 * sl.y;
    const Axis ax = make_axis(tkeys + 2 * sl.x, n2);
    unsigned short* o = tmap + (size_t)blockIdx.y * HW;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) o[i] = (unsigned short)bin_of(ax, n2, p[i]);
}

constexpr int HIST_PX = 2048;          // pixels of an evaluation per workgroup
constexpr int LDS_BINS = 64;           // an n x 2n u32 copy fits the workgroup's 32 KiB up to here

// strategy 0: by bin count, 1: LDS copy (n <= 64 only, checked by the caller), 2: global atomics
__global__ __launch_bounds__(256) void hist_kernel(const float* __restrict__ warped, const unsigned short* __restrict__ tmap,
                                                   const MiEval* __restrict__ ev, const int* __restrict__ nact, int G,
                                                   const unsigned* __restrict__ keys, int HW, unsigned* __restrict__ counts,
                                                   float* __restrict__ minmax, int strategy)
{
    extern __shared__ unsigned local[];      // n x 2n counters of the launch's largest LDS-counted evaluation, or nothing
    const int e = blockIdx.y;
    if (!active(nact, G, e)) return;
    const MiEval me = ev[e];
    const int n = me.bins, n2 = 2 * n;
    if (minmax && blockIdx.x == 0 && threadIdx.x == 0) {
        minmax[2 * e] = key2f(~keys[2 * e]);
        minmax[2 * e + 1] = key2f(keys[2 * e + 1]);
    }
    const Axis ax = make_axis(keys + 2 * e, n);
    const float* w = warped + (size_t)e * HW;
    const unsigned short* t = tmap + (size_t)me.tslot * HW;
    unsigned* c = counts + me.off;
    const int p0 = blockIdx.x * HIST_PX, p1 = min(HW, p0 + HIST_PX);
    const bool lds = strategy == 1 || (strategy == 0 && n <= LDS_BINS);       // (uniform over the workgroup)
    if (lds) {
        for (int i = threadIdx.x; i < n * n2; i += 256) local[i] = 0u;
        __syncthreads();
        for (int i = p0 + threadIdx.x; i < p1; i += 256) atomicAdd(&local[bin_of(ax, n, w[i]) * n2 + t[i]], 1u);
        __syncthreads();
        for (int i = threadIdx.x; i < n * n2; i += 256) {
            const unsigned v = local[i];
            if (v) atomicAdd(&c[i], v);
        }
    } else {
        for (int i = p0 + threadIdx.x; i < p1; i += 256) atomicAdd(&c[bin_of(ax, n, w[i]) * n2 + t[i]], 1u);
    }
}

// ---- smoothing: scipy.ndimage.gaussian_filter(jh, sigma, mode='constant'), one axis per launch, in double ----
// weights exp(-x^2 / 2 sigma^2) over x in [-r, r], r = int(4 sigma + 0.5), normalised by their sum (added in order)
template <typename SRC, int AXIS>
__global__ __launch_bounds__(256) void smooth_kernel(const SRC* __restrict__ in, long long in_stride, const MiEval* __restrict__ ev,
                                                     const int* __restrict__ nact, int G, double sigma, int r,
                                                     double* __restrict__ out, long long out_stride)
{
    __shared__ double wgt[2 * MI_MAX_RADIUS + 1];
    __shared__ double total;
    const int e = blockIdx.y;
    if (!active(nact, G, e)) return;
    if ((int)threadIdx.x <= 2 * r) {
        const double x = (double)((int)threadIdx.x - r);
        wgt[threadIdx.x] = exp(-0.5 / (sigma * sigma) * (x * x));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int k = 0; k <= 2 * r; ++k) sum += wgt[k];
        total = sum;
    }
    __syncthreads();
    if ((int)threadIdx.x <= 2 * r) wgt[threadIdx.x] /= total;
    __syncthreads();
    const int n = ev[e].bins, n2 = 2 * n;
    const SRC* src = in + (in_stride < 0 ? ev[e].off : (long long)e * in_stride);
    double* dst = out + (long long)e * out_stride;
    for (int f = blockIdx.x * 256 + threadIdx.x; f < n * n2; f += gridDim.x * 256) {
        const int i = f / n2, j = f - i * n2;
        double acc = 0.0;
        for (int k = 0; k <= 2 * r; ++k) {
            const int q = (AXIS == 0 ? i : j) + k - r;
            if (q < 0 || q >= (AXIS == 0 ? n : n2)) continue;
            acc += wgt[k] * (double)src[AXIS == 0 ? q * n2 + j : i * n2 + q];
        }
        dst[f] = acc;
    }
}

// ---- score ----
// fixed-order sum of one double per thread over the 256 threads of a workgroup (every thread gets it)
__device__ __forceinline__ double block_sum(double v, double* red)
{
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

constexpr double MI_EPS = 2.220446049250313e-16;      // np.finfo(float).eps

// part [E][MI_PARTS] | rowsum [E][256] | colpart [E][MI_PARTS][512]
template <typename SRC>
__global__ __launch_bounds__(256) void partial_kernel(const SRC* __restrict__ in, long long in_stride, const MiEval* __restrict__ ev,
                                                      const int* __restrict__ nact, int G, double* __restrict__ part,
                                                      double* __restrict__ rowsum, double* __restrict__ colpart)
{
    __shared__ double red[256];
    const int e = blockIdx.y, b = blockIdx.x;
    if (!active(nact, G, e)) return;
    const int n = ev[e].bins, n2 = 2 * n;
    const int rows = (n + MI_PARTS - 1) / MI_PARTS;
    const int i0 = b * rows, i1 = min(n, i0 + rows);
    if (i0 >= n) return;
    const SRC* src = in + (in_stride < 0 ? ev[e].off : (long long)e * in_stride);
    double xl = 0.0;
    for (int j = threadIdx.x; j < n2; j += 256) {
        double col = 0.0;
        for (int i = i0; i < i1; ++i) {
            const double x = (double)src[i * n2 + j] + MI_EPS;
            col += x;
            xl += x * log(x);
        }
        colpart[((size_t)e * MI_PARTS + b) * 512 + j] = col;
    }
    const double s = block_sum(xl, red);
    if (threadIdx.x == 0) part[(size_t)e * MI_PARTS + b] = s;
    const int lane = threadIdx.x & 63;
    for (int i = i0 + (threadIdx.x >> 6); i < i1; i += 4) {
        double r = 0.0;
        for (int j = lane; j < n2; j += 64) r += (double)src[i * n2 + j] + MI_EPS;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) r += __shfl_xor(r, o);
        if (lane == 0) rowsum[(size_t)e * 256 + i] = r;
    }
}

// values[e] = -(score) [+ |T_init[e / tg] - T[e]|_F]
__global__ __launch_bounds__(256) void final_kernel(const MiEval* __restrict__ ev, const int* __restrict__ nact, int G,
                                                    const double* __restrict__ part, const double* __restrict__ rowsum,
                                                    const double* __restrict__ colpart, int normalized,
                                                    const double* __restrict__ T, const double* __restrict__ Tinit, int tg,
                                                    double* __restrict__ values)
{
#pragma clang fp contract(off)
    __shared__ double red[256];
    const int e = blockIdx.x;
    if (!active(nact, G, e)) return;
    const int n = ev[e].bins, n2 = 2 * n;
    const int rows = (n + MI_PARTS - 1) / MI_PARTS, nb = (n + rows - 1) / rows;
    const int t = threadIdx.x;
    const double r = t < n ? rowsum[(size_t)e * 256 + t] : 0.0;
    const double S = block_sum(r, red);
    const double R = block_sum(t < n ? r * log(r) : 0.0, red);
    double cl = 0.0;
    for (int j = t; j < n2; j += 256) {
        double c = 0.0;
        for (int b = 0; b < nb; ++b) c += colpart[((size_t)e * MI_PARTS + b) * 512 + j];
        cl += c * log(c);
    }
    const double C = block_sum(cl, red);
    if (t != 0) return;
    double X = 0.0;
    for (int b = 0; b < nb; ++b) X += part[(size_t)e * MI_PARTS + b];
    const double lS = log(S);
    const double hj = X / S - lS, h1 = C / S - lS, h2 = R / S - lS;       // sum p log p of the joint and the two marginals
    double v = normalized ? -((h1 + h2) / hj - 1.0) : -((hj - h1) - h2);
    if (Tinit) {
        double q = 0.0;
        for (int i = 0; i < 9; ++i) {
            const double d = Tinit[(size_t)(e / tg) * 9 + i] - T[(size_t)e * 9 + i];
            q += d * d;
        }
        v += sqrt(q);
    }
    values[e] = v;
}

// ---- the motion model: n parameters -> the 3x3 matrix the objective reads (MP_MODEL_*; no clamping, as in the reference) ----
//   homography  the nine entries
//   similarity  (angle, scale, dx, dy) -> [[s cos a, s sin a, dx], [-s sin a, s cos a, dy], [0, 0, 1]]  (align.py:137-139)
//   affine      the six entries of the top two rows, last row (0, 0, 1)
__device__ __forceinline__ int model_params(int model)
{
    return model == MP_MODEL_SIMILARITY ? 4 : (model == MP_MODEL_AFFINE ? 6 : 9);
}

__device__ __forceinline__ void model_matrix(int model, const double* __restrict__ p, double* __restrict__ t)
{
#pragma clang fp contract(off)
    if (model == MP_MODEL_SIMILARITY) {
        const double c = p[1] * cos(p[0]), s = p[1] * sin(p[0]);
        t[0] = c; t[1] = s; t[2] = p[2];
        t[3] = -s; t[4] = c; t[5] = p[3];
        t[6] = 0.0; t[7] = 0.0; t[8] = 1.0;
    } else if (model == MP_MODEL_AFFINE) {
        for (int k = 0; k < 6; ++k) t[k] = p[k];
        t[6] = 0.0; t[7] = 0.0; t[8] = 1.0;
    } else {
        for (int k = 0; k < 9; ++k) t[k] = p[k];
    }
}

__global__ __launch_bounds__(64) void model_transform_kernel(int model, const double* __restrict__ params, int rows,
                                                             double* __restrict__ T)
{
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= rows) return;
    model_matrix(model, params + (size_t)r * model_params(model), T + (size_t)r * 9);
}

// ---- Nelder-Mead (scipy.optimize._optimize._minimize_neldermead, adaptive=False, no bounds), one thread per problem ----
// over the ND parameters of the motion model with a simplex of NV = ND + 1 vertices.  A problem's candidate points are rows
// of MI_PARAMS_MAX doubles in candp; nm_emit turns the first `count` of them into the matrices of its evaluation slots.
enum { NM_INIT = 0, NM_STEP = 1, NM_SHRINK = 2 };
constexpr int CS = MI_PARAMS_MAX;      // stride of a candidate point

// stable insertion sort of the simplex by value (scipy: np.argsort + np.take; ties keep their order here)
__device__ void nm_sort(MiNmState& st, int ND)
{
    const int NV = ND + 1;
    for (int i = 1; i < NV; ++i) {
        for (int j = i; j > 0 && st.fsim[j] < st.fsim[j - 1]; --j) {
            const double f = st.fsim[j]; st.fsim[j] = st.fsim[j - 1]; st.fsim[j - 1] = f;
            for (int k = 0; k < ND; ++k) {
                const double x = st.sim[j][k]; st.sim[j][k] = st.sim[j - 1][k]; st.sim[j - 1][k] = x;
            }
        }
    }
}

__device__ __forceinline__ void nm_take(MiNmState& st, int ND, const double* x, double f)
{
    for (int k = 0; k < ND; ++k) st.sim[ND][k] = x[k];
    st.fsim[ND] = f;
}

__device__ __forceinline__ void nm_emit(int model, const double* c, int count, double* T)
{
    for (int v = 0; v < count; ++v) model_matrix(model, c + v * CS, T + v * 9);
}

// one thread per problem: the initial simplex into the problem's candidate slots, the start's matrix into tinit
__global__ __launch_bounds__(64) void nm_begin_kernel(MiNmState* __restrict__ state, const MiNmOptions* __restrict__ opt,
                                                      int model, const double* __restrict__ start, int P,
                                                      double* __restrict__ candp, double* __restrict__ cand,
                                                      double* __restrict__ tinit, int* __restrict__ nact)
{
#pragma clang fp contract(off)
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= P) return;
    const int ND = model_params(model), NV = ND + 1;
    MiNmState& st = state[q];
    const double* x0 = start + (size_t)q * ND;
    double* c = candp + (size_t)q * MI_SLOTS * CS;
    for (int v = 0; v < NV; ++v)
        for (int k = 0; k < ND; ++k) {
            double y = x0[k];
            if (v == k + 1) y = y != 0.0 ? (1.0 + 0.05) * y : 0.00025;
            c[v * CS + k] = y;
            st.sim[v][k] = y;
        }
    nm_emit(model, c, NV, cand + (size_t)q * MI_SLOTS * 9);
    model_matrix(model, c, tinit + (size_t)q * 9);
    st.opt = opt[q];
    st.iterations = 0; st.fcalls = 0; st.phase = NM_INIT; st.done = 0; st.status = 0;
    nact[q] = NV;
}

// consumes the values of the problem's candidate slots, applies scipy's rules and writes the next candidates
__global__ __launch_bounds__(64) void nm_decide_kernel(MiNmState* __restrict__ state, int model, int P,
                                                       double* __restrict__ candp, double* __restrict__ cand,
                                                       const double* __restrict__ fc, int* __restrict__ nact,
                                                       int* __restrict__ live)
{
#pragma clang fp contract(off)
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= P) return;
    MiNmState& st = state[q];
    if (st.done) return;
    const int ND = model_params(model), NV = ND + 1;
    double* c = candp + (size_t)q * MI_SLOTS * CS;
    double* T = cand + (size_t)q * MI_SLOTS * 9;
    const double* f = fc + (size_t)q * MI_SLOTS;
    const int maxfun = st.opt.maxfun;
    // func(): scipy's wrapper refuses the call (and the iteration ends uncounted) once maxfun calls were made
    auto call = [&]() { if (st.fcalls >= maxfun) return false; ++st.fcalls; return true; };
    bool shrink = false;
    if (st.phase == NM_INIT) {
        for (int v = 0; v < NV; ++v) st.fsim[v] = call() ? f[v] : INFINITY;
        st.iterations = 1;
    } else if (st.phase == NM_STEP) {
        // candidates: 0 reflection, 1 expansion, 2 outside contraction, 3 inside contraction
        bool ok = call();
        const double fxr = f[0];
        if (ok) {
            if (fxr < st.fsim[0]) {
                ok = call();
                if (ok) { if (f[1] < fxr) nm_take(st, ND, c + CS, f[1]); else nm_take(st, ND, c, fxr); }
            } else if (fxr < st.fsim[NV - 2]) {
                nm_take(st, ND, c, fxr);
            } else if (fxr < st.fsim[NV - 1]) {
                ok = call();
                if (ok) { if (f[2] <= fxr) nm_take(st, ND, c + 2 * CS, f[2]); else shrink = true; }
            } else {
                ok = call();
                if (ok) { if (f[3] < st.fsim[NV - 1]) nm_take(st, ND, c + 3 * CS, f[3]); else shrink = true; }
            }
        }
        if (ok && !shrink) ++st.iterations;
    } else {
        // the shrunk vertices 1 .. ND in the candidate slots 0 .. ND - 1: vertex j moves before its value is asked for
        bool ok = true;
        for (int j = 1; j < NV && ok; ++j) {
            for (int k = 0; k < ND; ++k) st.sim[j][k] = c[(j - 1) * CS + k];
            ok = call();
            if (ok) st.fsim[j] = f[j - 1];
        }
        if (ok) ++st.iterations;
    }
    if (shrink) {
        for (int j = 1; j < NV; ++j)
            for (int k = 0; k < ND; ++k) c[(j - 1) * CS + k] = st.sim[0][k] + 0.5 * (st.sim[j][k] - st.sim[0][k]);
        nm_emit(model, c, NV - 1, T);
        st.phase = NM_SHRINK;
        nact[q] = NV - 1;
        atomicAdd(live, 1);
        return;
    }
    nm_sort(st, ND);
    bool go = st.fcalls < maxfun && st.iterations < st.opt.maxiter;
    if (go) {
        double dx = 0.0, df = 0.0;
        for (int j = 1; j < NV; ++j) {
            for (int k = 0; k < ND; ++k) dx = fmax(dx, fabs(st.sim[j][k] - st.sim[0][k]));
            df = fmax(df, fabs(st.fsim[0] - st.fsim[j]));
        }
        if (dx <= st.opt.xatol && df <= st.opt.fatol) go = false;
    }
    if (!go) {
        st.done = 1;
        st.status = st.fcalls >= maxfun ? 1 : (st.iterations >= st.opt.maxiter ? 2 : 0);
        nact[q] = 0;
        return;
    }
    for (int k = 0; k < ND; ++k) {
        double xbar = st.sim[0][k];
        for (int j = 1; j < NV - 1; ++j) xbar = xbar + st.sim[j][k];
        xbar = xbar / (double)ND;
        const double last = st.sim[NV - 1][k];
        c[k] = 2.0 * xbar - 1.0 * last;
        c[CS + k] = 3.0 * xbar - 2.0 * last;
        c[2 * CS + k] = 1.5 * xbar - 0.5 * last;
        c[3 * CS + k] = 0.5 * xbar + 0.5 * last;
    }
    nm_emit(model, c, 4, T);
    st.phase = NM_STEP;
    nact[q] = 4;
    atomicAdd(live, 1);
}

__global__ __launch_bounds__(64) void nm_result_kernel(const MiNmState* __restrict__ state, int model, int P,
                                                       double* __restrict__ T, double* __restrict__ params,
                                                       double* __restrict__ value, int* __restrict__ iterations,
                                                       int* __restrict__ fcalls, int* __restrict__ success)
{
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= P) return;
    const MiNmState& st = state[q];
    const int ND = model_params(model);
    // (a problem still running reports the best vertex of its latest sort and success 0)
    model_matrix(model, st.sim[0], T + (size_t)q * 9);
    if (params)
        for (int k = 0; k < ND; ++k) params[(size_t)q * ND + k] = st.sim[0][k];
    value[q] = st.fsim[0];
    iterations[q] = st.iterations;
    fcalls[q] = st.fcalls;
    success[q] = st.done && st.status == 0;
}

}  // namespace

void launch_mi_thermal(const float* thermal, int B, int HW, const int2* slots, int S, unsigned* tkeys, unsigned short* tmap,
                       hipStream_t s)
{
    (void)hipMemsetAsync(tkeys, 0, (size_t)B * 8, s);
    const int chunks = min(64, (HW + 2047) / 2048);
    minmax_kernel<<<dim3(chunks, B), 256, 0, s>>>(thermal, HW, tkeys);
    thermal_map_kernel<<<dim3(chunks, S), 256, 0, s>>>(thermal, HW, slots, tkeys, tmap);
}

void launch_mi_histograms(const MiLaunch& L, unsigned* counts, float* warped, float* minmax, int strategy, hipStream_t s)
{
    const int bh0 = L.H < 16 ? L.H : 16;
    const int bw0 = (1024 / bh0) < L.W ? (1024 / bh0) : L.W;
    const int HW = L.H * L.W;
    setup_kernel<<<(L.E + 63) / 64, 64, 0, s>>>(L.T, L.E, L.nact, L.G, L.M, L.keys);
    zero_kernel<<<dim3(8, L.E), 256, 0, s>>>(L.ev, L.nact, L.G, counts);
    warp_kernel<<<dim3((L.W + 63) / 64, (L.H + 3) / 4, L.E), 256, 0, s>>>(L.optical, L.Ho, L.Wo, L.ev, L.nact, L.G, L.M, L.H, L.W,
                                                                         bw0, warped, L.keys);
    // only a launch with an evaluation that counts in LDS reserves any
    const int nl = strategy == 2 ? 0 : L.lds_bins;
    hist_kernel<<<dim3((HW + HIST_PX - 1) / HIST_PX, L.E), 256, (size_t)(2 * nl * nl) * 4, s>>>(warped, L.tmap, L.ev, L.nact, L.G, L.keys, HW, counts,
                                                                        minmax, strategy);
}

// counts at ev[e].off; smooth_a / smooth_b: [E][2 max_bins^2] doubles (sigma > 0 only)
void launch_mi_score(const MiLaunch& L, const unsigned* counts, double sigma, int normalized, const double* Tinit, int tg,
                     long long smooth_stride, double* smooth_a, double* smooth_b, double* values, hipStream_t s)
{
    if (sigma > 0.0) {
        const int r = (int)(4.0 * sigma + 0.5);
        smooth_kernel<unsigned, 0><<<dim3(16, L.E), 256, 0, s>>>(counts, -1, L.ev, L.nact, L.G, sigma, r, smooth_a, smooth_stride);
        smooth_kernel<double, 1><<<dim3(16, L.E), 256, 0, s>>>(smooth_a, smooth_stride, L.ev, L.nact, L.G, sigma, r, smooth_b,
                                                              smooth_stride);
        partial_kernel<double><<<dim3(MI_PARTS, L.E), 256, 0, s>>>(smooth_b, smooth_stride, L.ev, L.nact, L.G, L.part, L.rowsum,
                                                                  L.colpart);
    } else {
        partial_kernel<unsigned><<<dim3(MI_PARTS, L.E), 256, 0, s>>>(counts, -1, L.ev, L.nact, L.G, L.part, L.rowsum, L.colpart);
    }
    final_kernel<<<L.E, 256, 0, s>>>(L.ev, L.nact, L.G, L.part, L.rowsum, L.colpart, normalized, L.T, Tinit, tg, values);
}

int mi_model_params(int model)
{
    return model == MP_MODEL_HOMOGRAPHY ? 9 : (model == MP_MODEL_SIMILARITY ? 4 : (model == MP_MODEL_AFFINE ? 6 : 0));
}

void launch_mi_model_transform(int model, const double* params, int rows, double* transforms, hipStream_t s)
{
    model_transform_kernel<<<(rows + 63) / 64, 64, 0, s>>>(model, params, rows, transforms);
}

void launch_mi_nm_begin(MiNmState* state, const MiNmOptions* opt, int model, const double* x0, int P, double* candp, double* cand,
                        double* tinit, int* nact, hipStream_t s)
{
    nm_begin_kernel<<<(P + 63) / 64, 64, 0, s>>>(state, opt, model, x0, P, candp, cand, tinit, nact);
}

void launch_mi_nm_decide(MiNmState* state, int model, int P, double* candp, double* cand, const double* values, int* nact,
                         int* live, hipStream_t s)
{
    (void)hipMemsetAsync(live, 0, 4, s);
    nm_decide_kernel<<<(P + 63) / 64, 64, 0, s>>>(state, model, P, candp, cand, values, nact, live);
}

void launch_mi_nm_result(const MiNmState* state, int model, int P, double* T, double* params, double* value, int* iterations,
                         int* fcalls, int* success, hipStream_t s)
{
    nm_result_kernel<<<(P + 63) / 64, 64, 0, s>>>(state, model, P, T, params, value, iterations, fcalls, success);
}
