// Local residual field: for every window of an aligned pair, the integer displacement of the optical feature frame
// that maximises the zero-mean normalised cross-correlation with the thermal one, its parabola refinement and its confidence terms.
//
//   residual_kernel   one workgroup (four waves) per (frame, window).  The w x w template of F_t, the (w + 2r)^2 search region of
//                     F_o and the mask bytes of that region are staged once in LDS (no mask: ones, so both forms run the same
//                     code).  The (2r + 1)^2 displacements are dealt to the waves (wave v takes v, v + 4, ...), the template
//                     pixels of a displacement to the lanes (lane l takes l, l + 64, ... in that order; the row and column of a
//                     pixel are stepped, not divided, so any w x w -- 64 pixels at w = 8, 576 at w = 24 -- runs the same loop).
//                     The three per-pixel products are fp32, the five sums and the count are float64 / int accumulators in
//                     registers, reduced by butterflies; lane 0 forms the score into LDS.  A search region in which the mask
//                     excludes nothing takes the template's two sums and the count once, in the same order of additions, instead
//                     of once per displacement: the same bits for three fifths of the work.  Wave 0 then picks the best score (ties:
//                     the lowest row-major index), the second peak outside its 3 x 3 block and the parabola offsets, and lane 0
//                     writes the window's record with ordinary per-lane stores.
//   No atomics, and nothing of a window's arithmetic depends on the grid or the batch: a window has the same bits alone, in any
//   batch and from run to run.
#include "../../include/multipoint_hip.h"
#include "mp_common.h"
#include "mp_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256, WAVES = THREADS / MP_WAVE;

// is candidate (sb, ib) a better peak than (sa, ia)?  NaN is "undefined"; equal scores go to the lower index
__device__ __forceinline__ bool better(double sa, int ia, double sb, int ib)
{
    if (!(sb == sb)) return false;
    if (!(sa == sa)) return true;
    return sb > sa || (sb == sa && ib < ia);
}

__device__ __forceinline__ void wave_best(double& s, int& i)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double so = __shfl_xor(s, off, 64);
        const int io = __shfl_xor(i, off, 64);
        if (better(s, i, so, io)) s = so, i = io;
    }
}

// offset of the vertex of the parabola through (-1, a), (0, b), (1, c) with b the largest: in [-0.5, 0.5]
__device__ __forceinline__ double parabola(double a, double b, double c)
{
    const double den = (a - 2.0 * b) + c;
    if (!(den < 0.0)) return 0.0;
    const double o = 0.5 * (a - c) / den;
    return o < -0.5 ? -0.5 : o > 0.5 ? 0.5 : o;
}

__global__ __launch_bounds__(THREADS) void residual_kernel(ResidualParams p)
{
    extern __shared__ __align__(16) unsigned char lds[];
    const int w = p.w, r = p.r, R = w + 2 * r, side = 2 * r + 1, ND = side * side, npx = w * w;
    double* score = reinterpret_cast<double*>(lds);                  // [ND], NaN: undefined
    int* cnt = reinterpret_cast<int*>(score + ND);                   // [ND] (+ 1 pad: the floats stay 8-byte aligned)
    float* tpl = reinterpret_cast<float*>(cnt + ND + (ND & 1));      // [w][w]
    float* srch = tpl + npx;                                         // [R][R]
    unsigned char* msk = reinterpret_cast<unsigned char*>(srch + R * R);   // [R][R]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, win = blockIdx.x;
    const int iy = win / p.gx, ix = win - iy * p.gx;
    const int y0 = p.r + iy * p.s, x0 = p.r + ix * p.s;              // y0 - r >= 0 and y0 + w + r <= H by the grid rule
    const size_t frame = (size_t)b * p.H * p.W;
    const float* ft = p.ft + frame + (size_t)y0 * p.W + x0;
    const float* fo = p.fo + frame + (size_t)(y0 - r) * p.W + (x0 - r);
    const unsigned char* mk = p.mask ? p.mask + (p.mask_frames > 1 ? frame : 0) + (size_t)(y0 - r) * p.W + (x0 - r) : nullptr;
    for (int i = tid; i < npx; i += THREADS) {
        const int py = i / w, px = i - py * w;
        tpl[i] = ft[(size_t)py * p.W + px];
    }
    int excluded = 0;
    for (int i = tid; i < R * R; i += THREADS) {
        const int py = i / R, px = i - py * R;
        srch[i] = fo[(size_t)py * p.W + px];
        const unsigned char use = mk ? (mk[(size_t)py * p.W + px] != 0) : 1;
        msk[i] = use;
        excluded |= !use;
    }
    // Does the mask exclude anything of this search region?  If not, S_d is the whole window for every d: the template's two sums
    // and the count are taken once, in the order the masked loop would take them (so the bits are those of a mask of ones).
    const bool masked = __syncthreads_or(excluded) != 0;

    // lane l's pixels are l, l + 64, ...: a step of 64 pixels is qa rows and ra columns, with at most one wrap
    const int qa = MP_WAVE / w, ra = MP_WAVE - qa * w;
    const int ly = lane / w, lx = lane - ly * w;
    const double need = p.min_valid * (double)npx;
    double st_all = 0.0, stt_all = 0.0;
    if (!masked) {
        for (int i = lane; i < npx; i += MP_WAVE) {
            const float t = tpl[i];
            const float tt = t * t;
            st_all += (double)t, stt_all += (double)tt;
        }
        st_all = wave_add(st_all), stt_all = wave_add(stt_all);
    }
    for (int d = wave; d < ND; d += WAVES) {                         // (d is the same in every lane of the wave)
        const int dy = d / side, dx = d - dy * side;                 // displacement + r
        const int base = dy * R + dx;
        double st = 0.0, so = 0.0, stt = 0.0, soo = 0.0, sto = 0.0;
        int n = 0;
        int px = lx, at = ly * R + lx + base;
        if (masked) {
            for (int i = lane; i < npx; i += MP_WAVE) {
                if (msk[at]) {
                    const float t = tpl[i], o = srch[at];
                    const float tt = t * t, oo = o * o, to = t * o;
                    st += (double)t, so += (double)o, stt += (double)tt, soo += (double)oo, sto += (double)to;
                    ++n;
                }
                px += ra, at += qa * R + ra;
                if (px >= w) px -= w, at += R - w;
            }
            st = wave_add(st), stt = wave_add(stt);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
        } else {
            for (int i = lane; i < npx; i += MP_WAVE) {
                const float t = tpl[i], o = srch[at];
                const float oo = o * o, to = t * o;
                so += (double)o, soo += (double)oo, sto += (double)to;
                px += ra, at += qa * R + ra;
                if (px >= w) px -= w, at += R - w;
            }
            st = st_all, stt = stt_all, n = npx;
        }
        so = wave_add(so), soo = wave_add(soo), sto = wave_add(sto);
        if (lane == 0) {
            double sc = __builtin_nan("");
            const double nd = (double)n;
            if (n > 0 && !(nd < need)) {
                const double mt = st / nd, mo = so / nd;
                const double ctt = stt - mt * st, coo = soo - mo * so, cto = sto - mt * so;
                const double floor_n = p.var_floor * nd;
                if (ctt > floor_n && coo > floor_n) sc = cto / (sqrt(ctt) * sqrt(coo));
            }
            score[d] = sc;
            cnt[d] = n;
        }
    }
    __syncthreads();
    if (wave != 0) return;

    double bs = __builtin_nan("");
    int bi = ND;
    for (int d = lane; d < ND; d += MP_WAVE)
        if (better(bs, bi, score[d], d)) bs = score[d], bi = d;
    wave_best(bs, bi);
    const int d0 = r * side + r;
    const bool few = (double)cnt[d0] < need;
    const bool found = bs == bs && !few;
    double s2 = __builtin_nan("");
    int i2 = ND;
    const int by = found ? bi / side : 0, bx = found ? bi - by * side : 0;
    if (found) {
        for (int d = lane; d < ND; d += MP_WAVE) {
            const int dy = d / side, dx = d - dy * side;
            if (abs(dy - by) <= 1 && abs(dx - bx) <= 1) continue;
            if (better(s2, i2, score[d], d)) s2 = score[d], i2 = d;
        }
        wave_best(s2, i2);
    }
    if (lane != 0) return;

    const double nan = __builtin_nan("");
    double o_dy = nan, o_dx = nan, o_rho = nan, o_rho0 = nan, o_second = nan;
    int o_n = cnt[d0], status = few ? MP_RES_FEW_VALID : MP_RES_FLAT;
    if (found) {
        double fy = 0.0, fx = 0.0;
        const bool edge_y = by == 0 || by == side - 1, edge_x = bx == 0 || bx == side - 1;
        if (!edge_y) {
            const double a = score[bi - side], c = score[bi + side];
            if (a == a && c == c) fy = parabola(a, bs, c);
        }
        if (!edge_x) {
            const double a = score[bi - 1], c = score[bi + 1];
            if (a == a && c == c) fx = parabola(a, bs, c);
        }
        o_dy = (double)(by - r) + fy, o_dx = (double)(bx - r) + fx;
        o_rho = bs, o_rho0 = score[d0];
        o_second = s2 == s2 ? s2 : -__builtin_inf();
        o_n = cnt[bi];
        status = (edge_y || edge_x) ? MP_RES_AT_EDGE : MP_RES_OK;
    }
    const size_t rec = (size_t)b * gridDim.x + win;
    double* od = p.out_d + rec * 5;
    od[0] = o_dy, od[1] = o_dx, od[2] = o_rho, od[3] = o_rho0, od[4] = o_second;
    p.out_i[rec * 2] = o_n, p.out_i[rec * 2 + 1] = status;
}

}  // namespace

size_t residual_lds_bytes(int w, int r)
{
    const size_t R = (size_t)w + 2 * r, side = 2 * (size_t)r + 1, ND = side * side;
    const size_t bytes = ND * sizeof(double) + (ND + (ND & 1)) * sizeof(int) + ((size_t)w * w + R * R) * sizeof(float) + R * R;
    return (bytes + 15) & ~(size_t)15;
}

void launch_residual_field(const ResidualParams& p, int B, hipStream_t s)
{
    const dim3 grid((unsigned)(p.gy * p.gx), (unsigned)B);
    hipLaunchKernelGGL(residual_kernel, grid, dim3(THREADS), residual_lds_bytes(p.w, p.r), s, p);
}
