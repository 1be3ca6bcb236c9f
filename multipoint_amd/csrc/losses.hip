// Forward-only evaluation of SuperPointLoss (reference multipoint/utils/losses.py:8-272): the detector loss
// (:85-122) and the dense descriptor loss (:207-272) with the working set O(B * Hc*Wc) instead of the reference's
// B x (Hc*Wc)^2 tensors (distances, correspondences, dot products, positive / negative terms, mask).
//
// detector_loss_kernel    one thread per cell: the 64 label bits of the cell (space_to_depth, channel 8*dy + dx,
//                         utils.py:71-76), cell validity (all 64 pixels valid: torch.prod, :96-98), then
//                           cross entropy: label = argmax([3*kp + noise, 2.0]) (first maximum), loss = logsumexp - logit
//                           BCE: multi-hot + dustbin 1 - min(sum, 1), normalised, on softmax (log clamped at -100)
//                         one fp32 partial sum of loss * valid and one count of valid cells per workgroup.
// desc_prologue_kernel    one thread per cell: the cell centre (8h+4, 8w+4) warped by inverse(homography) in the
//                         operation order of warp_points_pytorch (homographies.py:348-356), kept in fp32, and the
//                         cell's validity on each side; integer counts of valid cells per workgroup.
// desc_loss_tile_kernel   a 128 x 128 tile of desc2 . desc1^T on v_mfma_f32_32x32x2_f32 (operands staged through
//                         LDS in k-chunks of 32), the hinge / correspondence / mask epilogue in registers and one
//                         fp32 partial (positive, negative, corresponding pairs) per tile.  Nothing of size N^2 is
//                         written.  corr = sqrt_rn(dy^2 + dx^2) <= threshold is evaluated as s <= s_max, s_max the
//                         largest float whose correctly rounded square root is <= threshold (the host finds it; sqrt_rn
//                         is monotone, so the two tests agree for every s).
// *_reduce_kernel         one workgroup per image sums the partials in fp64 in a fixed order: the result is
//                         bit-identical from run to run (no float atomics anywhere).
#include "mp_common.h"
#include "mp_device.h"
#include "mp_workspace.h"

namespace {

constexpr int LT = 128;         // descriptor tile edge (cells of each side)
constexpr int KC = 32;          // k-chunk of the product staged in LDS
constexpr int KRS = KC + 4;     // LDS row stride in floats (the padding spreads the 16-byte reads over the banks)
constexpr int RED = 256;        // threads of every launch here

// label_noise 'device': a uniform draw in [0, 1) with 24 random bits (as torch.rand's fp32) per (seed, b, c, h, w)
__device__ __forceinline__ float hash_noise(unsigned long long seed, int b, int c, int hc, int wc, int Hc, int Wc)
{
    const unsigned long long idx = (((unsigned long long)b * 64 + c) * Hc + hc) * Wc + wc;
    return (float)(mix64(seed ^ mix64(idx)) >> 40) * 0x1p-24f;
}

// fixed-order sum of NV values over the 256 threads of a workgroup; thread 0 gets the totals
template <typename T, int NV>
__device__ __forceinline__ void block_sum(T (&v)[NV], T (*red)[RED])
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < NV; ++k) red[k][tid] = v[k];
    __syncthreads();
    for (int s = RED / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < NV; ++k) red[k][tid] = red[k][tid] + red[k][tid + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = red[k][0];
}

__global__ __launch_bounds__(RED) void detector_loss_kernel(const float* __restrict__ logits,
                                                           const unsigned char* __restrict__ kp,
                                                           const unsigned char* __restrict__ valid,
                                                           const float* __restrict__ noise, unsigned long long seed,
                                                           int H, int W, int use_ce, float* __restrict__ part_sum,
                                                           int* __restrict__ part_cnt)
{
    __shared__ float red_f[1][RED];
    __shared__ int red_i[1][RED];
    const int Hc = H >> 3, Wc = W >> 3, N = Hc * Wc;
    const int b = blockIdx.y;
    const int n = blockIdx.x * RED + threadIdx.x;
    float loss[1] = {0.f};
    int cnt[1] = {0};
    if (n < N) {
        const int hc = n / Wc, wc = n - hc * Wc;
        const long long pix0 = ((long long)b * H + hc * 8) * W + wc * 8;
        bool vcell = true;
        unsigned long long bits = 0;
#pragma unroll
        for (int dy = 0; dy < 8; ++dy) {
            const unsigned long long kr = *reinterpret_cast<const unsigned long long*>(kp + pix0 + (long long)dy * W);
            const unsigned long long vr = valid ? *reinterpret_cast<const unsigned long long*>(valid + pix0 + (long long)dy * W)
                                                : ~0ull;
#pragma unroll
            for (int dx = 0; dx < 8; ++dx) {
                bits |= (unsigned long long)(((kr >> (8 * dx)) & 0xff) != 0) << (8 * dy + dx);
                vcell = vcell && (((vr >> (8 * dx)) & 0xff) != 0);
            }
        }
        const float* lg = logits + (long long)b * 65 * N + n;
        float m = -__builtin_inff();
        for (int c = 0; c < 65; ++c) m = fmaxf(m, lg[(long long)c * N]);
        float se = 0.f;
        for (int c = 0; c < 65; ++c) se += expf(lg[(long long)c * N] - m);
        float l;
        if (use_ce) {
            // argmax over [3 * kp_c + noise_c (c < 64), 2.0]: channels without a keypoint stay below 1 < 2, so the label is the
            // FIRST keypoint channel with the largest fp32 value 3 + noise (ties after the rounding of 3 + u keep the lower
            // channel, as torch.argmax), or the dustbin 64 when the cell holds no keypoint
            int label = 64;
            float best = 2.f;
            for (unsigned long long rest = bits; rest; rest &= rest - 1) {
                const int c = __builtin_ctzll(rest);
                const float u = noise ? noise[(((long long)b * 64 + c) * Hc + hc) * Wc + wc]
                                      : hash_noise(seed, b, c, hc, wc, Hc, Wc);
                const float v = __fadd_rn(3.f, u);
                if (v > best) { best = v; label = c; }
            }
            l = logf(se) - (lg[(long long)label * N] - m);         // -log_softmax[label]
        } else {
            const int k = __builtin_popcountll(bits);
            const float dust = k ? 0.f : 1.f;
            const float S = (float)k + dust;
            l = 0.f;
            for (int c = 0; c < 65; ++c) {
                const float y = (c < 64 ? (float)((bits >> c) & 1) : dust) / S;
                const float p = expf(lg[(long long)c * N] - m) / se;
                // torch binary_cross_entropy: (y - 1) * max(log1p(-p), -100) - y * max(log(p), -100)
                l += (y - 1.f) * fmaxf(log1pf(-p), -100.f) - y * fmaxf(logf(p), -100.f);
            }
        }
        loss[0] = vcell ? l : 0.f * l;
        cnt[0] = vcell ? 1 : 0;
    }
    block_sum<float, 1>(loss, red_f);
    block_sum<int, 1>(cnt, red_i);
    if (threadIdx.x == 0) {
        part_sum[(long long)b * gridDim.x + blockIdx.x] = loss[0];
        part_cnt[(long long)b * gridDim.x + blockIdx.x] = cnt[0];
    }
}

__global__ __launch_bounds__(RED) void detector_reduce_kernel(const float* __restrict__ part_sum,
                                                             const int* __restrict__ part_cnt, int nblk,
                                                             double* __restrict__ out)
{
    __shared__ double red_d[1][RED];
    __shared__ long long red_l[1][RED];
    const int b = blockIdx.x;
    double s[1] = {0.0};
    long long c[1] = {0};
    for (int t = threadIdx.x; t < nblk; t += RED) {
        s[0] += (double)part_sum[(long long)b * nblk + t];
        c[0] += part_cnt[(long long)b * nblk + t];
    }
    block_sum<double, 1>(s, red_d);
    block_sum<long long, 1>(c, red_l);
    if (threadIdx.x == 0) { out[2 * b] = s[0]; out[2 * b + 1] = (double)c[0]; }
}

// fp32 inverse of a 3x3 (adjugate / determinant in fp64, rounded once per entry)
__device__ __forceinline__ void inverse3(const float* __restrict__ m, float* inv)
{
    const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
    const double A = e * i - f * h, B = -(d * i - f * g), C = d * h - e * g;
    const double det = a * A + b * B + c * C;
    const double r = 1.0 / det;
    inv[0] = (float)(A * r); inv[1] = (float)(-(b * i - c * h) * r); inv[2] = (float)((b * f - c * e) * r);
    inv[3] = (float)(B * r); inv[4] = (float)((a * i - c * g) * r);  inv[5] = (float)(-(a * f - c * d) * r);
    inv[6] = (float)(C * r); inv[7] = (float)(-(a * h - b * g) * r); inv[8] = (float)((a * e - b * d) * r);
}

__global__ __launch_bounds__(RED) void desc_prologue_kernel(const float* __restrict__ hom1, const float* __restrict__ hom2,
                                                           const unsigned char* __restrict__ valid1,
                                                           const unsigned char* __restrict__ valid2, int B, int H, int W,
                                                           float4* __restrict__ cells, float* __restrict__ warped,
                                                           int* __restrict__ cnt_part)
{
    __shared__ int red_i[2][RED];
    const int Hc = H >> 3, Wc = W >> 3, N = Hc * Wc;
    const int b = blockIdx.y;
    const int n = blockIdx.x * RED + threadIdx.x;
    int cnt[2] = {0, 0};
    if (n < N) {
        const int hc = n / Wc, wc = n - hc * Wc;
        const float y = hc * 8.f + 4.f, x = wc * 8.f + 4.f;
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const float* hom = side ? hom2 : hom1;
            const unsigned char* valid = side ? valid2 : valid1;
            float wy = y, wx = x;
            if (hom) {
                float hi[9];
                inverse3(hom + (long long)b * 9, hi);
                // bmm(H^-1, (x, y, 1)^T): row . (x, y, 1) summed left to right, every product and sum rounded
                const float px = __fadd_rn(__fadd_rn(__fmul_rn(hi[0], x), __fmul_rn(hi[1], y)), hi[2]);
                const float py = __fadd_rn(__fadd_rn(__fmul_rn(hi[3], x), __fmul_rn(hi[4], y)), hi[5]);
                const float pz = __fadd_rn(__fadd_rn(__fmul_rn(hi[6], x), __fmul_rn(hi[7], y)), hi[8]);
                wx = __fdiv_rn(px, pz);
                wy = __fdiv_rn(py, pz);
            }
            bool v = true;
            if (valid) {
                const long long pix0 = ((long long)b * H + hc * 8) * W + wc * 8;
#pragma unroll
                for (int dy = 0; dy < 8; ++dy) {
                    const unsigned long long r = *reinterpret_cast<const unsigned long long*>(valid + pix0 + (long long)dy * W);
#pragma unroll
                    for (int dx = 0; dx < 8; ++dx) v = v && (((r >> (8 * dx)) & 0xff) != 0);
                }
            }
            const long long at = ((long long)side * B + b) * N + n;
            cells[at] = make_float4(wy, wx, v ? 1.f : 0.f, 0.f);
            if (warped) { warped[2 * at] = wy; warped[2 * at + 1] = wx; }
            cnt[side] = v ? 1 : 0;
        }
    }
    block_sum<int, 2>(cnt, red_i);
    if (threadIdx.x == 0) {
        const long long at = ((long long)b * gridDim.x + blockIdx.x) * 2;
        cnt_part[at] = cnt[0];
        cnt_part[at + 1] = cnt[1];
    }
}

// One workgroup (4 waves) per 128 x 128 tile of image b: rows i = cells of side 2, columns j = cells of side 1 (the
// reference's dot_product_desc[b][i][j] = desc2[i] . desc1[j]).  Wave w owns the 64 x 64 quarter (w >> 1, w & 1) as 2 x 2
// blocks of 32 x 32; v_mfma_f32_32x32x2_f32 with the desc2 fragment as A: accumulator r of lane l is row
// 8 (r >> 2) + 4 (l >> 5) + (r & 3), column l & 31 of its block.
template <int D>
__global__ __launch_bounds__(RED) void desc_loss_tile_kernel(const float* __restrict__ desc1,
                                                            const float* __restrict__ desc2,
                                                            const float4* __restrict__ cells, int B, int N, float s_max,
                                                            float pos_margin, float neg_margin, int use_mask,
                                                            float* __restrict__ tile_part)
{
    __shared__ __attribute__((aligned(16))) float As[LT * KRS];
    __shared__ __attribute__((aligned(16))) float Bs[LT * KRS];
    __shared__ float4 rinfo[LT], cinfo[LT];
    __shared__ float red[4][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, half = lane >> 5;
    const int b = blockIdx.z, i0 = blockIdx.y * LT, j0 = blockIdx.x * LT;
    const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
    const float* X2 = desc2 + (long long)b * N * D;
    const float* X1 = desc1 + (long long)b * N * D;

    {   // per-cell data: (warped y, warped x, weight); weight = validity with the mask, 1 without; 0 outside the image
        const int t = tid & (LT - 1), side = tid < LT ? 1 : 0;          // rows: side 2, columns: side 1
        const int cell = (side ? i0 : j0) + t;
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
        if (cell < N) {
            c = cells[((long long)side * B + b) * N + cell];
            if (!use_mask) c.z = 1.f;
        }
        (side ? rinfo : cinfo)[t] = c;
    }

    // staging: 128 rows x KC floats of each operand = 1024 granules of 16 bytes, 4 per thread (rows past N repeat row N - 1;
    // their weight is 0)
    constexpr int GPT = LT * KC / 4 / RED, GPR = KC / 4;
    f32x4 sa[GPT], sb[GPT];
    auto gload = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < GPT; ++q) {
            const int gran = tid + q * RED, row = gran / GPR, c4 = gran - row * GPR;
            sa[q] = *reinterpret_cast<const f32x4*>(X2 + (long long)min(i0 + row, N - 1) * D + k0 + c4 * 4);
            sb[q] = *reinterpret_cast<const f32x4*>(X1 + (long long)min(j0 + row, N - 1) * D + k0 + c4 * 4);
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int si = 0; si < 2; ++si)
#pragma unroll
        for (int sj = 0; sj < 2; ++sj)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[si][sj][r] = 0.f;

    gload(0);
    for (int k0 = 0; k0 < D; k0 += KC) {
#pragma unroll
        for (int q = 0; q < GPT; ++q) {
            const int gran = tid + q * RED, row = gran / GPR, c4 = gran - row * GPR;
            *reinterpret_cast<f32x4*>(&As[row * KRS + c4 * 4]) = sa[q];
            *reinterpret_cast<f32x4*>(&Bs[row * KRS + c4 * 4]) = sb[q];
        }
        __syncthreads();
        if (k0 + KC < D) gload(k0 + KC);                 // in flight across this chunk's MFMAs
#pragma unroll
        for (int g = 0; g < KC / 8; ++g) {
            // lanes of half h supply k = g*8 + 4h + e to the e-th MFMA: the same k mapping for both operands
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(&As[(wi + li) * KRS + g * 8 + half * 4]);
            const f32x4 a1 = *reinterpret_cast<const f32x4*>(&As[(wi + 32 + li) * KRS + g * 8 + half * 4]);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(&Bs[(wj + li) * KRS + g * 8 + half * 4]);
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(&Bs[(wj + 32 + li) * KRS + g * 8 + half * 4]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[e], b0[e], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[e], b1[e], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[e], b0[e], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[e], b1[e], acc[1][1], 0, 0, 0);
            }
        }
        __syncthreads();                                 // before the next chunk overwrites the operands
    }

    // epilogue: corr = |w1[j] - w2[i]| <= threshold, pos = corr * max(0, m_p - dot), neg = (1 - corr) * max(0, dot - m_n),
    // each times the pair's weight; lambda_d is applied by the reduction
    float pos = 0.f, neg = 0.f, cnt = 0.f;
#pragma unroll
    for (int sj = 0; sj < 2; ++sj) {
        const float4 cj = cinfo[wj + sj * 32 + li];
#pragma unroll
        for (int si = 0; si < 2; ++si) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float4 ci = rinfo[wi + si * 32 + 8 * (r >> 2) + 4 * half + (r & 3)];
                const float dy = __fsub_rn(cj.x, ci.x), dx = __fsub_rn(cj.y, ci.y);
                const float s = __fadd_rn(__fmul_rn(dy, dy), __fmul_rn(dx, dx));
                const float w = ci.z * cj.z;
                const float c = s <= s_max ? w : 0.f;
                const float dot = acc[si][sj][r];
                pos = fmaf(c, fmaxf(pos_margin - dot, 0.f), pos);
                neg = fmaf(w - c, fmaxf(dot - neg_margin, 0.f), neg);
                cnt += c;
            }
        }
    }
    // fixed-order reduction: the wave by butterflies, then the four waves in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        pos += __shfl_xor(pos, o);
        neg += __shfl_xor(neg, o);
        cnt += __shfl_xor(cnt, o);
    }
    if (lane == 0) { red[wave][0] = pos; red[wave][1] = neg; red[wave][2] = cnt; }
    __syncthreads();
    if (tid < 3) {
        const float v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        const long long t = ((long long)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        tile_part[t * 3 + tid] = v;
    }
}

__global__ __launch_bounds__(RED) void descriptor_reduce_kernel(const float* __restrict__ tile_part, int T,
                                                               const int* __restrict__ cnt_part, int nblk, int N,
                                                               int use_mask, double lambda_d, double* __restrict__ out)
{
    __shared__ double red_d[3][RED];
    __shared__ long long red_l[2][RED];
    const int b = blockIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    long long c[2] = {0, 0};
    for (int t = threadIdx.x; t < T; t += RED) {
        const float* p = tile_part + ((long long)b * T + t) * 3;
        s[0] += (double)p[0];
        s[1] += (double)p[1];
        s[2] += (double)p[2];
    }
    for (int t = threadIdx.x; t < nblk; t += RED) {
        c[0] += cnt_part[((long long)b * nblk + t) * 2];
        c[1] += cnt_part[((long long)b * nblk + t) * 2 + 1];
    }
    block_sum<double, 3>(s, red_d);
    block_sum<long long, 2>(c, red_l);
    if (threadIdx.x == 0) {
        out[4 * b] = lambda_d * s[0];
        out[4 * b + 1] = s[1];
        out[4 * b + 2] = s[2];
        out[4 * b + 3] = use_mask ? (double)c[0] * (double)c[1] : (double)N * (double)N;
    }
}

// ---- backward (the gradient of the loss; every kernel recomputes what it needs from the forward's inputs) ----

// One thread per cell: dlogits[c] = gamma * valid / (B * count_b) * d(loss)/d(logit_c).  CE: softmax - onehot(label), the
// label as the forward picks it; BCE: torch's binary_cross_entropy backward gp_c = (p_c - y_c) / max(p_c (1 - p_c), 1e-12)
// chained through the softmax, p (gp - sum_c p_c gp_c).  A zero count gives NaN (0 * inf), as the reference's autograd.
__global__ __launch_bounds__(RED) void detector_loss_backward_kernel(const float* __restrict__ logits,
                                                                    const unsigned char* __restrict__ kp,
                                                                    const unsigned char* __restrict__ valid,
                                                                    const float* __restrict__ noise,
                                                                    unsigned long long seed, int B, int H, int W,
                                                                    int use_ce, const double* __restrict__ fwd_out,
                                                                    const double* __restrict__ coef,
                                                                    float* __restrict__ grad)
{
    const int Hc = H >> 3, Wc = W >> 3, N = Hc * Wc;
    const int b = blockIdx.y;
    const int n = blockIdx.x * RED + threadIdx.x;
    if (n >= N) return;
    const int hc = n / Wc, wc = n - hc * Wc;
    const long long pix0 = ((long long)b * H + hc * 8) * W + wc * 8;
    bool vcell = true;
    unsigned long long bits = 0;
#pragma unroll
    for (int dy = 0; dy < 8; ++dy) {
        const unsigned long long kr = *reinterpret_cast<const unsigned long long*>(kp + pix0 + (long long)dy * W);
        const unsigned long long vr = valid ? *reinterpret_cast<const unsigned long long*>(valid + pix0 + (long long)dy * W)
                                            : ~0ull;
#pragma unroll
        for (int dx = 0; dx < 8; ++dx) {
            bits |= (unsigned long long)(((kr >> (8 * dx)) & 0xff) != 0) << (8 * dy + dx);
            vcell = vcell && (((vr >> (8 * dx)) & 0xff) != 0);
        }
    }
    const float scale = (float)(coef[0] / ((double)B * fwd_out[2 * b + 1])) * (vcell ? 1.f : 0.f);
    const float* lg = logits + (long long)b * 65 * N + n;
    float* gd = grad + (long long)b * 65 * N + n;
    float m = -__builtin_inff();
    for (int c = 0; c < 65; ++c) m = fmaxf(m, lg[(long long)c * N]);
    float se = 0.f;
    for (int c = 0; c < 65; ++c) se += expf(lg[(long long)c * N] - m);
    if (use_ce) {
        int label = 64;
        float best = 2.f;
        for (unsigned long long rest = bits; rest; rest &= rest - 1) {
            const int c = __builtin_ctzll(rest);
            const float u = noise ? noise[(((long long)b * 64 + c) * Hc + hc) * Wc + wc] : hash_noise(seed, b, c, hc, wc, Hc, Wc);
            const float v = __fadd_rn(3.f, u);
            if (v > best) { best = v; label = c; }
        }
        for (int c = 0; c < 65; ++c) {
            const float p = expf(lg[(long long)c * N] - m) / se;
            gd[(long long)c * N] = scale * (c == label ? p - 1.f : p);
        }
    } else {
        const int k = __builtin_popcountll(bits);
        const float dust = k ? 0.f : 1.f;
        const float S = (float)k + dust;
        auto gp = [&](int c, float p) __attribute__((always_inline)) {
            const float y = (c < 64 ? (float)((bits >> c) & 1) : dust) / S;
            return (p - y) / fmaxf(p * (1.f - p), 1e-12f);
        };
        float dot = 0.f;
        for (int c = 0; c < 65; ++c) {
            const float p = expf(lg[(long long)c * N] - m) / se;
            dot = fmaf(p, gp(c, p), dot);
        }
        for (int c = 0; c < 65; ++c) {
            const float p = expf(lg[(long long)c * N] - m) / se;
            gd[(long long)c * N] = scale * (p * (gp(c, p) - dot));
        }
    }
}

// torch's maximum(0, x) backward: 1 above, 1/2 at the tie, 0 below
__device__ __forceinline__ float hinge_grad(float x) { return x > 0.f ? 1.f : (x == 0.f ? 0.5f : 0.f); }

// dX_own[j] = sum_i G[i][j] X_other[i] for one side ("own"), G[i][j] = (-alpha lambda_d c h(m_p - dot) + beta (w - c)
// h(dot - m_n)) / (B norm_b).  G is symmetric under swapping the sides with their cell data, so one template serves
// both gradients.  A workgroup (4 waves) owns OWN = 128 own cells, 32 per wave, and walks the other side in tiles of TI
// rows in a fixed order:
//   dot   v_mfma_f32_32x32x2_f32 with the other side's rows as A and the wave's own cells (held in registers) as B: the
//         accumulator's register r of lane l is other row 8 (r >> 2) + 4 (l >> 5) + (r & 3), own cell l & 31; the k
//         mapping is the forward tile kernel's.  Every hinge and tie is decided on this kernel's own fp32 dot; in the
//         launch with side 1 as own the operand roles are also the forward's, in the other launch A and B are exchanged
//   G     formed in place in the dot registers
//   dX    += G^T X_other, summed over the accumulator's row index: MFMA r takes dot register r as A, and the B operand of
//         lane half h is the other side's row 8 (r >> 2) + 4h + (r & 3), channels d0 + (l & 31); no LDS transpose.
//         Accumulator register r of block db is own cell 8 (r >> 2) + 4h + (r & 3), channel 32 db + (l & 31).
// Each own cell's gradient is written once: no atomics, bit-identical from run to run.
template <int D>
struct GradShape {
    static constexpr int TI = D <= 128 ? 64 : 32;          // other-side rows per tile (2 or 1 dot blocks of 32)
};

template <int D>
__global__ __launch_bounds__(RED) void desc_loss_grad_kernel(const float* __restrict__ x_own,
                                                            const float* __restrict__ x_other,
                                                            const float4* __restrict__ cells_own,
                                                            const float4* __restrict__ cells_other, int B, int N,
                                                            float s_max, float pos_margin, float neg_margin,
                                                            float lambda_d, int use_mask,
                                                            const double* __restrict__ fwd_out,
                                                            const double* __restrict__ coef,
                                                            float* __restrict__ grad_own)
{
    constexpr int TI = GradShape<D>::TI, NT = TI / 32, RS = D + 4, NDB = D / 32;
    __shared__ __attribute__((aligned(16))) float Xs[TI * RS];
    __shared__ float4 oinfo[TI];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, half = lane >> 5;
    const int b = blockIdx.y;
    const int j = blockIdx.x * (4 * 32) + wave * 32 + li;            // this lane's own cell
    const float* Xo = x_other + (long long)b * N * D;
    const float4* co = cells_other + (long long)b * N;

    // per-image coefficients (double on the device: no host synchronisation); a zero norm makes every G NaN
    const double inv = 1.0 / ((double)B * fwd_out[4 * b + 3]);
    const float ka = (float)(-coef[0] * (double)lambda_d * inv), kb = (float)(coef[1] * inv);

    // the own cell's descriptor as the B operand of the dot: lane half h supplies k = 8g + 4h + e to MFMA (g, e)
    f32x4 own[D / 8];
    {
        const float* xr = x_own + ((long long)b * N + min(j, N - 1)) * D + half * 4;
#pragma unroll
        for (int g = 0; g < D / 8; ++g) own[g] = *reinterpret_cast<const f32x4*>(xr + g * 8);
    }
    float4 cj = j < N ? cells_own[(long long)b * N + j] : make_float4(0.f, 0.f, 0.f, 0.f);
    if (!use_mask) cj.z = 1.f;

    f32x16 dx[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) dx[db][r] = 0.f;

    // staging of a TI x D tile: granules of 16 bytes, GPT per thread; rows past N are zero (their G is 0 too)
    constexpr int GPR = D / 4, GPT = TI * GPR / RED;
    f32x4 st[GPT];
    auto gload = [&](int i0) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < GPT; ++q) {
            const int gran = tid + q * RED, row = gran / GPR, c4 = gran - row * GPR;
            st[q] = i0 + row < N ? *reinterpret_cast<const f32x4*>(Xo + (long long)(i0 + row) * D + c4 * 4)
                                 : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    gload(0);
    for (int i0 = 0; i0 < N; i0 += TI) {
#pragma unroll
        for (int q = 0; q < GPT; ++q) {
            const int gran = tid + q * RED, row = gran / GPR, c4 = gran - row * GPR;
            *reinterpret_cast<f32x4*>(&Xs[row * RS + c4 * 4]) = st[q];
        }
        if (tid < TI) {
            float4 c = make_float4(0.f, 0.f, 0.f, 0.f);           // .w: the row is a cell of the image
            if (i0 + tid < N) {
                c = co[i0 + tid];
                if (!use_mask) c.z = 1.f;
                c.w = 1.f;
            }
            oinfo[tid] = c;
        }
        __syncthreads();
        if (i0 + TI < N) gload(i0 + TI);                          // in flight across this tile's MFMAs

        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
#pragma unroll
        for (int g = 0; g < D / 8; ++g) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(&Xs[(t * 32 + li) * RS + g * 8 + half * 4]);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], own[g][e], acc[t], 0, 0, 0);
            }
        }

        // G in place, with the forward's fp32 correspondence test and hinge arguments
#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float4 ci = oinfo[t * 32 + 8 * (r >> 2) + 4 * half + (r & 3)];
                const float dy = __fsub_rn(cj.x, ci.x), dxx = __fsub_rn(cj.y, ci.y);
                const float s = __fadd_rn(__fmul_rn(dy, dy), __fmul_rn(dxx, dxx));
                const float w = ci.z * cj.z;
                const float c = s <= s_max ? w : 0.f;
                const float dot = acc[t][r];
                const float gv = c * hinge_grad(pos_margin - dot) * ka + (w - c) * hinge_grad(dot - neg_margin) * kb;
                acc[t][r] = ci.w != 0.f ? gv : 0.f;
            }
        }

#pragma unroll
        for (int t = 0; t < NT; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* xr = &Xs[(t * 32 + 8 * (r >> 2) + 4 * half + (r & 3)) * RS + li];
#pragma unroll
                for (int db = 0; db < NDB; ++db)
                    dx[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(acc[t][r], xr[db * 32], dx[db], 0, 0, 0);
            }
        }
        __syncthreads();                                          // before the next tile overwrites Xs / oinfo
    }

    const int jb = blockIdx.x * (4 * 32) + wave * 32;
    float* go = grad_own + (long long)b * N * D;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int jj = jb + 8 * (r >> 2) + 4 * half + (r & 3);
        if (jj < N) {
#pragma unroll
            for (int db = 0; db < NDB; ++db) go[(long long)jj * D + db * 32 + li] = dx[db][r];
        }
    }
}

struct LossWorkspace {
    float4* cells;          // [2][B][N]       warped centre (y, x), validity
    float* tile_part;       // [B][T][3]       per-tile positive, negative, corresponding pairs
    int* cnt_part;          // [B][nblk][2]    valid cells per prologue workgroup, side 1 / side 2
    float* det_sum;         // [B][nblk]       detector loss per workgroup
    int* det_cnt;           // [B][nblk]       valid cells per workgroup
    size_t bytes;
};

LossWorkspace loss_workspace(void* base, int B, int H, int W)
{
    const long long N = (long long)(H >> 3) * (W >> 3);
    const long long nt = (N + LT - 1) / LT, T = nt * nt, nblk = (N + RED - 1) / RED;
    Carver c(base);
    LossWorkspace w;
    w.cells = c.take<float4>(2 * B * N);
    w.tile_part = c.take<float>(3 * B * T);
    w.cnt_part = c.take<int>(2 * B * nblk);
    w.det_sum = c.take<float>(B * nblk);
    w.det_cnt = c.take<int>(B * nblk);
    w.bytes = c.bytes();
    return w;
}

}  // namespace

size_t loss_workspace_bytes(int B, int H, int W)
{
    return loss_workspace(nullptr, B, H, W).bytes;
}

void launch_detector_loss(const float* logits, const unsigned char* kp, const unsigned char* valid, const float* noise,
                          unsigned long long seed, int B, int H, int W, int use_ce, void* workspace, double* out,
                          hipStream_t s)
{
    const LossWorkspace w = loss_workspace(workspace, B, H, W);
    const int N = (H >> 3) * (W >> 3), nblk = (N + RED - 1) / RED;
    hipLaunchKernelGGL(detector_loss_kernel, dim3(nblk, B), dim3(RED), 0, s, logits, kp, valid, noise, seed, H, W, use_ce,
                       w.det_sum, w.det_cnt);
    hipLaunchKernelGGL(detector_reduce_kernel, dim3(B), dim3(RED), 0, s, w.det_sum, w.det_cnt, nblk, out);
}

void launch_descriptor_loss(const float* desc1, const float* desc2, const float* hom1, const float* hom2,
                            const unsigned char* valid1, const unsigned char* valid2, int B, int H, int W, int D,
                            float s_max, float pos_margin, float neg_margin, double lambda_d, int use_mask,
                            void* workspace, double* out, float* warped, hipStream_t s)
{
    const LossWorkspace w = loss_workspace(workspace, B, H, W);
    const int N = (H >> 3) * (W >> 3), nblk = (N + RED - 1) / RED, nt = (N + LT - 1) / LT;
    hipLaunchKernelGGL(desc_prologue_kernel, dim3(nblk, B), dim3(RED), 0, s, hom1, hom2, valid1, valid2, B, H, W, w.cells,
                       warped, w.cnt_part);
    const dim3 grid(nt, nt, B);
    if (D == 64)
        hipLaunchKernelGGL(desc_loss_tile_kernel<64>, grid, dim3(RED), 0, s, desc1, desc2, w.cells, B, N, s_max, pos_margin,
                           neg_margin, use_mask, w.tile_part);
    else if (D == 128)
        hipLaunchKernelGGL(desc_loss_tile_kernel<128>, grid, dim3(RED), 0, s, desc1, desc2, w.cells, B, N, s_max, pos_margin,
                           neg_margin, use_mask, w.tile_part);
    else
        hipLaunchKernelGGL(desc_loss_tile_kernel<256>, grid, dim3(RED), 0, s, desc1, desc2, w.cells, B, N, s_max, pos_margin,
                           neg_margin, use_mask, w.tile_part);
    hipLaunchKernelGGL(descriptor_reduce_kernel, dim3(B), dim3(RED), 0, s, w.tile_part, nt * nt, w.cnt_part, nblk, N, use_mask,
                       lambda_d, out);
}

void launch_detector_loss_backward(const float* logits, const unsigned char* kp, const unsigned char* valid,
                                   const float* noise, unsigned long long seed, int B, int H, int W, int use_ce,
                                   const double* fwd_out, const double* coef, float* grad, hipStream_t s)
{
    const int N = (H >> 3) * (W >> 3), nblk = (N + RED - 1) / RED;
    hipLaunchKernelGGL(detector_loss_backward_kernel, dim3(nblk, B), dim3(RED), 0, s, logits, kp, valid, noise, seed, B, H, W,
                       use_ce, fwd_out, coef, grad);
}

namespace {
template <int D>
void launch_desc_grad_sides(const float* desc1, const float* desc2, const float4* cells, int B, int N, float s_max,
                            float pos_margin, float neg_margin, float lambda_d, int use_mask, const double* fwd_out,
                            const double* coef, float* grad1, float* grad2, hipStream_t s)
{
    const dim3 grid((N + 127) / 128, B);
    const float4* c1 = cells;
    const float4* c2 = cells + (long long)B * N;
    if (grad1)                                               // a NULL gradient: that side is not needed
        hipLaunchKernelGGL(desc_loss_grad_kernel<D>, grid, dim3(RED), 0, s, desc1, desc2, c1, c2, B, N, s_max, pos_margin,
                           neg_margin, lambda_d, use_mask, fwd_out, coef, grad1);
    if (grad2)
        hipLaunchKernelGGL(desc_loss_grad_kernel<D>, grid, dim3(RED), 0, s, desc2, desc1, c2, c1, B, N, s_max, pos_margin,
                           neg_margin, lambda_d, use_mask, fwd_out, coef, grad2);
}
}  // namespace

void launch_descriptor_loss_backward(const float* desc1, const float* desc2, const float* hom1, const float* hom2,
                                     const unsigned char* valid1, const unsigned char* valid2, int B, int H, int W, int D,
                                     float s_max, float pos_margin, float neg_margin, float lambda_d, int use_mask,
                                     const double* fwd_out, const double* coef, void* workspace, float* grad1,
                                     float* grad2, hipStream_t s)
{
    const LossWorkspace w = loss_workspace(workspace, B, H, W);
    const int N = (H >> 3) * (W >> 3), nblk = (N + RED - 1) / RED;
    hipLaunchKernelGGL(desc_prologue_kernel, dim3(nblk, B), dim3(RED), 0, s, hom1, hom2, valid1, valid2, B, H, W, w.cells,
                       nullptr, w.cnt_part);
    if (D == 64)
        launch_desc_grad_sides<64>(desc1, desc2, w.cells, B, N, s_max, pos_margin, neg_margin, lambda_d, use_mask, fwd_out,
                                   coef, grad1, grad2, s);
    else if (D == 128)
        launch_desc_grad_sides<128>(desc1, desc2, w.cells, B, N, s_max, pos_margin, neg_margin, lambda_d, use_mask, fwd_out,
                                    coef, grad1, grad2, s);
    else
        launch_desc_grad_sides<256>(desc1, desc2, w.cells, B, N, s_max, pos_margin, neg_margin, lambda_d, use_mask, fwd_out,
                                    coef, grad1, grad2, s);
}
