// Photometric augmentation (reference multipoint/datasets/augmentation/photometric_augmentation.py, driven by
// augmentation.py:8-22) for a batch of n fp32 images [n][H][W] with one host-drawn plan per image.
//
// The plans list their primitives in the order they run; images of one batch may run them in different orders.  The
// launcher walks the steps s = 0 .. max(n_ops) - 1 and at each step launches, for the whole batch,
//   photo_mean_kernel       (if some plan has random_contrast at s) one workgroup per image: numpy's float32 image.mean()
//                           bit for bit -- the C-order pixels in chunks of 8192 (the reduction iterator's buffer), each
//                           chunk a pairwise sum (8 accumulators, leaves of <= 128, splits at n/2 - (n/2) % 8), the chunk
//                           sums accumulated in order, divided by H*W in float32
//   shade_ellipse_kernel    (if some plan has additive_shade at s) one workgroup per (ellipse, image): cv::ellipse(...,
//                           thickness -1) -- EllipseEx / ellipse2Poly vertices in 16.16 fixed point, the LINE_8 outline
//                           (one lane per edge), the FillConvexPoly edge walk (one lane) and the spans (all lanes).  Each
//                           pixel write stores 1.0, so the ellipses of one image need no ordering and no atomics.
//   blur_weights_kernel     getGaussianKernel(k, 0, CV_32F) per image: exp in double, stored as float, normalised
//   blur_rows_kernel        the row filter of sepFilter2D through LDS: taps summed left to right, BORDER_REFLECT_101
//   blur_cols_kernel        the symmetric column filter through LDS: ky[r] S[0] + sum_j ky[r+j] (S[+j] + S[-j])
//   photo_step_kernel       one thread per pixel: the elementwise primitive of step s (noise, speckle, brightness, contrast,
//                           shade) in place, or motion blur (cv2.filter2D) from the current into the other buffer
// and at the end copies the images whose plan ran an odd number of motion blurs back from the ping-pong buffer.
//
// All pixel arithmetic follows numpy's float32 operation order with every step rounded (no contraction into FMA).
#include "mp_common.h"
#include "mp_device.h"
#include "mp_raster.h"
#include "mp_workspace.h"
#include "../../include/multipoint_hip.h"

#pragma clang fp contract(off)

static_assert(sizeof(mp_photometric_op) == 88 && sizeof(mp_photometric_plan) == 1416,
              "mp_photometric_plan layout: multipoint_amd/_lib.py binds it with ctypes");

namespace {

using namespace mp_raster;             // the 16.16 drawing rules shared with shapes.hip
constexpr int MEAN_CHUNK = 8192;        // numpy's iterator buffer (np.getbufsize())
constexpr int MEAN_LEAVES = 160;        // pairwise leaves of a chunk of <= 8192 (leaves hold >= 57 elements: 8192 -> 128)
constexpr int MEAN_GROUP = 16;          // chunks whose leaves are summed in one parallel pass
constexpr int FULL_LEAVES = 64;         // a chunk of 8192 halves evenly down to 64 leaves of 128: a balanced tree
constexpr int COL_TX = 16, COL_TY = 64; // column-filter tile (columns x output rows)
constexpr int STACK = 64;               // pairwise-tree walk stacks (depth <= 7 for a chunk of 8192)
// static LDS of shade_ellipse_kernel (vx, vy, rx, ry and three ints) in front of its dynamic spans, rounded up to 16 bytes
constexpr size_t SHADE_STATIC_LDS = (4 * MAX_VERTS * sizeof(long long) + 3 * sizeof(int) + 15) & ~(size_t)15;

// device noise: normals by Box-Muller from the counters 2p and 2p + 1 of hash_uniform (mp_device.h)
__device__ __forceinline__ double hash_normal(unsigned long long key, unsigned long long p)
{
    const double u1 = ((double)(mix64(key ^ mix64(2 * p)) >> 11) + 0.5) * 0x1p-53;     // (0, 1)
    const double u2 = hash_uniform(key, 2 * p + 1);
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// ---------------------------------------------------------------------------------------------
// image.mean()
// ---------------------------------------------------------------------------------------------
// leaves of numpy's pairwise_sum over n elements, left to right (explicit stacks in LDS: no recursion, no scratch)
__device__ int pairwise_leaves(int n, int* start, int* len, int* st_off, int* st_n)
{
    int sp = 0, cnt = 0;
    st_off[sp] = 0; st_n[sp] = n; ++sp;
    while (sp > 0) {
        --sp;
        const int o = st_off[sp], m = st_n[sp];
        if (m <= 128) {
            start[cnt] = o; len[cnt] = m; ++cnt;
        } else {
            int m2 = m / 2;
            m2 -= m2 % 8;
            st_off[sp] = o + m2; st_n[sp] = m - m2; ++sp;      // right, popped after the left subtree
            st_off[sp] = o; st_n[sp] = m2; ++sp;
        }
    }
    return cnt;
}

// the sum of the tree over n elements from its leaf sums (in leaf order): the post-order combination of pairwise_sum
__device__ float pairwise_combine(int n, const float* leaf, int* st_n, float* val)
{
    int sp = 0, next = 0, vp = 0;              // st_n < 0 marks "combine the top two values"
    st_n[sp++] = n;
    while (sp > 0) {
        const int m = st_n[--sp];
        if (m < 0) {
            const float b = val[--vp], a = val[--vp];
            val[vp++] = a + b;
        } else if (m <= 128) {
            val[vp++] = leaf[next++];
        } else {
            int m2 = m / 2;
            m2 -= m2 % 8;
            st_n[sp++] = -1;
            st_n[sp++] = m - m2;
            st_n[sp++] = m2;
        }
    }
    return val[0];
}

__device__ float leaf_sum(const float* a, int n)
{
    if (n < 8) {
        float res = 0.f;
        for (int i = 0; i < n; ++i) res = res + a[i];
        return res;
    }
    float r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - n % 8; i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = r[j] + a[i + j];
    }
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res = res + a[i];
    return res;
}

__global__ __launch_bounds__(256) void photo_mean_kernel(const float* const* cur_ptrs, const mp_photometric_plan* plans,
                                                         int step, long long HW, float* mean)
{
    const int img = blockIdx.x;
    if (step >= plans[img].n_ops || plans[img].op[step].kind != MP_PHOTO_CONTRAST) return;
    const float* x = cur_ptrs[img];
    __shared__ int full_start[MEAN_LEAVES], full_len[MEAN_LEAVES], tail_start[MEAN_LEAVES], tail_len[MEAN_LEAVES];
    __shared__ float leaf[MEAN_GROUP * MEAN_LEAVES];
    __shared__ int nl_full, nl_tail, st_a[STACK], st_b[STACK];
    __shared__ float st_v[STACK];
    const long long nchunks = (HW + MEAN_CHUNK - 1) / MEAN_CHUNK;
    const int tail = (int)(HW - (nchunks - 1) * MEAN_CHUNK);
    if (threadIdx.x == 0) {
        nl_full = pairwise_leaves(MEAN_CHUNK, full_start, full_len, st_a, st_b);
        nl_tail = pairwise_leaves(tail, tail_start, tail_len, st_a, st_b);
    }
    __syncthreads();
    float acc = 0.f;                                  // thread 0's running total
    for (long long c0 = 0; c0 < nchunks; c0 += MEAN_GROUP) {
        const int g = (int)min((long long)MEAN_GROUP, nchunks - c0);
        for (int t = threadIdx.x; t < g * MEAN_LEAVES; t += blockDim.x) {
            const int c = t / MEAN_LEAVES, l = t % MEAN_LEAVES;
            const bool last = c0 + c == nchunks - 1;
            if (l < (last ? nl_tail : nl_full)) {
                const int s = last ? tail_start[l] : full_start[l], n = last ? tail_len[l] : full_len[l];
                leaf[t] = leaf_sum(x + (c0 + c) * MEAN_CHUNK + s, n);
            }
        }
        __syncthreads();
        // the full chunks' trees level by level (node = left + right, as the recursion adds them)
        for (int w = FULL_LEAVES / 2; w >= 1; w >>= 1) {
            float v[(MEAN_GROUP * FULL_LEAVES / 2 + 255) / 256];
#pragma unroll
            for (int k = 0; k < (int)(sizeof(v) / sizeof(v[0])); ++k) {
                const int t = threadIdx.x + 256 * k, c = t / w, j = t % w;
                if (c < g) v[k] = leaf[c * MEAN_LEAVES + 2 * j] + leaf[c * MEAN_LEAVES + 2 * j + 1];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < (int)(sizeof(v) / sizeof(v[0])); ++k) {
                const int t = threadIdx.x + 256 * k, c = t / w, j = t % w;
                const bool full = c0 + c < nchunks - 1 || tail == MEAN_CHUNK;
                if (c < g && full) leaf[c * MEAN_LEAVES + j] = v[k];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0)
            for (int c = 0; c < g; ++c) {
                const bool full = c0 + c < nchunks - 1 || tail == MEAN_CHUNK;
                acc = acc + (full ? leaf[c * MEAN_LEAVES] : pairwise_combine(tail, leaf + c * MEAN_LEAVES, st_a, st_v));
            }
        __syncthreads();
    }
    if (threadIdx.x == 0) mean[img] = acc / (float)HW;
}

// ---------------------------------------------------------------------------------------------
// additive_shade: cv::ellipse fill + GaussianBlur
// ---------------------------------------------------------------------------------------------
// one workgroup (one wave) per (ellipse, image); dynamic LDS: 2 ints per row of the frame (the spans)
__global__ __launch_bounds__(64) void shade_ellipse_kernel(const mp_photometric_plan* plans, const int* ellipses, int step,
                                                           int H, int W, float* mask)
{
    const int img = blockIdx.y, e = blockIdx.x;
    if (step >= plans[img].n_ops) return;
    const mp_photometric_op& op = plans[img].op[step];
    if (op.kind != MP_PHOTO_SHADE || e >= op.ellipse_count) return;
    const int* el = ellipses + 5 * (op.ellipse_offset + e);
    float* m = mask + (long long)img * H * W;
    __shared__ long long vx[MAX_VERTS], vy[MAX_VERTS], rx[MAX_VERTS], ry[MAX_VERTS];
    __shared__ int npts_s, ylo_s, yhi_s;
    extern __shared__ int spans[];             // [H][2]: xx1, xx2 of row y (xx1 > xx2: empty row)
    ellipse_poly(el, vx, vy, rx, ry, &npts_s);
    const int npts = npts_s;
    const auto put = [&](long long x, long long y) {
        if (0 <= x && x < W && 0 <= y && y < H) m[y * (long long)W + x] = 1.f;
    };
    // the outline: edge t runs from vertex t-1 (npts-1 for t = 0) to vertex t
    for (int t = threadIdx.x; t < npts; t += blockDim.x) {
        const int t0 = t == 0 ? npts - 1 : t - 1;
        line2(H, W, vx[t0], vy[t0], vx[t], vy[t], put);
    }
    if (threadIdx.x == 0) {
        int ylo = 0, yhi = -1;                              // rows [ylo, yhi] have spans
        convex_spans(vx, vy, npts, H, W, [&](int y, int a, int b) {
            if (yhi < 0) ylo = y;
            spans[2 * y] = a;
            spans[2 * y + 1] = b;
            yhi = y;
        });
        ylo_s = ylo;
        yhi_s = yhi;
    }
    __syncthreads();
    for (int y = ylo_s; y <= yhi_s; ++y) {
        const int a = spans[2 * y], b = spans[2 * y + 1];
        for (int x = a + (int)threadIdx.x; x <= b; x += blockDim.x) m[(long long)y * W + x] = 1.f;
    }
}

// the blur size of image `img`: its shade op at `step`, or ksizes[img] when the caller blurs plain frames (0: no blur)
__device__ __forceinline__ int blur_ksize(const mp_photometric_plan* plans, int step, const int* ksizes, int img)
{
    if (ksizes) return ksizes[img];
    return step < plans[img].n_ops && plans[img].op[step].kind == MP_PHOTO_SHADE ? plans[img].op[step].ksize : 0;
}

// getGaussianKernel(k, 0, CV_32F): weights [n][MP_PHOTO_MAX_BLUR]
__global__ __launch_bounds__(64) void blur_weights_kernel(const mp_photometric_plan* plans, int step, const int* ksizes,
                                                          float* weights)
{
    const int img = blockIdx.x;
    const int k = blur_ksize(plans, step, ksizes, img);
    if (k == 0) return;
    float* w = weights + (long long)img * MP_PHOTO_MAX_BLUR;
    const double sigma = ((k - 1) * 0.5 - 1) * 0.3 + 0.8;
    const double scale2x = -0.5 / (sigma * sigma);
    for (int i = threadIdx.x; i < k; i += blockDim.x) {
        const double x = i - (k - 1) * 0.5;
        w[i] = (float)exp(scale2x * x * x);
    }
    __syncthreads();
    __shared__ double inv;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < k; ++i) s += (double)w[i];
        inv = 1.0 / s;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < k; i += blockDim.x) w[i] = (float)((double)w[i] * inv);
}

// row filter: one workgroup per (row, image); dynamic LDS: the reflected row (W + 2r) and the k weights
__global__ __launch_bounds__(256) void blur_rows_kernel(const mp_photometric_plan* plans, int step, const int* ksizes,
                                                        const float* weights, const float* mask, int H, int W, float* tmp)
{
    const int img = blockIdx.y, y = blockIdx.x;
    const int k = blur_ksize(plans, step, ksizes, img), r = k / 2;
    if (k == 0) return;
    extern __shared__ float lds[];
    float* w = lds;
    float* ext = lds + k;
    const float* src = mask + ((long long)img * H + y) * W;
    for (int i = threadIdx.x; i < k; i += blockDim.x) w[i] = weights[(long long)img * MP_PHOTO_MAX_BLUR + i];
    for (int i = threadIdx.x; i < W + 2 * r; i += blockDim.x) ext[i] = src[reflect101(i - r, W)];
    __syncthreads();
    float* dst = tmp + ((long long)img * H + y) * W;
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        float s = w[0] * ext[x];
        for (int j = 1; j < k; ++j) s = s + w[j] * ext[x + j];
        dst[x] = s;
    }
}

// symmetric column filter: one workgroup per (COL_TX columns, COL_TY rows, image); 256 threads = COL_TX columns x 8
// row groups; dynamic LDS: the k weights and the reflected input rows [COL_TY + 2r][COL_TX]
__global__ __launch_bounds__(256) void blur_cols_kernel(const mp_photometric_plan* plans, int step, const int* ksizes,
                                                        const float* weights, const float* tmp, int H, int W, float* mask)
{
    const int img = blockIdx.z;
    const int k = blur_ksize(plans, step, ksizes, img), r = k / 2;
    if (k == 0) return;
    const int x0 = blockIdx.x * COL_TX, y0 = blockIdx.y * COL_TY;
    extern __shared__ float lds[];
    float* w = lds;
    float* tile = lds + k;
    const int rows = COL_TY + 2 * r;
    for (int i = threadIdx.x; i < k; i += blockDim.x) w[i] = weights[(long long)img * MP_PHOTO_MAX_BLUR + i];
    const float* src = tmp + (long long)img * H * W;
    const int tx = threadIdx.x % COL_TX, tg = threadIdx.x / COL_TX;
    const int x = x0 + tx;
    for (int i = tg; i < rows; i += 256 / COL_TX)
        tile[i * COL_TX + tx] = x < W ? src[(long long)reflect101(y0 - r + i, H) * W + x] : 0.f;
    __syncthreads();
    if (x >= W) return;
    for (int yy = tg; yy < COL_TY && y0 + yy < H; yy += 256 / COL_TX) {
        const float* c = tile + (yy + r) * COL_TX + tx;
        float s = w[r] * c[0];
        for (int j = 1; j <= r; ++j) s = s + w[r + j] * (c[j * COL_TX] + c[-j * COL_TX]);
        mask[((long long)img * H + y0 + yy) * W + x] = s;
    }
}

// ---------------------------------------------------------------------------------------------
// one primitive per image: elementwise in place, or motion blur into the other buffer
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void photo_step_kernel(float* out, float* alt, const mp_photometric_plan* plans, int step,
                                                         int H, int W, const double* normal, const double* uniform,
                                                         const float* mean, const float* mask)
{
    const int img = blockIdx.y;
    const mp_photometric_plan& plan = plans[img];
    if (step >= plan.n_ops) return;
    const long long HW = (long long)H * W;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= HW) return;
    int parity = 0;                                  // motion blurs before this step: which buffer is current
    for (int s = 0; s < step; ++s) parity ^= plan.op[s].kind == MP_PHOTO_MOTION_BLUR;
    float* cur = (parity ? alt : out) + img * HW;
    const mp_photometric_op& op = plan.op[step];
    switch (op.kind) {
    case MP_PHOTO_GAUSSIAN_NOISE:
    case MP_PHOTO_GAUSSIAN_ADD: {
        const double n = plan.noise_device ? op.value * hash_normal(op.key, (unsigned long long)p)
                                           : normal[op.field * HW + p];
        const float v = (float)((double)cur[p] + n);
        cur[p] = op.kind == MP_PHOTO_GAUSSIAN_NOISE ? clip01(v) : v;
        break;
    }
    case MP_PHOTO_SPECKLE: {
        const double u = plan.noise_device ? hash_uniform(op.key, (unsigned long long)p) : uniform[op.field * HW + p];
        float v = cur[p];
        if (u < op.value) v = 0.f;
        if (u > 1.0 - op.value) v = 1.f;
        cur[p] = v;
        break;
    }
    case MP_PHOTO_BRIGHTNESS:
        cur[p] = clip01(cur[p] + (float)op.value);
        break;
    case MP_PHOTO_CONTRAST: {
        const float m = mean[img];
        cur[p] = clip01((cur[p] - m) * (float)op.value + m);
        break;
    }
    case MP_PHOTO_SHADE:
        cur[p] = clip01(cur[p] * (1.f - (float)op.value * mask[img * HW + p]));
        break;
    case MP_PHOTO_MOTION_BLUR: {
        float* dst = (parity ? out : alt) + img * HW;
        const int y = (int)(p / W), x = (int)(p % W), c = (op.ksize - 1) / 2;
        float s = 0.f;
        for (int t = 0; t < op.ksize; ++t) {
            const int d = t - c;
            const int dy = op.mode == 0 ? 0 : d;
            const int dx = op.mode == 1 ? 0 : op.mode == 3 ? -d : d;
            s = s + op.taps[t] * cur[(long long)reflect101(y + dy, H) * W + reflect101(x + dx, W)];
        }
        dst[p] = s;
        break;
    }
    default:
        break;
    }
}

__global__ __launch_bounds__(256) void photo_copy_back_kernel(float* out, const float* alt, const mp_photometric_plan* plans,
                                                              long long HW)
{
    const int img = blockIdx.y;
    int parity = 0;
    for (int s = 0; s < plans[img].n_ops; ++s) parity ^= plans[img].op[s].kind == MP_PHOTO_MOTION_BLUR;
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (parity && p < HW) out[img * HW + p] = alt[img * HW + p];
}

__global__ __launch_bounds__(256) void photo_cur_ptrs_kernel(float* out, float* alt, const mp_photometric_plan* plans, int step,
                                                             long long HW, int n, const float** cur)
{
    const int img = blockIdx.x * blockDim.x + threadIdx.x;
    if (img >= n) return;
    int parity = 0;
    for (int s = 0; s < step && s < plans[img].n_ops; ++s) parity ^= plans[img].op[s].kind == MP_PHOTO_MOTION_BLUR;
    cur[img] = (parity ? alt : out) + img * HW;
}

struct PhotoWorkspace {
    mp_photometric_plan* plans;   // [n]
    int* ellipses;                // [n_ellipses][5]
    const float** cur;            // [n] current buffer of each image (mean kernel)
    float* mean;                  // [n]
    float* weights;               // [n][MP_PHOTO_MAX_BLUR]
    float* mask;                  // [n][H][W]  shade mask, blurred in place by the column pass
    float* tmp;                   // [n][H][W]  row-filtered mask
    float* alt;                   // [n][H][W]  motion-blur ping-pong buffer
    size_t bytes;
};

PhotoWorkspace photo_workspace(void* base, int n, int H, int W, int n_ellipses)
{
    const size_t px = (size_t)n * H * W;
    Carver c(base);
    PhotoWorkspace w;
    w.plans = c.take<mp_photometric_plan>(n);
    w.ellipses = c.take<int>(5 * (size_t)(n_ellipses > 0 ? n_ellipses : 1));
    w.cur = c.take<const float*>(n);
    w.mean = c.take<float>(n);
    w.weights = c.take<float>((size_t)MP_PHOTO_MAX_BLUR * n);
    w.mask = c.take<float>(px);
    w.tmp = c.take<float>(px);
    w.alt = c.take<float>(px);
    w.bytes = c.bytes();
    return w;
}

bool any_kind(const mp_photometric_plan* plans, int n, int step, int kind)
{
    for (int i = 0; i < n; ++i)
        if (step < plans[i].n_ops && plans[i].op[step].kind == kind) return true;
    return false;
}

int max_ellipses(const mp_photometric_plan* plans, int n, int step)
{
    int m = 0;
    for (int i = 0; i < n; ++i)
        if (step < plans[i].n_ops && plans[i].op[step].kind == MP_PHOTO_SHADE) m = max(m, plans[i].op[step].ellipse_count);
    return m;
}

int max_blur(const mp_photometric_plan* plans, int n, int step)
{
    int m = 1;
    for (int i = 0; i < n; ++i)
        if (step < plans[i].n_ops && plans[i].op[step].kind == MP_PHOTO_SHADE) m = max(m, plans[i].op[step].ksize);
    return m;
}

// GaussianBlur of n frames in place (through tmp): the shade masks of `step`, or plain frames with ksizes[img] (device)
void launch_blur(const mp_photometric_plan* plans, int step, const int* ksizes, int k, float* weights, float* img, float* tmp,
                 int n, int H, int W, hipStream_t s)
{
    const int r = k / 2;
    hipLaunchKernelGGL(blur_weights_kernel, dim3(n), dim3(64), 0, s, plans, step, ksizes, weights);
    hipLaunchKernelGGL(blur_rows_kernel, dim3(H, n), dim3(256), sizeof(float) * (size_t)(k + W + 2 * r), s, plans, step, ksizes,
                       weights, img, H, W, tmp);
    hipLaunchKernelGGL(blur_cols_kernel, dim3((W + COL_TX - 1) / COL_TX, (H + COL_TY - 1) / COL_TY, n), dim3(256),
                       sizeof(float) * (size_t)(k + (COL_TY + 2 * r) * COL_TX), s, plans, step, ksizes, weights, tmp, H, W, img);
}

// the (blurred) shade masks of step `step` into w.mask
void run_shade(const PhotoWorkspace& w, const mp_photometric_plan* host_plans, int n, int H, int W, int step, bool blurred,
               hipStream_t s)
{
    (void)hipMemsetAsync(w.mask, 0, sizeof(float) * (size_t)n * H * W, s);
    const int ne = max_ellipses(host_plans, n, step);
    if (ne > 0)
        hipLaunchKernelGGL(shade_ellipse_kernel, dim3(ne, n), dim3(64), sizeof(int) * 2 * (size_t)H, s, w.plans, w.ellipses,
                           step, H, W, w.mask);
    if (!blurred) return;
    launch_blur(w.plans, step, nullptr, max_blur(host_plans, n, step), w.weights, w.mask, w.tmp, n, H, W, s);
}

void upload(const PhotoWorkspace& w, const mp_photometric_plan* plans, int n, const int* ellipses, int n_ellipses,
            hipStream_t s)
{
    (void)hipMemcpyAsync(w.plans, plans, sizeof(mp_photometric_plan) * n, hipMemcpyHostToDevice, s);
    if (n_ellipses > 0)
        (void)hipMemcpyAsync(w.ellipses, ellipses, sizeof(int) * 5 * (size_t)n_ellipses, hipMemcpyHostToDevice, s);
    // the caller's host arrays may be gone once the entry point returns: wait for the copies to have read them
    (void)hipStreamSynchronize(s);
}

}  // namespace

size_t gaussian_blur_lds_bytes(int k, int W)
{
    const int r = k / 2;
    return max(sizeof(float) * (size_t)(k + W + 2 * r), sizeof(float) * (size_t)(k + (COL_TY + 2 * r) * COL_TX));
}

void launch_gaussian_blur_frames(float* img, float* tmp, float* weights, const int* ksizes, int kmax, int n, int H, int W,
                                 hipStream_t s)
{
    launch_blur(nullptr, 0, ksizes, kmax, weights, img, tmp, n, H, W, s);
}

size_t photometric_workspace_bytes(int n, int H, int W, int n_ellipses)
{
    return photo_workspace(nullptr, n, H, W, n_ellipses).bytes;
}

// the largest LDS request of a launch of these plans (the caller checks it against the device limit): the dynamic part of
// the blur kernels, dynamic plus static of shade_ellipse_kernel (its four vertex arrays and three ints)
size_t photometric_lds_bytes(const mp_photometric_plan* plans, int n, int H, int W)
{
    size_t b = 0;
    for (int s = 0; s < MP_PHOTO_MAX_OPS; ++s) {
        if (!any_kind(plans, n, s, MP_PHOTO_SHADE)) continue;
        if (max_ellipses(plans, n, s) > 0) b = max(b, sizeof(int) * 2 * (size_t)H + SHADE_STATIC_LDS);
        const int k = max_blur(plans, n, s), r = k / 2;
        b = max(b, sizeof(float) * (size_t)(k + W + 2 * r));
        b = max(b, sizeof(float) * (size_t)(k + (COL_TY + 2 * r) * COL_TX));
    }
    return b;
}

void launch_photometric(const float* in, float* out, int n, int H, int W, const mp_photometric_plan* plans,
                        const int* ellipses, int n_ellipses, const double* normal, const double* uniform, void* workspace,
                        hipStream_t s)
{
    const PhotoWorkspace w = photo_workspace(workspace, n, H, W, n_ellipses);
    const long long HW = (long long)H * W;
    upload(w, plans, n, ellipses, n_ellipses, s);
    if (in != out) (void)hipMemcpyAsync(out, in, sizeof(float) * (size_t)n * HW, hipMemcpyDeviceToDevice, s);
    int steps = 0;
    for (int i = 0; i < n; ++i) steps = max(steps, plans[i].n_ops);
    const dim3 grid((unsigned)((HW + 255) / 256), n);
    for (int step = 0; step < steps; ++step) {
        if (any_kind(plans, n, step, MP_PHOTO_CONTRAST)) {
            hipLaunchKernelGGL(photo_cur_ptrs_kernel, dim3((n + 255) / 256), dim3(256), 0, s, out, w.alt, w.plans, step, HW,
                               n, w.cur);
            hipLaunchKernelGGL(photo_mean_kernel, dim3(n), dim3(256), 0, s, w.cur, w.plans, step, HW, w.mean);
        }
        if (any_kind(plans, n, step, MP_PHOTO_SHADE)) run_shade(w, plans, n, H, W, step, true, s);
        hipLaunchKernelGGL(photo_step_kernel, grid, dim3(256), 0, s, out, w.alt, w.plans, step, H, W, normal, uniform, w.mean,
                           w.mask);
    }
    hipLaunchKernelGGL(photo_copy_back_kernel, grid, dim3(256), 0, s, out, w.alt, w.plans, HW);
}

void launch_photometric_shade_mask(int n, int H, int W, const mp_photometric_plan* plans, const int* ellipses,
                                   int n_ellipses, int op_index, int blurred, float* out, void* workspace, hipStream_t s)
{
    const PhotoWorkspace w = photo_workspace(workspace, n, H, W, n_ellipses);
    upload(w, plans, n, ellipses, n_ellipses, s);
    run_shade(w, plans, n, H, W, op_index, blurred != 0, s);
    (void)hipMemcpyAsync(out, w.mask, sizeof(float) * (size_t)n * H * W, hipMemcpyDeviceToDevice, s);
}
