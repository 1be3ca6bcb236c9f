// C ABI of the pooled ECC refinement (ecc_pooled.hip): mask growth, the static mask, flags in the packed plane,
// the raw per-pair sums at given group transforms, and the refinement with one transform per group.  The caller owns every
// buffer.  The host-side lists of an entry point (group of every pair, active flags, mask of every group) are copied into the
// workspace on the stream, which is synchronised once behind those copies so that the caller may free them on return.
// mp_ecc_pooled_step never synchronises.
#include <vector>

#include "host.h"

using namespace mp_host;

namespace {

size_t up(size_t v) { return (v + 255) & ~(size_t)255; }

struct PooledLayout { size_t group, active, offsets, list, tmask, groups, recs, quant, partial, total; };

PooledLayout pooled_layout(long long P, long long G, long long H, long long W)
{
    PooledLayout l{};
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += up(bytes); return o; };
    l.group = take((size_t)P * sizeof(int));
    l.active = take((size_t)P * sizeof(int));
    l.offsets = take((size_t)(G + 1) * sizeof(int));
    l.list = take((size_t)P * sizeof(int));
    l.tmask = take((size_t)G * sizeof(int));
    l.groups = take((size_t)G * sizeof(EccGroup));
    l.recs = take((size_t)P * sizeof(EccPairRec));
    l.quant = take((size_t)P * MP_ECC_POOLED_MAX_Q * sizeof(double));
    l.partial = take((size_t)P * ecc_chunks((int)H, (int)W) * MP_ECC_MAX_SUMS * sizeof(double));
    l.total = at;
    return l;
}

bool frame_ok(int H, int W) { return H >= 8 && W >= 8 && H <= 4096 && W <= 4096; }

// the checks mp_ecc_pooled_sums and mp_ecc_pooled_begin share; copies the lists into the workspace
int pooled_stage(mp_handle* h, const std::string& fn, const float* packed, int Ho, int Wo, const float* thermal, int H, int W,
                 int P, const int* group, const int* active, int G, const double* transforms, const unsigned char* masks,
                 int n_masks, const int* mask_of_group, int model, void* workspace, long long bytes, hipStream_t s,
                 PooledLayout& lay)
{
    if (!packed || !thermal || !group || !transforms || !workspace) return fail(h, MP_EINVAL, fn + ": NULL tensor");
    if (!frame_ok(H, W) || !frame_ok(Ho, Wo)) return fail(h, MP_EINVAL, fn + ": frames must be 8 x 8 to 4096 x 4096");
    if (P < 1 || P > 65535) return fail(h, MP_EINVAL, fn + ": n_pairs must be in [1, 65535]");
    if (G < 1 || G > MP_ECC_MAX_PROBLEMS)
        return fail(h, MP_EINVAL, fn + ": n_groups must be in [1, " + std::to_string(MP_ECC_MAX_PROBLEMS) + "]");
    if (ecc_model_params(model) == 0)
        return fail(h, MP_EINVAL, fn + ": unknown model " + std::to_string(model) +
                                      " (MP_MODEL_HOMOGRAPHY, MP_MODEL_SIMILARITY, MP_MODEL_AFFINE or MP_MODEL_TRANSLATION)");
    if (n_masks < 0 || (n_masks > 0 && !masks) || (mask_of_group && n_masks == 0))
        return fail(h, MP_EINVAL, fn + ": thermal masks need their planes, a non-negative count and an index per group");
    std::vector<int> offsets((size_t)G + 1, 0), list((size_t)P), tmask((size_t)G, -1), act((size_t)P, 1);
    for (int p = 0; p < P; ++p) {
        if (group[p] < 0 || group[p] >= G) return fail(h, MP_EINVAL, fn + ": group index outside [0, n_groups)");
        offsets[(size_t)group[p] + 1] += 1;
        if (active) act[p] = active[p] != 0;
    }
    for (int g = 0; g < G; ++g) {
        if (offsets[(size_t)g + 1] == 0) return fail(h, MP_EINVAL, fn + ": group " + std::to_string(g) + " has no pair");
        offsets[(size_t)g + 1] += offsets[g];
        if (mask_of_group) {
            if (mask_of_group[g] < -1 || mask_of_group[g] >= n_masks)
                return fail(h, MP_EINVAL, fn + ": mask index outside [-1, n_masks)");
            tmask[g] = mask_of_group[g];
        }
    }
    {
        std::vector<int> at(offsets.begin(), offsets.end() - 1);
        for (int p = 0; p < P; ++p) list[at[group[p]]++] = p;                          // ascending pair index inside a group
    }
    if (((size_t)packed & 15) != 0) return fail(h, MP_EINVAL, fn + ": packed must be 16-byte aligned");
    lay = pooled_layout(P, G, H, W);
    if (bytes < (long long)lay.total)
        return fail(h, MP_EINVAL, fn + ": workspace of " + std::to_string(bytes) + " B, needs " + std::to_string(lay.total) +
                                      " B (mp_ecc_pooled_workspace_bytes)");
    MP_HIP(hipSetDevice(h->device));
    char* ws = static_cast<char*>(workspace);
    MP_HIP(hipMemcpyAsync(ws + lay.group, group, (size_t)P * sizeof(int), hipMemcpyHostToDevice, s));
    MP_HIP(hipMemcpyAsync(ws + lay.active, act.data(), (size_t)P * sizeof(int), hipMemcpyHostToDevice, s));
    MP_HIP(hipMemcpyAsync(ws + lay.offsets, offsets.data(), (size_t)(G + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    MP_HIP(hipMemcpyAsync(ws + lay.list, list.data(), (size_t)P * sizeof(int), hipMemcpyHostToDevice, s));
    MP_HIP(hipMemcpyAsync(ws + lay.tmask, tmask.data(), (size_t)G * sizeof(int), hipMemcpyHostToDevice, s));
    MP_HIP(hipStreamSynchronize(s));
    return MP_OK;
}

}  // namespace

extern "C" {

int mp_ecc_mask_grow(mp_handle* h, const unsigned char* mask, int n, int H, int W, int radius, unsigned char* tmp, unsigned char* out,
                     void* stream)
{
    if (!h) return MP_EINVAL;
    if (!mask || !tmp || !out) return fail(h, MP_EINVAL, "mp_ecc_mask_grow: NULL tensor");
    if (tmp == mask || tmp == out) return fail(h, MP_EINVAL, "mp_ecc_mask_grow: tmp must not alias mask or out");
    if (n < 1 || n > 65535) return fail(h, MP_EINVAL, "mp_ecc_mask_grow: n must be in [1, 65535]");
    if (!frame_ok(H, W)) return fail(h, MP_EINVAL, "mp_ecc_mask_grow: frames must be 8 x 8 to 4096 x 4096");
    if (radius < 0) return fail(h, MP_EINVAL, "mp_ecc_mask_grow: radius must not be negative");
    MP_HIP(hipSetDevice(h->device));
    launch_ecc_mask_grow(mask, n, H, W, radius, tmp, out, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_ecc_static_update(mp_handle* h, const float* frames, int n, int H, int W, int first, float* lo, float* hi, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!frames || !lo || !hi) return fail(h, MP_EINVAL, "mp_ecc_static_update: NULL tensor");
    if (n < 1 || n > 65535) return fail(h, MP_EINVAL, "mp_ecc_static_update: n must be in [1, 65535]");
    if (!frame_ok(H, W)) return fail(h, MP_EINVAL, "mp_ecc_static_update: frames must be 8 x 8 to 4096 x 4096");
    MP_HIP(hipSetDevice(h->device));
    launch_ecc_static_update(frames, n, H * W, first != 0, lo, hi, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_ecc_static_finish(mp_handle* h, const float* lo, const float* hi, int H, int W, unsigned char* mask, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!lo || !hi || !mask) return fail(h, MP_EINVAL, "mp_ecc_static_finish: NULL tensor");
    if (!frame_ok(H, W)) return fail(h, MP_EINVAL, "mp_ecc_static_finish: frames must be 8 x 8 to 4096 x 4096");
    MP_HIP(hipSetDevice(h->device));
    launch_ecc_static_finish(lo, hi, H * W, mask, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_ecc_flag_packed(mp_handle* h, float* packed, int n, int H, int W, const unsigned char* masks, int n_masks,
                       const int* mask_of_frame, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!packed || !masks || !mask_of_frame) return fail(h, MP_EINVAL, "mp_ecc_flag_packed: NULL tensor");
    if (((size_t)packed & 15) != 0) return fail(h, MP_EINVAL, "mp_ecc_flag_packed: packed must be 16-byte aligned");
    if (n < 1 || n > 65535) return fail(h, MP_EINVAL, "mp_ecc_flag_packed: n must be in [1, 65535]");
    if (!frame_ok(H, W)) return fail(h, MP_EINVAL, "mp_ecc_flag_packed: frames must be 8 x 8 to 4096 x 4096");
    if (n_masks < 1) return fail(h, MP_EINVAL, "mp_ecc_flag_packed: n_masks must be positive");
    for (int i = 0; i < n; ++i)
        if (mask_of_frame[i] < -1 || mask_of_frame[i] >= n_masks)
            return fail(h, MP_EINVAL, "mp_ecc_flag_packed: mask index outside [-1, n_masks)");
    MP_HIP(hipSetDevice(h->device));
    const size_t HW = (size_t)H * W;
    for (int i = 0; i < n;) {                                                       // one launch per run of frames under one mask
        int j = i + 1;
        while (j < n && mask_of_frame[j] == mask_of_frame[i]) ++j;
        if (mask_of_frame[i] >= 0)
            launch_ecc_flag_packed(packed + 4 * HW * i, j - i, (int)HW, masks + HW * mask_of_frame[i], static_cast<hipStream_t>(stream));
        i = j;
    }
    return launch_status(h);
}

int mp_ecc_pooled_workspace_bytes(int n_pairs, int n_groups, int H, int W, long long* bytes)
{
    if (!bytes || n_pairs < 1 || n_pairs > 65535 || n_groups < 1 || n_groups > MP_ECC_MAX_PROBLEMS || !frame_ok(H, W)) return MP_EINVAL;
    *bytes = (long long)pooled_layout(n_pairs, n_groups, H, W).total;
    return MP_OK;
}

int mp_ecc_pooled_sums(mp_handle* h, const float* packed, int Ho, int Wo, const float* thermal, int H, int W, int n_pairs,
                       const int* group, int n_groups, const double* transforms, const unsigned char* thermal_masks, int n_masks,
                       const int* mask_of_group, int model, double* sums, void* workspace, long long workspace_bytes, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!sums) return fail(h, MP_EINVAL, "mp_ecc_pooled_sums: NULL tensor");
    hipStream_t s = static_cast<hipStream_t>(stream);
    PooledLayout lay;
    const int rc = pooled_stage(h, "mp_ecc_pooled_sums", packed, Ho, Wo, thermal, H, W, n_pairs, group, nullptr, n_groups, transforms,
                                thermal_masks, n_masks, mask_of_group, model, workspace, workspace_bytes, s, lay);
    if (rc != MP_OK) return rc;
    char* ws = static_cast<char*>(workspace);
    const int K = ecc_model_params(model);
    double* partial = reinterpret_cast<double*>(ws + lay.partial);
    launch_ecc_pooled_sums(K, packed, Ho, Wo, thermal, H, W, thermal_masks, reinterpret_cast<const int*>(ws + lay.tmask),
                           reinterpret_cast<const int*>(ws + lay.group), reinterpret_cast<const int*>(ws + lay.active), transforms,
                           nullptr, n_pairs, partial, s);
    launch_ecc_reduce(K, partial, n_pairs, ecc_chunks(H, W), sums, s);
    return launch_status(h);
}

int mp_ecc_pooled_begin(mp_handle* h, const float* packed, int Ho, int Wo, const float* thermal, int H, int W, int n_pairs,
                        const int* group, const int* active, int n_groups, const double* init_transforms,
                        const unsigned char* thermal_masks, int n_masks, const int* mask_of_group, int model, double eps, int maxiter,
                        double min_valid, void* workspace, long long workspace_bytes, void* stream)
{
    if (!h) return MP_EINVAL;
    h->ecc_pooled = EccPooledRefine{};
    if (!(eps >= 0.0) || maxiter < 1 || !(min_valid >= 0.0 && min_valid <= 1.0))
        return fail(h, MP_EINVAL, "mp_ecc_pooled_begin: eps must be non-negative, maxiter positive, min_valid in [0, 1]");
    hipStream_t s = static_cast<hipStream_t>(stream);
    PooledLayout lay;
    const int rc = pooled_stage(h, "mp_ecc_pooled_begin", packed, Ho, Wo, thermal, H, W, n_pairs, group, active, n_groups,
                                init_transforms, thermal_masks, n_masks, mask_of_group, model, workspace, workspace_bytes, s, lay);
    if (rc != MP_OK) return rc;
    char* ws = static_cast<char*>(workspace);
    EccPooledRefine r;
    r.workspace = workspace;
    r.packed = packed; r.thermal = thermal; r.tmasks = thermal_masks;
    r.Ho = Ho; r.Wo = Wo; r.H = H; r.W = W; r.P = n_pairs; r.G = n_groups; r.K = ecc_model_params(model);
    r.opt = EccOptions{eps, min_valid, maxiter, 0};
    r.group = reinterpret_cast<const int*>(ws + lay.group);
    r.active = reinterpret_cast<const int*>(ws + lay.active);
    r.offsets = reinterpret_cast<const int*>(ws + lay.offsets);
    r.list = reinterpret_cast<const int*>(ws + lay.list);
    r.tmask = reinterpret_cast<const int*>(ws + lay.tmask);
    r.groups = reinterpret_cast<EccGroup*>(ws + lay.groups);
    r.recs = reinterpret_cast<EccPairRec*>(ws + lay.recs);
    r.quant = reinterpret_cast<double*>(ws + lay.quant);
    r.partial = reinterpret_cast<double*>(ws + lay.partial);
    launch_ecc_pooled_begin(init_transforms, thermal_masks, r.tmask, H * W, n_groups, n_pairs, r.groups, r.recs, s);
    h->ecc_pooled = r;
    return launch_status(h);
}

int mp_ecc_pooled_step(mp_handle* h, void* workspace, int n_iters, int* live, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!workspace || !live) return fail(h, MP_EINVAL, "mp_ecc_pooled_step: NULL tensor");
    if (!h->ecc_pooled.workspace || h->ecc_pooled.workspace != workspace)
        return fail(h, MP_ESTATE, "mp_ecc_pooled_step: no pooled refinement was begun in this workspace");
    if (n_iters < 1 || n_iters > 100000) return fail(h, MP_EINVAL, "mp_ecc_pooled_step: n_iters must be in [1, 100000]");
    MP_HIP(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const EccPooledRefine& r = h->ecc_pooled;
    const int chunks = ecc_chunks(r.H, r.W);
    for (int i = 0; i < n_iters; ++i) {
        launch_ecc_pooled_sums(r.K, r.packed, r.Ho, r.Wo, r.thermal, r.H, r.W, r.tmasks, r.tmask, r.group, r.active, nullptr, r.groups,
                               r.P, r.partial, s);
        launch_ecc_pooled_pair(r.K, r.partial, r.P, chunks, r.group, r.active, r.opt, r.groups, r.recs, r.quant, s);
        launch_ecc_pooled_solve(r.K, r.offsets, r.list, r.recs, r.quant, r.G, r.opt, r.groups, s);
    }
    launch_ecc_pooled_live(r.groups, r.G, live, s);
    return launch_status(h);
}

int mp_ecc_pooled_result(mp_handle* h, void* workspace, double* transforms, double* rho, int* iterations, int* status, int* converged,
                         int* n_included, double* rho_pair, double* n_pair, int* included, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!workspace || !transforms || !rho || !iterations || !status || !converged || !n_included || !rho_pair || !n_pair || !included)
        return fail(h, MP_EINVAL, "mp_ecc_pooled_result: NULL tensor");
    if (!h->ecc_pooled.workspace || h->ecc_pooled.workspace != workspace)
        return fail(h, MP_ESTATE, "mp_ecc_pooled_result: no pooled refinement was begun in this workspace");
    MP_HIP(hipSetDevice(h->device));
    const EccPooledRefine& r = h->ecc_pooled;
    launch_ecc_pooled_result(r.groups, r.G, r.recs, r.P, transforms, rho, iterations, status, converged, n_included, rho_pair, n_pair,
                             included, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

}  // extern "C"
