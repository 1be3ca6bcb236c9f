// C ABI of the pooled ECC refinement (ecc_pooled.hip): mask growth, the static mask, flags in the packed plane,
// the raw per-pair sums at given group transforms, and the refinement with one transform per group.  The caller owns every
// buffer.  The host-side lists of an entry point (group of every pair, active flags, mask of every group) are copied into the
// workspace on the stream, which is synchronised once behind those copies so that the caller may free them on return.
// mp_ecc_pooled_step never synchronises.
#include <vector>

#include "host.h"

using namespace mp_host;

namespace {

EccPooledWorkspace pooled_workspace(void* base, size_t P, size_t G, int H, int W)
{
    Carver c(base);
    EccPooledWorkspace w{};
    w.group = c.take<int>(P);
    w.active = c.take<int>(P);
    w.offsets = c.take<int>(G + 1);
    w.list = c.take<int>(P);
    w.tmask = c.take<int>(G);
    w.groups = c.take<EccGroup>(G);
    w.recs = c.take<EccPairRec>(P);
    w.quant = c.take<double>(P * MP_ECC_POOLED_MAX_Q);
    w.partial = c.take<double>(P * ecc_chunks(H, W) * MP_ECC_MAX_SUMS);
    w.bytes = c.bytes();
    return w;
}

// the checks mp_ecc_pooled_sums and mp_ecc_pooled_begin share; copies the lists into the workspace
int pooled_stage(mp_handle* h, const std::string& fn, const float* packed, int Ho, int Wo, const float* thermal, int H, int W,
                 int P, const int* group, const int* active, int G, const double* transforms, const unsigned char* masks,
                 int n_masks, const int* mask_of_group, int model, void* workspace, long long bytes, hipStream_t s,
                 EccPooledWorkspace& w)
{
    if (!packed || !thermal || !group || !transforms || !workspace) return fail(h, MP_EINVAL, fn + ": NULL tensor");
    if (!sides_ok(H, W, 8, 4096) || !sides_ok(Ho, Wo, 8, 4096)) return fail(h, MP_EINVAL, fn + ": frames must be 8 x 8 to 4096 x 4096");
    if (!count_ok(P)) return fail(h, MP_EINVAL, fn + ": n_pairs must be in [1, 65535]");
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
    w = pooled_workspace(workspace, P, G, H, W);
    const int rc = need_workspace(h, fn, bytes, w.bytes, "mp_ecc_pooled_workspace_bytes");
    if (rc != MP_OK) return rc;
    MP_HIP(hipSetDevice(h->device));
    MP_HIP(hipMemcpyAsync(w.group, group, (size_t)P * sizeof(int), hipMemcpyHostToDevice, s));
    MP_HIP(hipMemcpyAsync(w.active, act.data(), (size_t)P * sizeof(int), hipMemcpyHostToDevice, s));
    MP_HIP(hipMemcpyAsync(w.offsets, offsets.data(), (size_t)(G + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    MP_HIP(hipMemcpyAsync(w.list, list.data(), (size_t)P * sizeof(int), hipMemcpyHostToDevice, s));
    MP_HIP(hipMemcpyAsync(w.tmask, tmask.data(), (size_t)G * sizeof(int), hipMemcpyHostToDevice, s));
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
    if (!count_ok(n)) return fail(h, MP_EINVAL, "mp_ecc_mask_grow: n must be in [1, 65535]");
    if (!sides_ok(H, W, 8, 4096)) return fail(h, MP_EINVAL, "mp_ecc_mask_grow: frames must be 8 x 8 to 4096 x 4096");
    if (radius < 0) return fail(h, MP_EINVAL, "mp_ecc_mask_grow: radius must not be negative");
    MP_HIP(hipSetDevice(h->device));
    launch_ecc_mask_grow(mask, n, H, W, radius, tmp, out, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_ecc_static_update(mp_handle* h, const float* frames, int n, int H, int W, int first, float* lo, float* hi, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!frames || !lo || !hi) return fail(h, MP_EINVAL, "mp_ecc_static_update: NULL tensor");
    if (!count_ok(n)) return fail(h, MP_EINVAL, "mp_ecc_static_update: n must be in [1, 65535]");
    if (!sides_ok(H, W, 8, 4096)) return fail(h, MP_EINVAL, "mp_ecc_static_update: frames must be 8 x 8 to 4096 x 4096");
    MP_HIP(hipSetDevice(h->device));
    launch_ecc_static_update(frames, n, H * W, first != 0, lo, hi, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_ecc_static_finish(mp_handle* h, const float* lo, const float* hi, int H, int W, unsigned char* mask, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!lo || !hi || !mask) return fail(h, MP_EINVAL, "mp_ecc_static_finish: NULL tensor");
    if (!sides_ok(H, W, 8, 4096)) return fail(h, MP_EINVAL, "mp_ecc_static_finish: frames must be 8 x 8 to 4096 x 4096");
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
    if (!count_ok(n)) return fail(h, MP_EINVAL, "mp_ecc_flag_packed: n must be in [1, 65535]");
    if (!sides_ok(H, W, 8, 4096)) return fail(h, MP_EINVAL, "mp_ecc_flag_packed: frames must be 8 x 8 to 4096 x 4096");
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
    if (!bytes || !count_ok(n_pairs) || n_groups < 1 || n_groups > MP_ECC_MAX_PROBLEMS || !sides_ok(H, W, 8, 4096)) return MP_EINVAL;
    *bytes = (long long)pooled_workspace(nullptr, n_pairs, n_groups, H, W).bytes;
    return MP_OK;
}

int mp_ecc_pooled_sums(mp_handle* h, const float* packed, int Ho, int Wo, const float* thermal, int H, int W, int n_pairs,
                       const int* group, int n_groups, const double* transforms, const unsigned char* thermal_masks, int n_masks,
                       const int* mask_of_group, int model, double* sums, void* workspace, long long workspace_bytes, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!sums) return fail(h, MP_EINVAL, "mp_ecc_pooled_sums: NULL tensor");
    hipStream_t s = static_cast<hipStream_t>(stream);
    EccPooledWorkspace w;
    const int rc = pooled_stage(h, "mp_ecc_pooled_sums", packed, Ho, Wo, thermal, H, W, n_pairs, group, nullptr, n_groups, transforms,
                                thermal_masks, n_masks, mask_of_group, model, workspace, workspace_bytes, s, w);
    if (rc != MP_OK) return rc;
    const int K = ecc_model_params(model);
    launch_ecc_pooled_sums(K, packed, Ho, Wo, thermal, H, W, thermal_masks, w.tmask, w.group, w.active, transforms, nullptr, n_pairs,
                           w.partial, s);
    launch_ecc_reduce(K, w.partial, n_pairs, ecc_chunks(H, W), sums, s);
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
    EccPooledRefine r;
    const int rc = pooled_stage(h, "mp_ecc_pooled_begin", packed, Ho, Wo, thermal, H, W, n_pairs, group, active, n_groups,
                                init_transforms, thermal_masks, n_masks, mask_of_group, model, workspace, workspace_bytes, s, r.w);
    if (rc != MP_OK) return rc;
    r.workspace = workspace;
    r.packed = packed; r.thermal = thermal; r.tmasks = thermal_masks;
    r.Ho = Ho; r.Wo = Wo; r.H = H; r.W = W; r.P = n_pairs; r.G = n_groups; r.K = ecc_model_params(model);
    r.opt = EccOptions{eps, min_valid, maxiter, 0};
    launch_ecc_pooled_begin(init_transforms, thermal_masks, r.w.tmask, H * W, n_groups, n_pairs, r.w.groups, r.w.recs, s);
    h->ecc_pooled = r;
    return launch_status(h);
}

int mp_ecc_pooled_step(mp_handle* h, void* workspace, int n_iters, int* live, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!workspace || !live) return fail(h, MP_EINVAL, "mp_ecc_pooled_step: NULL tensor");
    if (const int rc = begun_in(h, "mp_ecc_pooled_step", h->ecc_pooled.workspace, workspace)) return rc;
    if (n_iters < 1 || n_iters > 100000) return fail(h, MP_EINVAL, "mp_ecc_pooled_step: n_iters must be in [1, 100000]");
    MP_HIP(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const EccPooledRefine& r = h->ecc_pooled;
    const EccPooledWorkspace& w = r.w;
    const int chunks = ecc_chunks(r.H, r.W);
    for (int i = 0; i < n_iters; ++i) {
        launch_ecc_pooled_sums(r.K, r.packed, r.Ho, r.Wo, r.thermal, r.H, r.W, r.tmasks, w.tmask, w.group, w.active, nullptr, w.groups,
                               r.P, w.partial, s);
        launch_ecc_pooled_pair(r.K, w.partial, r.P, chunks, w.group, w.active, r.opt, w.groups, w.recs, w.quant, s);
        launch_ecc_pooled_solve(r.K, w.offsets, w.list, w.recs, w.quant, r.G, r.opt, w.groups, s);
    }
    launch_ecc_pooled_live(w.groups, r.G, live, s);
    return launch_status(h);
}

int mp_ecc_pooled_result(mp_handle* h, void* workspace, double* transforms, double* rho, int* iterations, int* status, int* converged,
                         int* n_included, double* rho_pair, double* n_pair, int* included, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!workspace || !transforms || !rho || !iterations || !status || !converged || !n_included || !rho_pair || !n_pair || !included)
        return fail(h, MP_EINVAL, "mp_ecc_pooled_result: NULL tensor");
    if (const int rc = begun_in(h, "mp_ecc_pooled_result", h->ecc_pooled.workspace, workspace)) return rc;
    MP_HIP(hipSetDevice(h->device));
    const EccPooledRefine& r = h->ecc_pooled;
    launch_ecc_pooled_result(r.w.groups, r.G, r.w.recs, r.P, transforms, rho, iterations, status, converged, n_included, rho_pair, n_pair,
                             included, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

}  // extern "C"
