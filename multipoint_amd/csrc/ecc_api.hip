// C ABI of the ECC direct alignment (ecc.hip): the feature frames, the raw sums of given transforms, and the
// batched Gauss-Newton refinement.  The caller owns every buffer.  The host-side pair list of an entry point is copied into the
// workspace on the stream, which is synchronised once behind that copy so that the caller may free it on return.  mp_ecc_step
// never synchronises.
#include "host.h"

using namespace mp_host;

namespace {

EccWorkspace ecc_workspace(void* base, size_t P, int H, int W)
{
    Carver c(base);
    EccWorkspace w{};
    w.pair = c.take<int>(P);
    w.state = c.take<EccState>(P);
    w.partial = c.take<double>(P * ecc_chunks(H, W) * MP_ECC_MAX_SUMS);
    w.bytes = c.bytes();
    return w;
}

// the checks mp_ecc_sums and mp_ecc_begin share; copies the pair list into the workspace
int ecc_stage(mp_handle* h, const std::string& fn, const float* packed, int Ho, int Wo, const float* thermal, int H, int W,
              int n_pairs, const int* pair, const double* transforms, int P, int model, void* workspace, long long bytes,
              hipStream_t s, EccWorkspace& w)
{
    if (!packed || !thermal || !pair || !transforms || !workspace) return fail(h, MP_EINVAL, fn + ": NULL tensor");
    if (!sides_ok(H, W, 8, 4096) || !sides_ok(Ho, Wo, 8, 4096)) return fail(h, MP_EINVAL, fn + ": frames must be 8 x 8 to 4096 x 4096");
    if (!count_ok(n_pairs)) return fail(h, MP_EINVAL, fn + ": n_pairs must be in [1, 65535]");
    if (P < 1 || P > MP_ECC_MAX_PROBLEMS)
        return fail(h, MP_EINVAL, fn + ": n_problems must be in [1, " + std::to_string(MP_ECC_MAX_PROBLEMS) + "]");
    if (ecc_model_params(model) == 0)
        return fail(h, MP_EINVAL, fn + ": unknown model " + std::to_string(model) +
                                      " (MP_MODEL_HOMOGRAPHY, MP_MODEL_SIMILARITY, MP_MODEL_AFFINE or MP_MODEL_TRANSLATION)");
    for (int q = 0; q < P; ++q)
        if (pair[q] < 0 || pair[q] >= n_pairs) return fail(h, MP_EINVAL, fn + ": pair index outside [0, n_pairs)");
    if (((size_t)packed & 15) != 0) return fail(h, MP_EINVAL, fn + ": packed must be 16-byte aligned");
    w = ecc_workspace(workspace, P, H, W);
    const int rc = need_workspace(h, fn, bytes, w.bytes, "mp_ecc_workspace_bytes");
    if (rc != MP_OK) return rc;
    MP_HIP(hipSetDevice(h->device));
    MP_HIP(hipMemcpyAsync(w.pair, pair, (size_t)P * sizeof(int), hipMemcpyHostToDevice, s));
    MP_HIP(hipStreamSynchronize(s));
    return MP_OK;
}

}  // namespace

extern "C" {

int mp_ecc_workspace_bytes(int n_problems, int H, int W, long long* bytes)
{
    if (!bytes || n_problems < 1 || n_problems > MP_ECC_MAX_PROBLEMS || !sides_ok(H, W, 8, 4096)) return MP_EINVAL;
    *bytes = (long long)ecc_workspace(nullptr, n_problems, H, W).bytes;
    return MP_OK;
}

int mp_ecc_prepare(mp_handle* h, const float* blurred, int n, int H, int W, int feature, float* feat, float* packed, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!blurred || !feat) return fail(h, MP_EINVAL, "mp_ecc_prepare: NULL tensor");
    if (blurred == feat) return fail(h, MP_EINVAL, "mp_ecc_prepare: feat must not alias blurred");
    if (!count_ok(n)) return fail(h, MP_EINVAL, "mp_ecc_prepare: n must be in [1, 65535]");
    if (!sides_ok(H, W, 8, 4096)) return fail(h, MP_EINVAL, "mp_ecc_prepare: frames must be 8 x 8 to 4096 x 4096");
    if (feature != MP_ECC_GRADIENT && feature != MP_ECC_INTENSITY)
        return fail(h, MP_EINVAL, "mp_ecc_prepare: feature must be MP_ECC_GRADIENT or MP_ECC_INTENSITY");
    if (((size_t)packed & 15) != 0) return fail(h, MP_EINVAL, "mp_ecc_prepare: packed must be 16-byte aligned");
    MP_HIP(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    launch_ecc_feature(blurred, n, H, W, feature == MP_ECC_GRADIENT, feat, s);
    if (packed) launch_ecc_pack(feat, n, H, W, packed, s);
    return launch_status(h);
}

int mp_ecc_sums(mp_handle* h, const float* packed, int Ho, int Wo, const float* thermal, int H, int W, int n_pairs, const int* pair,
                const double* transforms, int n_problems, int model, double* sums, void* workspace, long long workspace_bytes,
                void* stream)
{
    if (!h) return MP_EINVAL;
    if (!sums) return fail(h, MP_EINVAL, "mp_ecc_sums: NULL tensor");
    hipStream_t s = static_cast<hipStream_t>(stream);
    EccWorkspace w;
    const int rc = ecc_stage(h, "mp_ecc_sums", packed, Ho, Wo, thermal, H, W, n_pairs, pair, transforms, n_problems, model,
                             workspace, workspace_bytes, s, w);
    if (rc != MP_OK) return rc;
    const int K = ecc_model_params(model);
    launch_ecc_sums(K, packed, Ho, Wo, thermal, H, W, w.pair, transforms, nullptr, n_problems, w.partial, s);
    launch_ecc_reduce(K, w.partial, n_problems, ecc_chunks(H, W), sums, s);
    return launch_status(h);
}

int mp_ecc_begin(mp_handle* h, const float* packed, int Ho, int Wo, const float* thermal, int H, int W, int n_pairs,
                 const int* pair, const double* init_transforms, int n_problems, int model, double eps, int maxiter,
                 double min_valid, void* workspace, long long workspace_bytes, void* stream)
{
    if (!h) return MP_EINVAL;
    h->ecc = EccRefine{};
    if (!(eps >= 0.0) || maxiter < 1 || !(min_valid >= 0.0 && min_valid <= 1.0))
        return fail(h, MP_EINVAL, "mp_ecc_begin: eps must be non-negative, maxiter positive, min_valid in [0, 1]");
    hipStream_t s = static_cast<hipStream_t>(stream);
    EccRefine r;
    const int rc = ecc_stage(h, "mp_ecc_begin", packed, Ho, Wo, thermal, H, W, n_pairs, pair, init_transforms, n_problems, model,
                             workspace, workspace_bytes, s, r.w);
    if (rc != MP_OK) return rc;
    r.workspace = workspace;
    r.packed = packed; r.thermal = thermal;
    r.Ho = Ho; r.Wo = Wo; r.H = H; r.W = W; r.P = n_problems; r.K = ecc_model_params(model);
    r.opt = EccOptions{eps, min_valid, maxiter, 0};
    launch_ecc_begin(r.w.pair, init_transforms, n_problems, r.w.state, s);
    h->ecc = r;
    return launch_status(h);
}

int mp_ecc_step(mp_handle* h, void* workspace, int n_iters, int* live, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!workspace || !live) return fail(h, MP_EINVAL, "mp_ecc_step: NULL tensor");
    if (const int rc = begun_in(h, "mp_ecc_step", h->ecc.workspace, workspace)) return rc;
    if (n_iters < 1 || n_iters > 100000) return fail(h, MP_EINVAL, "mp_ecc_step: n_iters must be in [1, 100000]");
    MP_HIP(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const EccRefine& r = h->ecc;
    for (int i = 0; i < n_iters; ++i) {
        launch_ecc_sums(r.K, r.packed, r.Ho, r.Wo, r.thermal, r.H, r.W, nullptr, nullptr, r.w.state, r.P, r.w.partial, s);
        launch_ecc_solve(r.K, r.w.partial, r.P, ecc_chunks(r.H, r.W), r.H * r.W, r.opt, r.w.state, s);
    }
    launch_ecc_live(r.w.state, r.P, live, s);
    return launch_status(h);
}

int mp_ecc_result(mp_handle* h, void* workspace, double* transforms, double* rho, int* iterations, int* status, int* converged,
                  void* stream)
{
    if (!h) return MP_EINVAL;
    if (!workspace || !transforms || !rho || !iterations || !status || !converged)
        return fail(h, MP_EINVAL, "mp_ecc_result: NULL tensor");
    if (const int rc = begun_in(h, "mp_ecc_result", h->ecc.workspace, workspace)) return rc;
    MP_HIP(hipSetDevice(h->device));
    launch_ecc_result(h->ecc.w.state, h->ecc.P, transforms, rho, iterations, status, converged, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

}  // extern "C"
