// C ABI of the mutual-information alignment (mutual_info.hip): joint histograms, the objective, and the batched
// Nelder-Mead refinement.  The caller owns every buffer; the host-side lists of an entry point (pair index and bin count
// per evaluation, the problems of a refinement) are copied into the workspace on the stream, which is synchronised once
// behind that copy so that the caller may free them on return.  mp_mi_refine_step never synchronises.
#include "host.h"

#include <map>
#include <utility>

using namespace mp_host;

static_assert(MI_SLOTS == MP_MI_SLOTS, "the kernels' slots per problem and the public header's must agree");
static_assert(MI_PARAMS_MAX == MP_MI_PARAMS_MAX && MI_PARAMS_MAX + 1 <= MI_SLOTS,
              "the largest simplex must fit a problem's evaluation slots");

namespace {

// the arrays of a call with E evaluations of B pairs, S thermal bin maps and histograms of at most max_bins bins per side
MiWorkspace mi_workspace(void* base, long long E, long long B, long long S, long long H, long long W, long long max_bins,
                         bool smoothing)
{
    const size_t hist = (size_t)(2 * max_bins * max_bins), P = (size_t)((E + MI_SLOTS - 1) / MI_SLOTS), px = (size_t)(H * W);
    Carver c(base);
    MiWorkspace w{};
    w.ev = c.take<MiEval>(E);
    w.slots = c.take<int2>(S);
    w.nact = c.take<int>(P);
    w.M = c.take<double>(E * 9);
    w.keys = c.take<unsigned>(E * 2);
    w.tkeys = c.take<unsigned>(B * 2);
    w.tmap = c.take<unsigned short>(S * px);
    w.warped = c.take<float>(E * px);
    w.counts = c.take<unsigned>(E * hist);
    w.smooth_a = c.take<double>(smoothing ? E * hist : 0);
    w.smooth_b = c.take<double>(smoothing ? E * hist : 0);
    w.part = c.take<double>(E * MI_PARTS);
    w.rowsum = c.take<double>(E * 256);
    w.colpart = c.take<double>((size_t)E * MI_PARTS * 512);
    w.values = c.take<double>(E);
    w.cand = c.take<double>(E * 9);
    w.candp = c.take<double>(E * MI_PARAMS_MAX);
    w.state = c.take<MiNmState>(P);
    w.opts = c.take<MiNmOptions>(P);
    w.tinit = c.take<double>(P * 9);
    w.live = c.take<int>(1);
    w.bytes = c.bytes();
    return w;
}

struct MiCall {
    MiWorkspace w{};
    MiLaunch L{};
    long long stride = 0;          // counters per evaluation inside the workspace: 2 max_bins^2
};

// Checks the arguments the three entry points share, writes the evaluation list and the thermal bin maps into the workspace and
// fills c.  `packed`: the counters of evaluation e follow those of e - 1 directly (the caller's array of mp_mi_joint_histogram);
// otherwise they lie 2 max_bins^2 apart in the workspace.
int mi_stage(mp_handle* h, const std::string& fn, const float* optical, int Ho, int Wo, const float* thermal, int H, int W, int B,
             const int* pair, const int* bins, int E, int G, bool packed, bool smoothing, void* workspace, long long bytes,
             hipStream_t s, MiCall& c)
{
    if (!optical || !thermal || !pair || !bins || !workspace) return fail(h, MP_EINVAL, fn + ": NULL tensor");
    if (B > MAX_GRID_Y) return fail(h, MP_EINVAL, fn + ": at most 65535 pairs per call");
    if (B <= 0 || E <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return fail(h, MP_EINVAL, fn + ": sizes must be positive");
    if (H > 32767 || W > 32767 || Ho > 32767 || Wo > 32767 || (long long)H * W > 0x3fffffffLL || (long long)Ho * Wo > 0x3fffffffLL)
        return fail(h, MP_EINVAL, fn + ": frames of at most 32767 x 32767 and 2^30 pixels");
    if (E > MAX_GRID_Y) return fail(h, MP_EINVAL, fn + ": at most 65535 evaluations per call (" + std::to_string(MI_SLOTS) + " per problem)");
    std::vector<MiEval> ev((size_t)E);
    std::vector<int2> slots;
    std::map<std::pair<int, int>, int> slot_of;
    int maxb = 1, lds_bins = 0;
    long long off = 0;
    for (int e = 0; e < E; ++e) {
        if (pair[e] < 0 || pair[e] >= B) return fail(h, MP_EINVAL, fn + ": pair index outside [0, n_pairs)");
        if (bins[e] < 1 || bins[e] > 256) return fail(h, MP_EINVAL, fn + ": bins must be in [1, 256]");
        if (bins[e] > maxb) maxb = bins[e];
        if (bins[e] <= 64 && bins[e] > lds_bins) lds_bins = bins[e];
        auto it = slot_of.find({pair[e], bins[e]});
        if (it == slot_of.end()) {
            it = slot_of.emplace(std::make_pair(pair[e], bins[e]), (int)slots.size()).first;
            slots.push_back(int2{pair[e], bins[e]});
        }
        ev[e] = MiEval{pair[e], bins[e], it->second, 0, off};
        off += 2LL * bins[e] * bins[e];
    }
    c.stride = 2LL * maxb * maxb;
    if (!packed) for (int e = 0; e < E; ++e) ev[e].off = e * c.stride;
    const MiWorkspace w = c.w = mi_workspace(workspace, E, B, (long long)slots.size(), H, W, maxb, smoothing);
    const int rc = need_workspace(h, fn, bytes, w.bytes, "mp_mi_workspace_bytes");
    if (rc != MP_OK) return rc;
    MP_HIP(hipSetDevice(h->device));
    MP_HIP(hipMemcpyAsync(w.ev, ev.data(), ev.size() * sizeof(MiEval), hipMemcpyHostToDevice, s));
    MP_HIP(hipMemcpyAsync(w.slots, slots.data(), slots.size() * sizeof(int2), hipMemcpyHostToDevice, s));
    launch_mi_thermal(thermal, B, H * W, w.slots, (int)slots.size(), w.tkeys, w.tmap, s);
    MP_HIP(hipStreamSynchronize(s));
    c.L = MiLaunch{optical, Ho, Wo, H, W, E, G, lds_bins, w.ev, nullptr, nullptr, w.M, w.keys, w.tmap, w.part, w.rowsum, w.colpart};
    return MP_OK;
}

int sigma_check(mp_handle* h, const std::string& fn, double sigma)
{
    if (!(sigma >= 0.0) || (int)(4.0 * sigma + 0.5) > MI_MAX_RADIUS)
        return fail(h, MP_EINVAL, fn + ": smoothing sigma must be in [0, " + std::to_string(MI_MAX_RADIUS / 4) + "]");
    return MP_OK;
}

// one objective launch of the running refinement followed by scipy's decision rules
void refine_iteration(const MiRefine& r, int* live, hipStream_t s)
{
    const MiWorkspace& w = r.w;
    launch_mi_histograms(r.L, w.counts, w.warped, nullptr, 0, s);
    launch_mi_score(r.L, w.counts, r.sigma, r.normalized, r.reg_init, MI_SLOTS, r.smooth_stride, w.smooth_a, w.smooth_b, w.values, s);
    launch_mi_nm_decide(w.state, r.model, r.P, w.candp, w.cand, w.values, w.nact, live, s);
}

// mp_mi_refine_begin and mp_mi_refine_begin_model: `start` device double [n_problems][n], the start parameters of `model`
int mi_refine_begin(mp_handle* h, const std::string& fn, const float* optical, int Ho, int Wo, const float* thermal, int H, int W,
                    int n_pairs, const mp_mi_problem* problems, const double* start, int n_problems, double sigma, int normalized,
                    int regularize, int model, void* workspace, long long workspace_bytes, void* stream)
{
    if (!h) return MP_EINVAL;
    h->mi = MiRefine{};
    if (mi_model_params(model) == 0)
        return fail(h, MP_EINVAL, fn + ": unknown model " + std::to_string(model) +
                                      " (MP_MODEL_HOMOGRAPHY, MP_MODEL_SIMILARITY or MP_MODEL_AFFINE)");
    if (!problems || !start) return fail(h, MP_EINVAL, fn + ": NULL tensor");
    if (n_problems <= 0 || n_problems > MAX_GRID_Y / MI_SLOTS)
        return fail(h, MP_EINVAL, fn + ": need 0 < n_problems <= " + std::to_string(MAX_GRID_Y / MI_SLOTS));
    int rc = sigma_check(h, fn, sigma);
    if (rc != MP_OK) return rc;
    const int P = n_problems, E = P * MI_SLOTS;
    std::vector<int> pair((size_t)E), bins((size_t)E);
    std::vector<MiNmOptions> opts((size_t)P);
    for (int q = 0; q < P; ++q) {
        const mp_mi_problem& pr = problems[q];
        if (pr.maxiter < 1 || pr.maxfun < 1 || !(pr.xatol >= 0.0) || !(pr.fatol >= 0.0))
            return fail(h, MP_EINVAL, fn + ": maxiter and maxfun must be positive, xatol and fatol non-negative");
        for (int v = 0; v < MI_SLOTS; ++v) { pair[q * MI_SLOTS + v] = pr.pair; bins[q * MI_SLOTS + v] = pr.bins; }
        opts[q] = MiNmOptions{pr.maxiter, pr.maxfun, pr.xatol, pr.fatol};
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    MiCall c;
    rc = mi_stage(h, fn, optical, Ho, Wo, thermal, H, W, n_pairs, pair.data(), bins.data(), E, MI_SLOTS, false, sigma > 0.0,
                  workspace, workspace_bytes, s, c);
    if (rc != MP_OK) return rc;
    MiRefine r;
    r.workspace = workspace;
    const MiWorkspace& w = r.w = c.w;
    r.L = c.L;
    r.P = P; r.normalized = normalized != 0; r.model = model; r.sigma = sigma; r.smooth_stride = c.stride;
    r.L.T = w.cand;
    r.L.nact = w.nact;
    // the matrices of the problems' start parameters are kept in the workspace (tinit): the regulariser reads them at every evaluation
    MP_HIP(hipMemcpyAsync(w.opts, opts.data(), opts.size() * sizeof(MiNmOptions), hipMemcpyHostToDevice, s));
    launch_mi_nm_begin(w.state, w.opts, model, start, P, w.candp, w.cand, w.tinit, w.nact, s);
    MP_HIP(hipStreamSynchronize(s));
    r.reg_init = regularize ? w.tinit : nullptr;
    h->mi = r;
    return launch_status(h);
}

}  // namespace

extern "C" {

int mp_mi_workspace_bytes(int n_evals, int n_pairs, int n_thermal_maps, int H, int W, int max_bins, int smoothing,
                          long long* bytes)
{
    if (!bytes || !count_ok(n_evals) || !count_ok(n_pairs) || n_thermal_maps <= 0 || !sides_ok(H, W, 1, 32767) ||
        (long long)H * W > 0x3fffffffLL || max_bins < 1 || max_bins > 256)
        return MP_EINVAL;
    *bytes = (long long)mi_workspace(nullptr, n_evals, n_pairs, n_thermal_maps, H, W, max_bins, smoothing != 0).bytes;
    return MP_OK;
}

int mp_mi_joint_histogram(mp_handle* h, const float* optical, int Ho, int Wo, const float* thermal, int H, int W, int n_pairs,
                          const int* eval_pair, const int* eval_bins, const double* transforms, int n_evals, int strategy,
                          unsigned int* counts, float* minmax, float* warped, void* workspace, long long workspace_bytes,
                          void* stream)
{
    if (!h) return MP_EINVAL;
    if (!transforms || !counts || !minmax) return fail(h, MP_EINVAL, "mp_mi_joint_histogram: NULL tensor");
    if (strategy < 0 || strategy > 2)
        return fail(h, MP_EINVAL, "mp_mi_joint_histogram: strategy must be 0 (by bin count), 1 (LDS copies) or 2 (global atomics)");
    if (strategy == 1 && eval_bins)
        for (int e = 0; e < n_evals; ++e)
            if (eval_bins[e] > 64) return fail(h, MP_EINVAL, "mp_mi_joint_histogram: the LDS copies hold at most 64 bins");
    hipStream_t s = static_cast<hipStream_t>(stream);
    MiCall c;
    const int rc = mi_stage(h, "mp_mi_joint_histogram", optical, Ho, Wo, thermal, H, W, n_pairs, eval_pair, eval_bins, n_evals, 1,
                            true, false, workspace, workspace_bytes, s, c);
    if (rc != MP_OK) return rc;
    c.L.T = transforms;
    launch_mi_histograms(c.L, counts, warped ? warped : c.w.warped, minmax, strategy, s);
    return launch_status(h);
}

int mp_mi_objective(mp_handle* h, const float* optical, int Ho, int Wo, const float* thermal, int H, int W, int n_pairs,
                    const int* eval_pair, const int* eval_bins, const double* transforms, int n_evals, double sigma,
                    int normalized, const double* init_transforms, double* values, void* workspace, long long workspace_bytes,
                    void* stream)
{
    if (!h) return MP_EINVAL;
    if (!transforms || !values) return fail(h, MP_EINVAL, "mp_mi_objective: NULL tensor");
    int rc = sigma_check(h, "mp_mi_objective", sigma);
    if (rc != MP_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    MiCall c;
    rc = mi_stage(h, "mp_mi_objective", optical, Ho, Wo, thermal, H, W, n_pairs, eval_pair, eval_bins, n_evals, 1, false,
                  sigma > 0.0, workspace, workspace_bytes, s, c);
    if (rc != MP_OK) return rc;
    c.L.T = transforms;
    launch_mi_histograms(c.L, c.w.counts, c.w.warped, nullptr, 0, s);
    launch_mi_score(c.L, c.w.counts, sigma, normalized != 0, init_transforms, 1, c.stride, c.w.smooth_a, c.w.smooth_b, values, s);
    return launch_status(h);
}

int mp_mi_refine_begin(mp_handle* h, const float* optical, int Ho, int Wo, const float* thermal, int H, int W, int n_pairs,
                       const mp_mi_problem* problems, const double* init_transforms, int n_problems, double sigma,
                       int normalized, int regularize, void* workspace, long long workspace_bytes, void* stream)
{
    return mi_refine_begin(h, "mp_mi_refine_begin", optical, Ho, Wo, thermal, H, W, n_pairs, problems, init_transforms, n_problems,
                           sigma, normalized, regularize, MP_MODEL_HOMOGRAPHY, workspace, workspace_bytes, stream);
}

int mp_mi_refine_begin_model(mp_handle* h, const float* optical, int Ho, int Wo, const float* thermal, int H, int W, int n_pairs,
                             const mp_mi_problem* problems, const double* init_transforms, int n_problems, double sigma,
                             int normalized, int regularize, void* workspace, long long workspace_bytes, void* stream, int model,
                             const double* init_params)
{
    if (!h) return MP_EINVAL;
    // the homography's parameters are the matrix entries: its caller may hand them in either argument
    const double* start = init_params ? init_params : (model == MP_MODEL_HOMOGRAPHY ? init_transforms : nullptr);
    return mi_refine_begin(h, "mp_mi_refine_begin_model", optical, Ho, Wo, thermal, H, W, n_pairs, problems, start, n_problems,
                           sigma, normalized, regularize, model, workspace, workspace_bytes, stream);
}

int mp_mi_refine_step(mp_handle* h, void* workspace, int n_iters, int* live, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!workspace || !live) return fail(h, MP_EINVAL, "mp_mi_refine_step: NULL tensor");
    if (const int rc = begun_in(h, "mp_mi_refine_step", h->mi.workspace, workspace)) return rc;
    if (n_iters < 1 || n_iters > 100000) return fail(h, MP_EINVAL, "mp_mi_refine_step: n_iters must be in [1, 100000]");
    MP_HIP(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int i = 0; i < n_iters; ++i) refine_iteration(h->mi, live, s);
    return launch_status(h);
}

int mp_mi_refine_result(mp_handle* h, void* workspace, double* transforms, double* values, int* iterations,
                        int* function_calls, int* success, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!workspace || !transforms || !values || !iterations || !function_calls || !success)
        return fail(h, MP_EINVAL, "mp_mi_refine_result: NULL tensor");
    if (const int rc = begun_in(h, "mp_mi_refine_result", h->mi.workspace, workspace)) return rc;
    MP_HIP(hipSetDevice(h->device));
    launch_mi_nm_result(h->mi.w.state, h->mi.model, h->mi.P, transforms, nullptr, values, iterations, function_calls, success,
                        static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_mi_refine_result_model(mp_handle* h, void* workspace, double* transforms, double* values, int* iterations,
                              int* function_calls, int* success, void* stream, double* params)
{
    if (!h) return MP_EINVAL;
    if (!workspace || !transforms || !values || !iterations || !function_calls || !success || !params)
        return fail(h, MP_EINVAL, "mp_mi_refine_result_model: NULL tensor");
    if (const int rc = begun_in(h, "mp_mi_refine_result_model", h->mi.workspace, workspace)) return rc;
    MP_HIP(hipSetDevice(h->device));
    launch_mi_nm_result(h->mi.w.state, h->mi.model, h->mi.P, transforms, params, values, iterations, function_calls, success,
                        static_cast<hipStream_t>(stream));
    return launch_status(h);
}

int mp_mi_model_transform(mp_handle* h, int model, const double* params, int n_rows, double* transforms, void* stream)
{
    if (!h) return MP_EINVAL;
    if (mi_model_params(model) == 0)
        return fail(h, MP_EINVAL, "mp_mi_model_transform: unknown model " + std::to_string(model) +
                                      " (MP_MODEL_HOMOGRAPHY, MP_MODEL_SIMILARITY or MP_MODEL_AFFINE)");
    if (!params || !transforms) return fail(h, MP_EINVAL, "mp_mi_model_transform: NULL tensor");
    if (n_rows <= 0) return fail(h, MP_EINVAL, "mp_mi_model_transform: n_rows must be positive");
    MP_HIP(hipSetDevice(h->device));
    launch_mi_model_transform(model, params, n_rows, transforms, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

}  // extern "C"
