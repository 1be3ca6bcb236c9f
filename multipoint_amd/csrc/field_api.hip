// C ABI of the local alignment correction (field.hip).  The caller owns every buffer, the fit's workspace included;
// nothing is synchronised.
#include "host.h"

using namespace mp_host;

namespace {

bool lattice_ok(int gy, int gx) { return sides_ok(gy, gx, 1, MP_FIELD_MAX_SIDE); }
long long fit_workspace_bytes(int B, int gy, int gx) { return (long long)B * gy * gx * MP_FIELD_WS_DOUBLES * (long long)sizeof(double); }

}  // namespace

extern "C" {

int mp_field_fit_workspace(int B, int gy, int gx, long long* bytes)
{
    if (!bytes || !count_ok(B) || !lattice_ok(gy, gx)) return MP_EINVAL;
    *bytes = fit_workspace_bytes(B, gy, gx);
    return MP_OK;
}

int mp_field_fit(mp_handle* h, const double* d, const double* weight, int B, int gy, int gx, double lambda, double robust_px, int rounds,
                 double tol, int max_iter, void* workspace, long long workspace_bytes, double* out_u, int* out_info, double* out_res,
                 double* out_w, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!d || !weight || !workspace || !out_u || !out_info || !out_res) return fail(h, MP_EINVAL, "mp_field_fit: NULL tensor");
    if (!count_ok(B)) return fail(h, MP_EINVAL, "mp_field_fit: B must be in [1, 65535]");
    if (!lattice_ok(gy, gx))
        return fail(h, MP_EINVAL, "mp_field_fit: the lattice sides must be in [1, " + std::to_string(MP_FIELD_MAX_SIDE) + "]");
    if (!(lambda > 0.0) || !finite64(lambda)) return fail(h, MP_EINVAL, "mp_field_fit: lambda must be positive and finite");
    if (!(robust_px >= 0.0) || !finite64(robust_px)) return fail(h, MP_EINVAL, "mp_field_fit: robust_px must be finite and not negative");
    if (!(tol >= 0.0) || !finite64(tol)) return fail(h, MP_EINVAL, "mp_field_fit: tol must be finite and not negative");
    if (rounds < 0 || rounds > MP_FIELD_MAX_ROUNDS)
        return fail(h, MP_EINVAL, "mp_field_fit: rounds must be in [0, " + std::to_string(MP_FIELD_MAX_ROUNDS) + "]");
    if (max_iter < 1 || max_iter > (1 << 20)) return fail(h, MP_EINVAL, "mp_field_fit: max_iter must be in [1, 2^20]");
    if (const int rc = need_workspace(h, "mp_field_fit", workspace_bytes, (size_t)fit_workspace_bytes(B, gy, gx), "mp_field_fit_workspace"))
        return rc;
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(h, MP_EINVAL, "mp_field_fit: the workspace must be 16-byte aligned");
    // out_u is the solver's working vector and is zeroed before d is read again; out_w is written while the inputs may be in use
    const void* outs[] = {out_u, out_info, out_res, out_w, workspace};
    for (const void* o : outs)
        if (o && (o == static_cast<const void*>(d) || o == static_cast<const void*>(weight)))
            return fail(h, MP_EINVAL, "mp_field_fit: an output or the workspace is one buffer with d or weight");
    if (static_cast<void*>(out_u) == workspace || (out_w && (out_w == out_u || static_cast<void*>(out_w) == workspace)))
        return fail(h, MP_EINVAL, "mp_field_fit: out_u, out_w and the workspace must be three buffers");
    FieldFitParams p{};
    p.d = d, p.weight = weight, p.ws = static_cast<double*>(workspace);
    p.out_u = out_u, p.out_info = out_info, p.out_res = out_res, p.out_w = out_w;
    p.gy = gy, p.gx = gx, p.rounds = rounds, p.max_iter = max_iter;
    p.p_in_lds = field_fit_lds_bytes(gy * gx) > 0;
    p.lambda = lambda, p.robust_px = robust_px, p.tol = tol;
    MP_HIP(hipSetDevice(h->device));
    MP_HIP(launch_field_fit(p, B, static_cast<hipStream_t>(stream)));
    return launch_status(h);
}

int mp_field_warp(mp_handle* h, const float* src, int n_src, int Hs, int Ws, const double* u, int gy, int gx, double y0, double x0,
                  double step, int extrapolate, const double* hom, int B, int H, int W, float* dst, unsigned char* valid, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!src || !u || !dst) return fail(h, MP_EINVAL, "mp_field_warp: NULL tensor");
    if (!count_ok(B)) return fail(h, MP_EINVAL, "mp_field_warp: B must be in [1, 65535]");
    if (n_src != 1 && n_src != B) return fail(h, MP_EINVAL, "mp_field_warp: src holds one frame or one per output frame");
    if (!sides_ok(H, W, 8, 4096) || !sides_ok(Hs, Ws, 8, 4096)) return fail(h, MP_EINVAL, "mp_field_warp: frames must be 8 x 8 to 4096 x 4096");
    if (!lattice_ok(gy, gx))
        return fail(h, MP_EINVAL, "mp_field_warp: the lattice sides must be in [1, " + std::to_string(MP_FIELD_MAX_SIDE) + "]");
    if (!finite64(y0) || !finite64(x0) || !(step > 0.0) || !finite64(step))
        return fail(h, MP_EINVAL, "mp_field_warp: the lattice origin must be finite and its step positive and finite");
    if (extrapolate != 0 && extrapolate != 1) return fail(h, MP_EINVAL, "mp_field_warp: extrapolate is 0 (clamp) or 1 (linear)");
    if (static_cast<const void*>(src) == static_cast<const void*>(dst)) return fail(h, MP_EINVAL, "mp_field_warp: src and dst are one buffer");
    if (reinterpret_cast<uintptr_t>(u) % 16) return fail(h, MP_EINVAL, "mp_field_warp: u must be 16-byte aligned (a node is read as one double2)");
    FieldWarpParams p{};
    p.src = src, p.u = u, p.hom = hom, p.dst = dst, p.valid = valid;
    p.n_src = n_src, p.Hs = Hs, p.Ws = Ws, p.H = H, p.W = W, p.gy = gy, p.gx = gx, p.extrapolate = extrapolate;
    p.y0 = y0, p.x0 = x0, p.step = step;
    MP_HIP(hipSetDevice(h->device));
    launch_field_warp(p, B, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

}  // extern "C"
