// C ABI of the local residual field (residual.hip).  The caller owns every buffer; nothing is synchronised and no
// workspace is needed: one launch over (window, frame).
#include "host.h"

using namespace mp_host;

namespace {

bool window_ok(int w) { return w == 8 || w == 16 || w == 24 || w == 32 || w == 48 || w == 64; }

// windows per column and row; false for parameters or sizes the kernel does not take
bool residual_grid(int H, int W, int w, int s, int r, int* gy, int* gx)
{
    if (H < 8 || W < 8 || H > 4096 || W > 4096 || !window_ok(w) || s < 1 || r < 1 || r > MP_RES_MAX_RADIUS) return false;
    if (H < w + 2 * r || W < w + 2 * r) return false;
    *gy = (H - w - 2 * r) / s + 1;
    *gx = (W - w - 2 * r) / s + 1;
    return true;
}

}  // namespace

extern "C" {

int mp_residual_grid(int H, int W, int window, int stride, int radius, int* gy, int* gx)
{
    if (!gy || !gx || !residual_grid(H, W, window, stride, radius, gy, gx)) return MP_EINVAL;
    return MP_OK;
}

int mp_residual_field(mp_handle* h, const float* optical_feat, const float* thermal_feat, const unsigned char* mask, int mask_frames,
                      int B, int H, int W, int window, int stride, int radius, double min_valid, double var_floor, double* out_d,
                      int* out_i, void* stream)
{
    if (!h) return MP_EINVAL;
    if (!optical_feat || !thermal_feat || !out_d || !out_i) return fail(h, MP_EINVAL, "mp_residual_field: NULL tensor");
    if (!count_ok(B)) return fail(h, MP_EINVAL, "mp_residual_field: B must be in [1, 65535]");
    if (H < 8 || W < 8 || H > 4096 || W > 4096) return fail(h, MP_EINVAL, "mp_residual_field: frames must be 8 x 8 to 4096 x 4096");
    if (!window_ok(window)) return fail(h, MP_EINVAL, "mp_residual_field: window must be 8, 16, 24, 32, 48 or 64");
    if (stride < 1) return fail(h, MP_EINVAL, "mp_residual_field: stride must be positive");
    if (radius < 1 || radius > MP_RES_MAX_RADIUS)
        return fail(h, MP_EINVAL, "mp_residual_field: radius must be in [1, " + std::to_string(MP_RES_MAX_RADIUS) + "]");
    if (!(min_valid > 0.0 && min_valid <= 1.0)) return fail(h, MP_EINVAL, "mp_residual_field: min_valid must be in (0, 1]");
    if (!(var_floor >= 0.0) || var_floor > 1.7976931348623157e308)
        return fail(h, MP_EINVAL, "mp_residual_field: var_floor must be finite and not negative");
    if (mask && mask_frames != 1 && mask_frames != B)
        return fail(h, MP_EINVAL, "mp_residual_field: the mask holds one plane or one per frame");
    ResidualParams p{};
    if (!residual_grid(H, W, window, stride, radius, &p.gy, &p.gx))
        return fail(h, MP_EINVAL, "mp_residual_field: a " + std::to_string(H) + " x " + std::to_string(W) + " frame holds no window of " +
                                      std::to_string(window) + " + 2 x " + std::to_string(radius) + " pixels");
    p.fo = optical_feat, p.ft = thermal_feat, p.mask = mask, p.mask_frames = mask ? mask_frames : 1;
    p.H = H, p.W = W, p.w = window, p.s = stride, p.r = radius;
    p.min_valid = min_valid, p.var_floor = var_floor;
    p.out_d = out_d, p.out_i = out_i;
    MP_HIP(hipSetDevice(h->device));
    launch_residual_field(p, B, static_cast<hipStream_t>(stream));
    return launch_status(h);
}

}  // extern "C"
