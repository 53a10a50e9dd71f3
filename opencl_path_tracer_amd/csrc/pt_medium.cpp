// pt_medium.cpp -- the homogeneous participating medium of pt_render_nee (include/pt_api.h pins the record, the free flight, the scatter
// vertex and the transmittance of light samples): validation, the view the kernels read, and pt_debug_medium's host side.  The kernel side
// is pt_nee.hip (k_nee*_medium) and pt_medium.hip (k_debug_medium); the refusals of the paths that would drop the fog sit with the
// other refusals in pt_launch.cpp.
#include "pt_context.hpp"

namespace ptamd {

MediumView medium_view(const pt_context* ctx) {
    const pt_medium& m = ctx->medium;
    MediumView v;
    v.sigma_t = m.sigma_t;
    v.g = m.g;
    for (int a = 0; a < 3; ++a) {
        v.albedo[a] = m.albedo[a];
        v.lo[a] = m.lo[a];
        v.hi[a] = m.hi[a];
    }
    return v;
}

// empty, or the field that is refused and why
static std::string medium_check(const pt_medium& m) {
    if (!(std::isfinite(m.sigma_t) && m.sigma_t >= 0.0f)) return "sigma_t must be finite and >= 0";
    for (int a = 0; a < 3; ++a)
        if (!(m.albedo[a] >= 0.0f && m.albedo[a] <= 1.0f)) return "albedo must lie in [0, 1]";
    if (!(std::fabs(m.g) <= 0.99f)) return "g must lie in [-0.99, 0.99]";
    for (int a = 0; a < 3; ++a)
        if (!(m.lo[a] < m.hi[a])) return "lo must be below hi on every axis (and neither a NaN)";      // (-inf / +inf are allowed)
    return "";
}

}  // namespace ptamd

extern "C" {

void pt_medium_defaults(pt_medium* m) {
    if (!m) return;
    m->sigma_t = 0.0f;
    m->g = 0.0f;
    for (int a = 0; a < 3; ++a) {
        m->albedo[a] = 1.0f;
        m->lo[a] = -std::numeric_limits<float>::infinity();
        m->hi[a] = std::numeric_limits<float>::infinity();
    }
}

int pt_set_medium(pt_context* ctx, const pt_medium* m) {
    if (!ctx) return PT_EINVAL;
    if (!m) return fail(ctx, PT_EINVAL, "pt_set_medium: medium is NULL");
    const std::string why = medium_check(*m);
    if (!why.empty()) return fail(ctx, PT_EINVAL, "pt_set_medium: " + why);
    ctx->medium = *m;          // (a kernel argument by value: a frame in flight keeps the view it was launched with)
    ctx->medium_set = true;
    return PT_OK;
}

int pt_clear_medium(pt_context* ctx) {
    if (!ctx) return PT_EINVAL;
    pt_medium_defaults(&ctx->medium);
    ctx->medium_set = false;
    return PT_OK;
}

int pt_get_medium(const pt_context* ctx, pt_medium* m) {
    if (!ctx || !m) return PT_EINVAL;
    *m = ctx->medium;
    return ctx->medium_set ? 1 : 0;
}

int pt_debug_medium(pt_context* ctx, const float* in, int64_t n, float* out) {
    if (!ctx) return PT_EINVAL;
    if (n < 0 || (n > 0 && (!in || !out))) return fail(ctx, PT_EINVAL, "pt_debug_medium: n < 0, or in / out is NULL");
    if (!medium_on(ctx)) return fail(ctx, PT_EINVAL, "pt_debug_medium: no medium with sigma_t > 0 is held (pt_set_medium)");
    PT_NEED_DEVICE(ctx);
    if (n == 0) return PT_OK;
    PT_HIP(ctx, hipSetDevice(ctx->device));
    struct Buf {
        void* p = nullptr;
        ~Buf() { if (p) (void)hipFree(p); }
    } d_in, d_out;
    PT_HIP(ctx, hipMalloc(&d_in.p, sizeof(float) * 12 * (size_t)n));
    PT_HIP(ctx, hipMalloc(&d_out.p, sizeof(float) * 10 * (size_t)n));
    PT_HIP(ctx, hipMemcpy(d_in.p, in, sizeof(float) * 12 * (size_t)n, hipMemcpyHostToDevice));
    PT_HIP(ctx, launch_debug_medium(medium_view(ctx), (const float*)d_in.p, n, (float*)d_out.p, ctx->stream));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP(ctx, hipMemcpy(out, d_out.p, sizeof(float) * 10 * (size_t)n, hipMemcpyDeviceToHost));
    return PT_OK;
}

}  // extern "C"
