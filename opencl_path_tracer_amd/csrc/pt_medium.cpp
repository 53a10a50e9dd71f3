// pt_medium.cpp -- the homogeneous participating medium of pt_render_nee (include/pt_api.h pins the record, the free flight, the scatter
// vertex and the transmittance of light samples): validation, the view the kernels read, and pt_debug_medium's host side.  The kernel side
// is pt_nee.hip (k_nee*_medium, k_nee*_grid) and pt_medium.hip (k_debug_medium, k_debug_grid).  The medium's density grid
// (pt_set_medium_density) is kept here too: validation, storage, the device copy and its view.  The refusals of the paths that would drop the fog sit with the
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

GridView grid_view(const pt_context* ctx) {
    const pt_medium& m = ctx->medium;
    GridView v;
    v.rho = ctx->d_grid;
    for (int a = 0; a < 3; ++a) {
        const float n = (float)ctx->grid_n[a], w = m.hi[a] - m.lo[a];
        v.n[a] = ctx->grid_n[a];
        v.cell[a] = w / n;
        v.inv_cell[a] = n / w;
    }
    return v;
}

std::string grid_unbounded(const pt_context* ctx) {
    static const char* const axis[3] = {"x", "y", "z"};
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(ctx->medium.lo[a])) return std::string("a density grid is held and the medium's lo.") + axis[a] + " is infinite: the grid divides a finite box (pt_set_medium)";
        if (!std::isfinite(ctx->medium.hi[a])) return std::string("a density grid is held and the medium's hi.") + axis[a] + " is infinite: the grid divides a finite box (pt_set_medium)";
    }
    return "";
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

int pt_set_medium_density(pt_context* ctx, const float* density, int32_t nx, int32_t ny, int32_t nz) {
    if (!ctx) return PT_EINVAL;
    if (!density) return fail(ctx, PT_EINVAL, "pt_set_medium_density: density is NULL");
    const int32_t dims[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a)
        if (dims[a] < 1 || dims[a] > PT_GRID_MAX_DIM)
            return fail(ctx, PT_EINVAL, "pt_set_medium_density: every dimension must lie in [1, " + std::to_string(PT_GRID_MAX_DIM) + "]");
    const size_t count = (size_t)nx * (size_t)ny * (size_t)nz;
    for (size_t i = 0; i < count; ++i)
        if (!(std::isfinite(density[i]) && density[i] >= 0.0f))
            return fail(ctx, PT_EINVAL, "pt_set_medium_density: density " + std::to_string(i) + " is negative or not finite");
    if (ctx->has_device) {
        // the copy first, so that a failed upload leaves the held grid as it was; a frame in flight may still read the previous one
        PT_HIP(ctx, hipSetDevice(ctx->device));
        PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        DeviceArray<float> fresh;
        int rc;
        if ((rc = upload_vec(ctx, &fresh, density, sizeof(float) * count)) != PT_OK) return rc;
        ctx->d_grid = std::move(fresh);
    }
    ctx->grid.assign(density, density + count);
    for (int a = 0; a < 3; ++a) ctx->grid_n[a] = dims[a];
    ctx->grid_set = true;
    return PT_OK;
}

int pt_clear_medium_density(pt_context* ctx) {
    if (!ctx) return PT_EINVAL;
    if (ctx->d_grid) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        ctx->d_grid.reset();
    }
    std::vector<float>().swap(ctx->grid);
    ctx->grid_n[0] = ctx->grid_n[1] = ctx->grid_n[2] = 0;
    ctx->grid_set = false;
    return PT_OK;
}

int pt_debug_medium_density(pt_context* ctx, float* out, int64_t cap, int32_t dims[3]) {
    if (!ctx) return PT_EINVAL;
    if (!dims || cap < 0 || (cap > 0 && !out)) return fail(ctx, PT_EINVAL, "pt_debug_medium_density: dims is NULL, cap < 0, or out is NULL");
    for (int a = 0; a < 3; ++a) dims[a] = ctx->grid_n[a];
    const size_t k = std::min<size_t>((size_t)cap, ctx->grid.size());
    if (k) std::memcpy(out, ctx->grid.data(), sizeof(float) * k);
    return ctx->grid_set ? 1 : 0;
}

int pt_debug_grid(pt_context* ctx, const float* in, int64_t n, float* out) {
    if (!ctx) return PT_EINVAL;
    if (n < 0 || (n > 0 && (!in || !out))) return fail(ctx, PT_EINVAL, "pt_debug_grid: n < 0, or in / out is NULL");
    if (!grid_on(ctx)) return fail(ctx, PT_EINVAL, "pt_debug_grid: no density grid is live (pt_set_medium with sigma_t > 0 and pt_set_medium_density)");
    if (!grid_unbounded(ctx).empty()) return fail(ctx, PT_EINVAL, "pt_debug_grid: " + grid_unbounded(ctx));
    PT_NEED_DEVICE(ctx);
    if (n == 0) return PT_OK;
    return debug_round_trip(ctx, in, sizeof(float) * 12 * (size_t)n, out, sizeof(float) * 8 * (size_t)n, [&](void* d_in, void* d_out) {
        return launch_debug_grid(medium_view(ctx), grid_view(ctx), (const float*)d_in, n, (float*)d_out, ctx->stream);
    });
}

int pt_debug_medium(pt_context* ctx, const float* in, int64_t n, float* out) {
    if (!ctx) return PT_EINVAL;
    if (n < 0 || (n > 0 && (!in || !out))) return fail(ctx, PT_EINVAL, "pt_debug_medium: n < 0, or in / out is NULL");
    if (!medium_on(ctx)) return fail(ctx, PT_EINVAL, "pt_debug_medium: no medium with sigma_t > 0 is held (pt_set_medium)");
    PT_NEED_DEVICE(ctx);
    if (n == 0) return PT_OK;
    return debug_round_trip(ctx, in, sizeof(float) * 12 * (size_t)n, out, sizeof(float) * 10 * (size_t)n,
                            [&](void* d_in, void* d_out) { return launch_debug_medium(medium_view(ctx), (const float*)d_in, n, (float*)d_out, ctx->stream); });
}

}  // extern "C"
