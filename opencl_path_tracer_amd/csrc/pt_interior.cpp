// pt_interior.cpp -- the interiors of dielectrics on pt_render_nee (include/pt_api.h pins the record, the free flight, the absorption factor and
// the scatter vertex): validation, storage per material index, the table the kernels read and pt_debug_interior's host
// side.  The kernel side is pt_nee.hip (k_nee*_interior, compiled in pt_nee_interior.hip) and pt_medium.hip (k_debug_interior); the refusals of
// the paths that would drop an interior sit with the other refusals in pt_launch.cpp.
#include "pt_context.hpp"

#include <cmath>
#include <cstring>

namespace ptamd {

// empty, or the field that is refused and why
static std::string interior_check(const pt_interior& in) {
    for (int c = 0; c < 3; ++c)
        if (!(std::isfinite(in.sigma_a[c]) && in.sigma_a[c] >= 0.0f)) return "sigma_a must be finite and >= 0 in every channel";
    if (!(std::isfinite(in.sigma_s) && in.sigma_s >= 0.0f)) return "sigma_s must be finite and >= 0";
    if (!(std::fabs(in.g) <= 0.99f)) return "g must lie in [-0.99, 0.99]";
    return "";
}

// The table of the materials on the device: {sigma_a.rgb, sigma_s}, {g, bound, 0, 0} per material, bound only where a binding is held and the
// uploaded material is of type 2 or 6 (as a texture binding counts only on a diffuse one).  The new copy first, then the old one is freed
int interior_prepare(pt_context* ctx, InteriorView* iv) {
    PT_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->interior_dirty || !ctx->d_interior) {
        const size_t nmat = std::max<size_t>((size_t)ctx->mats_on_device, 1);      // (one readable record for an empty scene)
        std::vector<float> rec(nmat * 8, 0.0f);
        for (size_t i = 0; i < std::min<size_t>({(size_t)ctx->mats_on_device, ctx->interior_bound.size(), ctx->mats.size()}); ++i) {
            if (!ctx->interior_bound[i] || !(ctx->mats[i].type == 2 || ctx->mats[i].type == 6)) continue;
            const pt_interior& in = ctx->interiors[i];
            float* r = rec.data() + i * 8;
            r[0] = in.sigma_a[0];
            r[1] = in.sigma_a[1];
            r[2] = in.sigma_a[2];
            r[3] = in.sigma_s;
            r[4] = in.g;
            r[5] = 1.0f;
        }
        PT_HIP(ctx, hipStreamSynchronize(ctx->stream));      // a frame in flight may still read the previous table
        DeviceArray<float4> fresh;
        int rc;
        if ((rc = upload_vec(ctx, &fresh, rec.data(), sizeof(float) * rec.size())) != PT_OK) return rc;
        ctx->d_interior = std::move(fresh);
        ctx->interior_dirty = false;
    }
    iv->rec = ctx->d_interior;
    return PT_OK;
}

}  // namespace ptamd

using namespace ptamd;

extern "C" {

void pt_interior_defaults(pt_interior* in) {
    if (!in) return;
    in->sigma_a[0] = in->sigma_a[1] = in->sigma_a[2] = 0.0f;
    in->sigma_s = 0.0f;
    in->g = 0.0f;
}

int pt_set_material_interior(pt_context* ctx, int32_t material, const pt_interior* interior) {
    if (!ctx) return PT_EINVAL;
    if (!interior) return fail(ctx, PT_EINVAL, "pt_set_material_interior: interior is NULL");
    if (material < 0 || (size_t)material >= ctx->mats.size())
        return fail(ctx, PT_EINVAL, "pt_set_material_interior: material must be the index of a material added so far");
    const std::string why = interior_check(*interior);
    if (!why.empty()) return fail(ctx, PT_EINVAL, "pt_set_material_interior: " + why);
    if (ctx->interiors.size() <= (size_t)material) {
        pt_interior none;
        pt_interior_defaults(&none);
        ctx->interiors.resize((size_t)material + 1, none);
        ctx->interior_bound.resize((size_t)material + 1, 0);
    }
    if (!ctx->interior_bound[(size_t)material]) ++ctx->interior_live;
    ctx->interiors[(size_t)material] = *interior;
    ctx->interior_bound[(size_t)material] = 1;
    ctx->interior_dirty = true;
    return PT_OK;
}

int pt_clear_material_interiors(pt_context* ctx) {
    if (!ctx) return PT_EINVAL;
    ctx->interiors.clear();
    ctx->interior_bound.clear();
    ctx->interior_live = 0;
    ctx->interior_dirty = true;      // (the table stays on the device until the next binding replaces it or the context goes)
    return PT_OK;
}

int pt_get_material_interior(const pt_context* ctx, int32_t material, pt_interior* interior) {
    if (!ctx || !interior) return PT_EINVAL;
    if (material < 0 || (size_t)material >= ctx->mats.size()) return PT_EINVAL;
    const bool held = (size_t)material < ctx->interior_bound.size() && ctx->interior_bound[(size_t)material];
    if (held) *interior = ctx->interiors[(size_t)material];
    else pt_interior_defaults(interior);
    return held ? 1 : 0;
}

int pt_debug_interior(pt_context* ctx, const float* in, int64_t n, float* out) {
    if (!ctx) return PT_EINVAL;
    if (n < 0 || (n > 0 && (!in || !out))) return fail(ctx, PT_EINVAL, "pt_debug_interior: n < 0, or in / out is NULL");
    PT_NEED_DEVICE(ctx);
    if (n == 0) return PT_OK;
    return debug_round_trip(ctx, in, sizeof(float) * 12 * (size_t)n, out, sizeof(float) * 10 * (size_t)n,
                            [&](void* d_in, void* d_out) { return launch_debug_interior((const float*)d_in, n, (float*)d_out, ctx->stream); });
}

}  // extern "C"
