// pt_lights.cpp -- the analytic lights of pt_render_nee (include/pt_api.h pins the set, the selection and the estimator): validation, the
// records and the selection table (host, double precision, stored as float), the device copies, and the host statement of the table.
// The kernel side is pt_nee.hip (k_nee*_lights).
#include "pt_context.hpp"

namespace ptamd {

// P_ana as the kernel uses it: u_ana = m 2^-24 (m < 2^24) is below `select` for ceil(select 2^24) values of m
float lights_select(const pt_context* ctx, bool no_other) {
    if (!ctx->lights_pickable) return 0.0f;
    if (no_other) return 1.0f;
    return (float)(std::ceil((double)ctx->lights_select * 16777216.0) / 16777216.0);
}

static bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// empty, or why light i is refused
static std::string light_check(const pt_light& l, int32_t i) {
    const std::string who = "light " + std::to_string(i) + ": ";
    if (l.type != PT_LIGHT_POINT && l.type != PT_LIGHT_DIRECTIONAL) return who + "type must be PT_LIGHT_POINT or PT_LIGHT_DIRECTIONAL";
    if (!finite3(l.position) || !finite3(l.direction) || !finite3(l.intensity) || !std::isfinite(l.cos_inner) || !std::isfinite(l.cos_outer) || !std::isfinite(l.weight))
        return who + "every field must be finite";
    if (!(l.intensity[0] >= 0.0f && l.intensity[1] >= 0.0f && l.intensity[2] >= 0.0f)) return who + "intensity must be >= 0";
    if (!(l.weight >= 0.0f)) return who + "weight must be >= 0";
    if (!(-1.0f <= l.cos_outer && l.cos_outer <= l.cos_inner && l.cos_inner <= 1.0f)) return who + "the cone needs -1 <= cos_outer <= cos_inner <= 1";
    const bool reads_direction = l.type == PT_LIGHT_DIRECTIONAL || l.cos_outer > -1.0f;
    if (reads_direction && l.direction[0] == 0.0f && l.direction[1] == 0.0f && l.direction[2] == 0.0f) return who + "direction must be non-zero";
    return "";
}

}  // namespace ptamd

extern "C" {

void pt_lights_defaults(pt_lights_params* p) {
    if (!p) return;
    p->select = 0.5f;
}

int pt_clear_lights(pt_context* ctx) {
    if (!ctx) return PT_EINVAL;
    ctx->lights.clear();           // the device buffers stay until the next set or pt_destroy
    ctx->lights_rec.clear();
    ctx->lights_cdf.clear();
    ctx->lights_plight.clear();
    ctx->lights_pickable = false;
    ctx->lights_select = 0.5f;
    return PT_OK;
}

int pt_set_lights(pt_context* ctx, const pt_light* lights, int32_t count, const pt_lights_params* params) {
    if (!ctx) return PT_EINVAL;
    pt_lights_params p;
    pt_lights_defaults(&p);
    if (params) p = *params;
    if (count < 0 || count > PT_LIGHTS_MAX) return fail(ctx, PT_EINVAL, "pt_set_lights: count must lie in [0, " + std::to_string(PT_LIGHTS_MAX) + "]");
    if (count > 0 && !lights) return fail(ctx, PT_EINVAL, "pt_set_lights: lights is NULL");
    if (!(p.select >= 0.0f && p.select <= 1.0f)) return fail(ctx, PT_EINVAL, "pt_set_lights: select must lie in [0, 1]");
    for (int32_t i = 0; i < count; ++i) {
        const std::string why = light_check(lights[i], i);
        if (!why.empty()) return fail(ctx, PT_EINVAL, "pt_set_lights: " + why);
    }
    if (count == 0) return pt_clear_lights(ctx);

    const size_t n = (size_t)count;
    std::vector<float> rec(16 * n, 0.0f), cdf(n), plight(n);
    std::vector<double> wgt(n);
    double total = 0.0;
    size_t last = 0;                   // the last pickable light
    for (size_t i = 0; i < n; ++i) {
        const pt_light& l = lights[i];
        float* r = rec.data() + 16 * i;
        const bool cone = l.type == PT_LIGHT_POINT && l.cos_outer > -1.0f;
        if (l.type == PT_LIGHT_POINT) std::memcpy(r, l.position, sizeof(float) * 3);
        std::memcpy(r + 3, &l.type, sizeof(int32_t));
        if (cone || l.type == PT_LIGHT_DIRECTIONAL) {
            const double d[3] = {l.direction[0], l.direction[1], l.direction[2]};
            const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            for (int a = 0; a < 3; ++a) r[4 + a] = (float)(d[a] / len);
        }
        r[7] = cone ? l.cos_inner : -1.0f;
        std::memcpy(r + 8, l.intensity, sizeof(float) * 3);
        r[11] = cone ? l.cos_outer : -1.0f;
        wgt[i] = l.weight > 0.0f ? (double)l.weight : ((double)l.intensity[0] + (double)l.intensity[1]) + (double)l.intensity[2];
        if (!std::isfinite(wgt[i])) wgt[i] = 0.0;
        total += wgt[i];
        if (wgt[i] > 0.0) last = i;
    }
    const bool any = total > 0.0 && std::isfinite(total);
    double run = 0.0;
    for (size_t i = 0; i < n; ++i) {
        run += any ? wgt[i] : 1.0;
        cdf[i] = i >= last || i + 1 == n ? 1.0f : (float)(run / (any ? total : (double)n));
    }
    // P_light as the kernel samples it (the counting rule of the light table, pt_host.cpp): u0 = m 2^-24 picks light j iff
    // cdf[j-1] <= u0 < cdf[j]
    bool pickable = false;
    double below = 0.0;
    for (size_t i = 0; i < n; ++i) {
        const double upto = std::ceil((double)cdf[i] * 16777216.0);
        plight[i] = any ? (float)((upto - below) / 16777216.0) : 0.0f;
        rec[16 * i + 12] = plight[i];
        pickable = pickable || plight[i] > 0.0f;
        below = upto;
    }
    // no set is held while the device copies are replaced: a failed upload leaves the context without lights (pt_debug_lights reports
    // none), never with the old records over new buffers
    pt_clear_lights(ctx);
    if (ctx->has_device) {
        PT_HIP(ctx, hipSetDevice(ctx->device));
        PT_HIP(ctx, hipStreamSynchronize(ctx->stream));     // a frame in flight may still read the previous set
        int rc;
        if ((rc = upload_vec(ctx, &ctx->d_lights_rec, rec.data(), sizeof(float) * rec.size())) != PT_OK) return rc;
        if ((rc = upload_vec(ctx, &ctx->d_lights_cdf, cdf.data(), sizeof(float) * n)) != PT_OK) return rc;
    }
    ctx->lights.assign(lights, lights + n);
    ctx->lights_rec.swap(rec);
    ctx->lights_cdf.swap(cdf);
    ctx->lights_plight.swap(plight);
    ctx->lights_select = p.select;
    ctx->lights_pickable = pickable;
    return PT_OK;
}

int pt_debug_lights(pt_context* ctx, float* records, float* cdf, float* P_light, int64_t cap, int64_t* n, float* P_ana) {
    if (!ctx) return PT_EINVAL;
    if (!n || cap < 0) return fail(ctx, PT_EINVAL, "pt_debug_lights: n is NULL or cap < 0");
    *n = (int64_t)ctx->lights.size();
    const size_t k = (size_t)std::min<int64_t>(cap, *n);
    for (size_t j = 0; j < k; ++j) {
        if (records) std::memcpy(records + 16 * j, ctx->lights_rec.data() + 16 * j, sizeof(float) * 16);
        if (cdf) cdf[j] = ctx->lights_cdf[j];
        if (P_light) P_light[j] = ctx->lights_plight[j];
    }
    if (P_ana) {
        bool no_other = !(ctx->env_set && ctx->env_dist);
        if (no_other && ctx->tris_uploaded && ctx->mats_uploaded) {
            const int rc = light_table_ready(ctx);
            if (rc != PT_OK) return rc;
            no_other = ctx->nee_tri.empty();
        }
        *P_ana = lights_select(ctx, no_other);
    }
    return PT_OK;
}

}  // extern "C"
