// pt_arealights.cpp -- the area lights of pt_render_nee (include/pt_api.h pins the set, the selection and the estimator): validation, the table
// (spheres before suns; host, double precision, stored as float), the device copies, the host statement of the table and pt_debug_area_light_eval.
// The kernel side is pt_nee_arealights.hip.
#include "pt_context.hpp"

namespace ptamd {

// P_area as the kernel uses it: u_area = m 2^-24 (m < 2^24) is below `select` for ceil(select 2^24) values of m
float area_select(const pt_context* ctx, bool no_other) {
    if (!ctx->area_pickable) return 0.0f;
    if (no_other) return 1.0f;
    return (float)(std::ceil((double)ctx->area_select * 16777216.0) / 16777216.0);
}

AreaLightsView area_view(const pt_context* ctx, bool no_other) {
    return AreaLightsView{ctx->d_area_rec, ctx->d_area_cdf, ctx->area_spheres, (int32_t)ctx->area_lights.size(), area_select(ctx, no_other)};
}

static bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// empty, or why light i is refused
static std::string area_check(const pt_area_light& l, int32_t i) {
    const std::string who = "light " + std::to_string(i) + ": ";
    if (l.type != PT_AREA_LIGHT_SPHERE && l.type != PT_AREA_LIGHT_SUN) return who + "type must be PT_AREA_LIGHT_SPHERE or PT_AREA_LIGHT_SUN";
    if (!finite3(l.position) || !finite3(l.direction) || !finite3(l.radiance) || !std::isfinite(l.size) || !std::isfinite(l.weight))
        return who + "every field must be finite";
    if (!(l.radiance[0] >= 0.0f && l.radiance[1] >= 0.0f && l.radiance[2] >= 0.0f)) return who + "radiance must be >= 0";
    if (!(l.weight >= 0.0f)) return who + "weight must be >= 0";
    if (l.type == PT_AREA_LIGHT_SPHERE && !(l.size > 0.0f)) return who + "a sphere's size (its radius) must be > 0";
    if (l.type == PT_AREA_LIGHT_SUN && !(l.size > 0.0f && l.size <= 1.57079637f /* pi / 2 rounded to float */)) return who + "a sun's size (its angular radius) must lie in (0, pi/2]";
    if (l.type == PT_AREA_LIGHT_SUN && l.direction[0] == 0.0f && l.direction[1] == 0.0f && l.direction[2] == 0.0f) return who + "direction must be non-zero";
    return "";
}

// the scene as uploaded has nothing else a light sample could pick
static int area_no_other(pt_context* ctx, bool* no_other) {
    *no_other = !(ctx->env_set && ctx->env_dist) && !lights_on(ctx);
    if (*no_other && ctx->tris_uploaded && ctx->mats_uploaded) {
        const int rc = light_table_ready(ctx);
        if (rc != PT_OK) return rc;
        *no_other = ctx->nee_tri.empty();
    }
    return PT_OK;
}

}  // namespace ptamd

extern "C" {

void pt_area_lights_defaults(pt_area_lights_params* p) {
    if (!p) return;
    p->select = 0.5f;
}

int pt_clear_area_lights(pt_context* ctx) {
    if (!ctx) return PT_EINVAL;
    post_area_lights_changed(ctx);      // lit guides (option aov_lights) show the set: stale, as after an upload
    ctx->area_lights.clear();      // the device buffers stay until the next set or pt_destroy
    ctx->area_rec.clear();
    ctx->area_cdf.clear();
    ctx->area_plight.clear();
    ctx->area_order.clear();
    ctx->area_spheres = 0;
    ctx->area_pickable = false;
    ctx->area_select = 0.5f;
    return PT_OK;
}

int pt_set_area_lights(pt_context* ctx, const pt_area_light* lights, int32_t count, const pt_area_lights_params* params) {
    if (!ctx) return PT_EINVAL;
    pt_area_lights_params p;
    pt_area_lights_defaults(&p);
    if (params) p = *params;
    if (count < 0 || count > PT_AREA_LIGHTS_MAX)
        return fail(ctx, PT_EINVAL, "pt_set_area_lights: count must lie in [0, " + std::to_string(PT_AREA_LIGHTS_MAX) + "]");
    if (count > 0 && !lights) return fail(ctx, PT_EINVAL, "pt_set_area_lights: lights is NULL");
    if (!(p.select >= 0.0f && p.select <= 1.0f)) return fail(ctx, PT_EINVAL, "pt_set_area_lights: select must lie in [0, 1]");
    for (int32_t i = 0; i < count; ++i) {
        const std::string why = area_check(lights[i], i);
        if (!why.empty()) return fail(ctx, PT_EINVAL, "pt_set_area_lights: " + why);
    }
    if (count == 0) return pt_clear_area_lights(ctx);

    const size_t n = (size_t)count;
    std::vector<int32_t> order;
    for (int pass = 0; pass < 2; ++pass)        // spheres, then suns, each in the order given
        for (size_t i = 0; i < n; ++i)
            if ((lights[i].type == PT_AREA_LIGHT_SUN) == (pass == 1)) order.push_back((int32_t)i);
    int32_t spheres = 0;
    std::vector<float> rec(12 * n, 0.0f), cdf(n), plight(n);
    std::vector<double> wgt(n);
    const double pi = 3.14159265358979323846;
    double total = 0.0;
    size_t last = 0;                   // the last pickable light
    for (size_t k = 0; k < n; ++k) {
        const pt_area_light& l = lights[(size_t)order[k]];
        float* r = rec.data() + 12 * k;
        const double sum = ((double)l.radiance[0] + (double)l.radiance[1]) + (double)l.radiance[2];
        double autow;
        if (l.type == PT_AREA_LIGHT_SPHERE) {
            ++spheres;
            std::memcpy(r, l.position, sizeof(float) * 3);
            r[3] = l.size;
            autow = sum * (4.0 * pi * pi) * ((double)l.size * (double)l.size);
        } else {
            const double d[3] = {l.direction[0], l.direction[1], l.direction[2]};
            const double len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            for (int a = 0; a < 3; ++a) r[a] = (float)(-d[a] / len);
            const double sh = std::sin(0.5 * (double)l.size), q = 2.0 * sh * sh;
            r[3] = (float)std::cos((double)l.size);
            r[8] = (float)q;
            autow = sum * (2.0 * pi) * q;
        }
        std::memcpy(r + 4, l.radiance, sizeof(float) * 3);
        wgt[k] = l.weight > 0.0f ? (double)l.weight : autow;
        if (sum == 0.0 || !std::isfinite(wgt[k])) wgt[k] = 0.0;      // a black light is never picked, whatever its weight
        total += wgt[k];
        if (wgt[k] > 0.0) last = k;
    }
    const bool any = total > 0.0 && std::isfinite(total);
    double run = 0.0;
    for (size_t k = 0; k < n; ++k) {
        run += any ? wgt[k] : 1.0;
        cdf[k] = k >= last || k + 1 == n ? 1.0f : (float)(run / (any ? total : (double)n));
    }
    bool pickable = false;
    double below = 0.0;
    for (size_t k = 0; k < n; ++k) {
        const double upto = std::ceil((double)cdf[k] * 16777216.0);
        plight[k] = any ? (float)((upto - below) / 16777216.0) : 0.0f;
        rec[12 * k + 7] = plight[k];
        pickable = pickable || plight[k] > 0.0f;
        below = upto;
    }
    // no set is held while the device copies are replaced, as in pt_set_lights
    pt_clear_area_lights(ctx);
    if (ctx->has_device) {
        PT_HIP(ctx, hipSetDevice(ctx->device));
        PT_HIP(ctx, hipStreamSynchronize(ctx->stream));     // a frame in flight may still read the previous set
        int rc;
        if ((rc = upload_vec(ctx, &ctx->d_area_rec, rec.data(), sizeof(float) * rec.size())) != PT_OK) return rc;
        if ((rc = upload_vec(ctx, &ctx->d_area_cdf, cdf.data(), sizeof(float) * n)) != PT_OK) return rc;
    }
    ctx->area_lights.assign(lights, lights + n);
    ctx->area_rec.swap(rec);
    ctx->area_cdf.swap(cdf);
    ctx->area_plight.swap(plight);
    ctx->area_order.swap(order);
    ctx->area_spheres = spheres;
    ctx->area_select = p.select;
    ctx->area_pickable = pickable;
    return PT_OK;
}

int pt_debug_area_lights(pt_context* ctx, float* records, int32_t* order, float* cdf, float* P_light, int64_t cap, int64_t* n, int32_t* n_sphere,
                         float* P_area) {
    if (!ctx) return PT_EINVAL;
    if (!n || cap < 0) return fail(ctx, PT_EINVAL, "pt_debug_area_lights: n is NULL or cap < 0");
    *n = (int64_t)ctx->area_lights.size();
    if (n_sphere) *n_sphere = ctx->area_spheres;
    const size_t k = (size_t)std::min<int64_t>(cap, *n);
    for (size_t j = 0; j < k; ++j) {
        if (records) std::memcpy(records + 12 * j, ctx->area_rec.data() + 12 * j, sizeof(float) * 12);
        if (order) order[j] = ctx->area_order[j];
        if (cdf) cdf[j] = ctx->area_cdf[j];
        if (P_light) P_light[j] = ctx->area_plight[j];
    }
    if (P_area) {
        bool no_other;
        const int rc = area_no_other(ctx, &no_other);
        if (rc != PT_OK) return rc;
        *P_area = area_select(ctx, no_other);
    }
    return PT_OK;
}

int pt_debug_area_light_eval(pt_context* ctx, const float* origins, const int32_t* lights, const float* u, int64_t n_samples, pt_area_light_sample* samples,
                             const float* rays, int64_t n_hits, pt_area_light_hit* hits) {
    if (!ctx) return PT_EINVAL;
    if (n_samples < 0 || n_hits < 0 || (n_samples > 0 && (!origins || !lights || !u || !samples)) || (n_hits > 0 && (!rays || !hits)))
        return fail(ctx, PT_EINVAL, "pt_debug_area_light_eval: a count < 0, or an array is NULL");
    const int64_t nl = (int64_t)ctx->area_lights.size();
    for (int64_t i = 0; i < n_samples; ++i) {
        if (lights[i] < 0 || lights[i] >= nl) return fail(ctx, PT_EINVAL, "pt_debug_area_light_eval: every light must be an index into the set held");
        if (!(u[2 * i] >= 0.0f && u[2 * i] < 1.0f && u[2 * i + 1] >= 0.0f && u[2 * i + 1] < 1.0f))
            return fail(ctx, PT_EINVAL, "pt_debug_area_light_eval: every u must lie in [0, 1)");
    }
    PT_NEED_DEVICE(ctx);
    if (nl == 0) return fail(ctx, PT_EINVAL, "pt_debug_area_light_eval: no area-light set is held");
    if (n_samples == 0 && n_hits == 0) return PT_OK;
    PT_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<float> s_in((size_t)n_samples * 6), h_in;
    for (int64_t i = 0; i < n_samples; ++i) {
        float* q = s_in.data() + 6 * i;
        std::memcpy(q, origins + 3 * i, 12);
        std::memcpy(q + 3, lights + i, 4);
        q[4] = u[2 * i];
        q[5] = u[2 * i + 1];
    }
    if (n_hits > 0) h_in.assign(rays, rays + 7 * n_hits);
    std::vector<int32_t> s_out((size_t)n_samples * 6), h_out((size_t)n_hits * 4);
    DeviceBuf d_si, d_so, d_hi, d_ho;      // (one float at least, so that every pointer is a device pointer)
    PT_HIP(ctx, d_si.alloc(sizeof(float) * std::max<size_t>(s_in.size(), 1)));
    PT_HIP(ctx, d_so.alloc(sizeof(int32_t) * std::max<size_t>(s_out.size(), 1)));
    PT_HIP(ctx, d_hi.alloc(sizeof(float) * std::max<size_t>(h_in.size(), 1)));
    PT_HIP(ctx, d_ho.alloc(sizeof(int32_t) * std::max<size_t>(h_out.size(), 1)));
    if (!s_in.empty()) PT_HIP(ctx, hipMemcpy(d_si.p, s_in.data(), sizeof(float) * s_in.size(), hipMemcpyHostToDevice));
    if (!h_in.empty()) PT_HIP(ctx, hipMemcpy(d_hi.p, h_in.data(), sizeof(float) * h_in.size(), hipMemcpyHostToDevice));
    const AreaLightsView v = area_view(ctx, true);
    PT_HIP(ctx, launch_debug_area_light(v, (const float*)d_si.p, n_samples, (int32_t*)d_so.p, (const float*)d_hi.p, n_hits, (int32_t*)d_ho.p, ctx->stream));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (!s_out.empty()) PT_HIP(ctx, hipMemcpy(s_out.data(), d_so.p, sizeof(int32_t) * s_out.size(), hipMemcpyDeviceToHost));
    if (!h_out.empty()) PT_HIP(ctx, hipMemcpy(h_out.data(), d_ho.p, sizeof(int32_t) * h_out.size(), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n_samples; ++i) {
        std::memcpy(&samples[i], s_out.data() + 6 * i, 24);
        if (!samples[i].accept) {
            samples[i].w[0] = samples[i].w[1] = samples[i].w[2] = samples[i].p_omega = 0.0f;
            samples[i].t_s = std::numeric_limits<float>::infinity();
        }
    }
    for (int64_t i = 0; i < n_hits; ++i) std::memcpy(&hits[i], h_out.data() + 4 * i, 16);
    return PT_OK;
}

}  // extern "C"
