// pt_post.cpp -- the post-process chain of libptamd.so: guide buffers, the a-trous filter, the variance read-out, the variance-guided
// filter, temporal accumulation, the firefly filter and the display stage (kernels: pt_denoise.hip, pt_temporal.hip, pt_despeckle.hip,
// pt_display.hip; every stage is pinned in include/pt_api.h), and what makes their results stale.  No file but this one writes the
// validity fields of the chain (pt_context.hpp, "the post-process chain"): the rest of the library reports what happened through the
// post_* functions below.
#include "pt_context.hpp"

namespace ptamd {

// ---- the state transitions of the chain
// pt_upload_triangles / pt_upload_materials: whatever was made from the old scene is stale
void post_scene_uploaded(pt_context* ctx) {
    ctx->aov_valid = false;
    ctx->despeckle_valid = false;    // (pt_despeckle's result is a frame of the old scene)
    ctx->display_has_prev = false;   // (and pt_display's remembered exposure its brightness)
}
// Shaded guides (pt_render_aovs_ex, PT_AOV_SHADED) are a snapshot of the vertex normals, uvs, textures and bindings: an authoring call
// for any of them makes them stale, as an upload makes any guides stale.  Geometric guides read none of that and stay valid.
void post_shading_inputs_changed(pt_context* ctx) {
    if (ctx->aov_shaded) ctx->aov_valid = false;
}
// lit guides (option aov_lights) show the area set: stale when it changes, as after an upload
void post_area_lights_changed(pt_context* ctx) {
    if (ctx->aov_lit) ctx->aov_valid = false;
}
// a guide launch through cam was enqueued
static void guides_rendered(pt_context* ctx, const pt_camera* cam, bool shaded, bool lit) {
    // the first guides after pt_upload_triangles / pt_upload_materials (which made the old ones stale): the temporal history describes
    // the old scene, and every accumulate needs guides, so this is where it is dropped
    if (!ctx->aov_valid) ctx->temporal_history = false;
    ctx->aov_valid = true;
    ctx->aov_shaded = shaded;
    ctx->aov_lit = lit;
    ctx->aov_cam = *cam;
    ++ctx->aov_serial;
}

// ---- the refusals the stages share (`who`: the entry point's name, the prefix of its texts)
static int need_one_rank(pt_context* ctx, const char* who) {
    return ctx->world == 1 ? PT_OK : fail(ctx, PT_EINVAL, std::string(who) + ": contexts of one rank (world == 1) only");
}
static int need_guides(pt_context* ctx, const char* who) {
    return ctx->aov_valid ? PT_OK : fail(ctx, PT_EINVAL, std::string(who) + ": no guides (pt_render_aovs has not run since the scene was last uploaded)");
}

// the lit instances of k_aovs: option aov_lights, and an area set with a non-black light (what selects kNeeAreaLights)
static bool aov_lit_now(const pt_context* ctx) { return ctx->aov_lights && area_on(ctx); }
static const char* guide_args_error(int32_t subpixels, int32_t specular_depth) {
    if (subpixels < 1 || subpixels > 8) return "subpixels must be 1..8";
    if (specular_depth < 0 || specular_depth > 16) return "specular_depth must be 0..16";
    return nullptr;
}
// The guide launch of pt_render_aovs and pt_render_aovs_ex, after their argument checks: prepare() readies what the shaded launcher
// reads besides RenderParams, launch(p, lit, lights) enqueues the kernel
template <class Prepare, class Launch>
static int render_guides(pt_context* ctx, const pt_camera* cam, bool shaded, Prepare prepare, Launch launch) {
    PT_NEED_DEVICE(ctx);
    int rc = check_ready(ctx, cam);
    if (rc != PT_OK) return rc;
    PT_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = prepare()) != PT_OK) return rc;
    PT_ALLOC(ctx, ctx->d_aov.reserve(2 * (size_t)std::max<int64_t>(ctx->npix, 1)));
    RenderParams p;
    fill_params(ctx, cam, &p);         // the render kernels' node placement
    const bool lit = aov_lit_now(ctx);
    const AreaLightsView lights = area_view(ctx, true);
    if ((rc = launch(p, lit, lights)) != PT_OK) return rc;
    guides_rendered(ctx, cam, shaded, lit);
    return PT_OK;
}

// The a-trous ping-pong over the two d_dn buffers: iteration i reads in0 (i == 0) or what iteration i - 1 wrote, launch(i, in, out)
// enqueues it, and d_denoised is left at what the last one wrote
template <class Launch>
static int atrous_iterations(pt_context* ctx, int iterations, const float4* in0, Launch launch) {
    const size_t npix = (size_t)ctx->npix;
    PT_ALLOC(ctx, ctx->d_dn.reserve(2 * std::max<size_t>(npix, 1)));
    for (int i = 0; i < iterations; ++i) {
        const float4* in = i == 0 ? in0 : ctx->d_dn + ((i - 1) & 1) * npix;
        float4* out = ctx->d_dn + (i & 1) * npix;
        const int rc = launch(i, in, out);
        if (rc != PT_OK) return rc;
    }
    ctx->d_denoised = ctx->d_dn + ((iterations - 1) & 1) * npix;
    return PT_OK;
}

}  // namespace ptamd

extern "C" {

// ---- guide buffers + a-trous denoiser (kernels: pt_denoise.hip; the filter is pinned in include/pt_api.h)
int pt_render_aovs(pt_context* ctx, const pt_camera* cam, int32_t subpixels, int32_t specular_depth) {
    if (!ctx) return PT_EINVAL;
    if (const char* why = guide_args_error(subpixels, specular_depth)) return fail(ctx, PT_EINVAL, std::string("pt_render_aovs: ") + why);
    return render_guides(ctx, cam, false, [] { return PT_OK; }, [&](const RenderParams& p, bool lit, const AreaLightsView& lights) {
        PT_HIP(ctx, launch_aovs(p, subpixels, specular_depth, ctx->npix, ctx->d_aov, ctx->d_aov + ctx->npix, lit ? &lights : nullptr, ctx->cu_count, ctx->stream));
        return (int)PT_OK;
    });
}
void pt_aov_defaults(pt_aov_params* p) {
    if (!p) return;
    p->subpixels = 1;
    p->specular_depth = 4;
    p->shading = PT_AOV_GEOMETRIC;
}
int pt_render_aovs_ex(pt_context* ctx, const pt_camera* cam, const pt_aov_params* ap) {
    if (!ctx) return PT_EINVAL;
    if (!ap) return fail(ctx, PT_EINVAL, "pt_render_aovs_ex: params is NULL");
    if (const char* why = guide_args_error(ap->subpixels, ap->specular_depth)) return fail(ctx, PT_EINVAL, std::string("pt_render_aovs_ex: ") + why);
    if (ap->shading != PT_AOV_GEOMETRIC && ap->shading != PT_AOV_SHADED)
        return fail(ctx, PT_EINVAL, "pt_render_aovs_ex: shading must be PT_AOV_GEOMETRIC or PT_AOV_SHADED");
    if (ap->shading == PT_AOV_GEOMETRIC) return pt_render_aovs(ctx, cam, ap->subpixels, ap->specular_depth);
    const float4* vn = nullptr;        // option smooth_normals: the packed vertex normals
    TexView tv;                        // option textures: uvs, texels, descriptors, bindings
    auto prepare = [&] {
        const int rc = smooth_prepare(ctx, &vn);
        return rc != PT_OK ? rc : texture_prepare(ctx, &tv);
    };
    return render_guides(ctx, cam, true, prepare, [&](const RenderParams& p, bool lit, const AreaLightsView& lights) {
        PT_HIP(ctx, launch_aovs_shaded(p, ap->subpixels, ap->specular_depth, ctx->npix, ctx->d_aov, ctx->d_aov + ctx->npix, vn, tv, ctx->glossy, ctx->coated, ctx->frosted,
                                       lit ? &lights : nullptr, ctx->cu_count, ctx->stream));
        return (int)PT_OK;
    });
}
int pt_read_aovs(pt_context* ctx, float* albedo_rgbm, float* normal_depth, int64_t npix) {
    PT_NEED_DEVICE(ctx);
    if (npix != ctx->npix) return fail(ctx, PT_EINVAL, "npix must equal the local pixel count");
    if (!ctx->d_aov) return fail(ctx, PT_EINVAL, "pt_read_aovs: pt_render_aovs has not run");
    int rc = PT_OK;
    if (albedo_rgbm && (rc = read_back(ctx, albedo_rgbm, ctx->d_aov, sizeof(float4) * (size_t)npix)) != PT_OK) return rc;
    if (normal_depth && (rc = read_back(ctx, normal_depth, ctx->d_aov + npix, sizeof(float4) * (size_t)npix)) != PT_OK) return rc;
    return PT_OK;
}
void pt_denoise_defaults(pt_denoise_params* p) {
    if (!p) return;
    p->iterations = 3;
    p->sigma_color = 0.125f;
    p->sigma_normal = 8.0f;
    p->sigma_depth = 0.05f;
    p->demodulate = 1;
}
int pt_denoise(pt_context* ctx, const pt_denoise_params* dp) {
    if (!ctx) return PT_EINVAL;
    if (!dp) return fail(ctx, PT_EINVAL, "pt_denoise: params is NULL");
    if (dp->iterations < 1 || dp->iterations > 10) return fail(ctx, PT_EINVAL, "pt_denoise: iterations must be 1..10");
    if (!(dp->sigma_color >= 0.0f) || !(dp->sigma_normal >= 0.0f) || !(dp->sigma_depth >= 0.0f))
        return fail(ctx, PT_EINVAL, "pt_denoise: sigmas must be >= 0 (and not NaN)");
    int rc = need_one_rank(ctx, "pt_denoise");
    if (rc != PT_OK || (rc = need_guides(ctx, "pt_denoise")) != PT_OK) return rc;
    PT_NEED_DEVICE(ctx);
    PT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->npix;
    return atrous_iterations(ctx, dp->iterations, ctx->d_colors, [&](int i, const float4* in, float4* out) {
        AtrousStep s;
        s.step = 1 << i;
        s.demodulate = dp->demodulate ? 1 : 0;
        s.color_on = std::isfinite(dp->sigma_color) ? 1 : 0;
        s.normal_on = std::isfinite(dp->sigma_normal) && dp->sigma_normal > 0.0f ? 1 : 0;
        s.depth_on = std::isfinite(dp->sigma_depth) ? 1 : 0;
        s.color_scale = (float)(1 << (2 * i));
        s.sigma_color2 = dp->sigma_color * dp->sigma_color;
        s.sigma_normal = dp->sigma_normal;
        s.sigma_depth = dp->sigma_depth;
        PT_HIP(ctx, launch_atrous(in, out, ctx->d_aov, ctx->d_aov + npix, ctx->W, ctx->local_rows, s, i == 0, i == dp->iterations - 1, ctx->stream));
        return (int)PT_OK;
    });
}
int pt_read_denoised(pt_context* ctx, float* out, int64_t npix) {
    PT_NEED_DEVICE(ctx);
    if (!out || npix != ctx->npix) return fail(ctx, PT_EINVAL, "npix must equal the local pixel count");
    if (!ctx->d_denoised) return fail(ctx, PT_EINVAL, "pt_read_denoised: pt_denoise has not run");
    return read_back(ctx, out, ctx->d_denoised, sizeof(float4) * (size_t)npix);
}
void* pt_device_denoised(pt_context* ctx) { return ctx ? (void*)ctx->d_denoised : nullptr; }

// ---- variance of each pixel's mean luminance (kernel k_variance, pt_denoise.hip; pinned in include/pt_api.h)
static int compute_variance(pt_context* ctx, const char* who) {
    if (!ctx->moments_valid) return fail(ctx, PT_EINVAL, std::string(who) + ": the frame was not rendered with option moments = 1 from its first sample");
    if (ctx->current_sample <= 0) return fail(ctx, PT_EINVAL, std::string(who) + ": the frame has no samples");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    PT_ALLOC(ctx, ctx->d_variance.reserve((size_t)std::max<int64_t>(ctx->npix, 1)));
    PT_HIP(ctx, launch_variance(ctx->d_colors, ctx->adaptive_frame ? ctx->d_adapt_spp : nullptr, ctx->current_sample, ctx->W, ctx->npix,
                                ctx->d_variance, ctx->stream));
    return PT_OK;
}
int pt_read_variance(pt_context* ctx, float* out, int64_t npix) {
    PT_NEED_DEVICE(ctx);
    if (!out || npix != ctx->npix) return fail(ctx, PT_EINVAL, "npix must equal the local pixel count");
    const int rc = compute_variance(ctx, "pt_read_variance");
    if (rc != PT_OK) return rc;
    return read_back(ctx, out, ctx->d_variance, sizeof(float) * (size_t)npix);
}
void* pt_device_variance(pt_context* ctx) {
    if (!ctx || !ctx->has_device) {
        if (ctx) (void)fail(ctx, PT_ENODEVICE, "context was created without a HIP device (host-only); no CPU render path exists");
        return nullptr;
    }
    return compute_variance(ctx, "pt_device_variance") == PT_OK ? (void*)ctx->d_variance : nullptr;
}

// ---- variance-guided a-trous filter (kernel k_atrous_var, pt_denoise.hip; pinned in include/pt_api.h)
void pt_denoise_variance_defaults(pt_denoise_variance_params* p) {
    if (!p) return;
    p->iterations = 2;
    p->sigma_luminance = 4.0f;
    p->sigma_normal = 8.0f;
    p->sigma_depth = 0.05f;
    p->demodulate = 0;
}
// the arguments of the variance-guided filter: "" or what is wrong (pt_denoise_variance, pt_denoise_temporal)
static std::string variance_params_error(const pt_denoise_variance_params* dp) {
    if (!dp) return "params is NULL";
    if (dp->iterations < 1 || dp->iterations > 10) return "iterations must be 1..10";
    if (!(dp->sigma_luminance >= 0.0f) || !(dp->sigma_normal >= 0.0f) || !(dp->sigma_depth >= 0.0f)) return "sigmas must be >= 0 (and not NaN)";
    return "";
}
// what the three entry points of the variance-guided filter check first: the arguments, then that the context is the only rank
static int variance_filter_check(pt_context* ctx, const char* who, const pt_denoise_variance_params* dp) {
    if (!ctx) return PT_EINVAL;
    const std::string why = variance_params_error(dp);
    if (!why.empty()) return fail(ctx, PT_EINVAL, std::string(who) + ": " + why);
    return need_one_rank(ctx, who);
}
// the iterations of k_atrous_var over colour in0 (.xyz) and variance var with the current guides, into the two d_dn buffers
static int atrous_var_iterations(pt_context* ctx, const pt_denoise_variance_params* dp, const float4* in0, const float* var) {
    const size_t npix = (size_t)ctx->npix;
    return atrous_iterations(ctx, dp->iterations, in0, [&](int i, const float4* in, float4* out) {
        AtrousVarStep s;
        s.step = 1 << i;
        s.demodulate = dp->demodulate ? 1 : 0;
        s.lum_on = std::isfinite(dp->sigma_luminance) ? 1 : 0;
        s.normal_on = std::isfinite(dp->sigma_normal) && dp->sigma_normal > 0.0f ? 1 : 0;
        s.depth_on = std::isfinite(dp->sigma_depth) ? 1 : 0;
        s.sigma_luminance = dp->sigma_luminance;
        s.sigma_normal = dp->sigma_normal;
        s.sigma_depth = dp->sigma_depth;
        PT_HIP(ctx, launch_atrous_var(in, var, out, ctx->d_aov, ctx->d_aov + npix, ctx->W, ctx->local_rows, s, i == 0,
                                      i == dp->iterations - 1, ctx->stream));
        return (int)PT_OK;
    });
}
int pt_denoise_variance(pt_context* ctx, const pt_denoise_variance_params* dp) {
    int rc = variance_filter_check(ctx, "pt_denoise_variance", dp);
    if (rc != PT_OK || (rc = need_guides(ctx, "pt_denoise_variance")) != PT_OK) return rc;
    PT_NEED_DEVICE(ctx);
    if ((rc = compute_variance(ctx, "pt_denoise_variance")) != PT_OK) return rc;       // (checks the moments)
    return atrous_var_iterations(ctx, dp, ctx->d_colors, ctx->d_variance);
}

// ---- temporal accumulation with reprojection (kernel k_temporal, pt_temporal.hip; pinned in include/pt_api.h)
void pt_temporal_defaults(pt_temporal_params* p) {
    if (!p) return;
    p->max_history = 64;
    p->normal_cos = 0.9f;
    p->depth_tolerance = 0.02f;
}
// set s of the two history sets: {r, g, b, m2}, {nx, ny, nz, depth}, {n, material} per local pixel
static float4* temporal_colour(const pt_context* ctx, int s) { return ctx->d_temporal + (size_t)s * (size_t)std::max<int64_t>(ctx->npix, 1); }
static float4* temporal_guides(const pt_context* ctx, int s) { return ctx->d_temporal + (size_t)(2 + s) * (size_t)std::max<int64_t>(ctx->npix, 1); }
static float2* temporal_nm(const pt_context* ctx, int s) {
    const size_t np = (size_t)std::max<int64_t>(ctx->npix, 1);
    return reinterpret_cast<float2*>(ctx->d_temporal + 4 * np) + (size_t)s * np;
}
int pt_temporal_accumulate(pt_context* ctx, const pt_temporal_params* tp) {
    if (!ctx) return PT_EINVAL;
    if (!tp) return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: params is NULL");
    if (tp->max_history < 0) return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: max_history must be >= 0");
    if (!(tp->normal_cos >= -1.0f && tp->normal_cos <= 1.0f)) return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: normal_cos must be in [-1, 1]");
    if (!(tp->depth_tolerance >= 0.0f)) return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: depth_tolerance must be >= 0 (and not NaN)");
    int rc = need_one_rank(ctx, "pt_temporal_accumulate");
    if (rc != PT_OK) return rc;
    PT_NEED_DEVICE(ctx);
    if ((rc = need_guides(ctx, "pt_temporal_accumulate")) != PT_OK) return rc;
    if (!ctx->moments_valid)
        return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: the frame was not rendered with option moments = 1 from its first sample");
    if (ctx->current_sample <= 0) return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: the frame has no samples");
    if (!ctx->frame_cam_same) return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: the launches of the frame used different cameras");
    if (std::memcmp(&ctx->aov_cam, &ctx->frame_cam, sizeof(pt_camera)) != 0)
        return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: the guides were rendered with a different camera from the frame");
    if (ctx->temporal_frame == ctx->frame_serial) return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: this frame was already accumulated");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t np = (size_t)std::max<int64_t>(ctx->npix, 1);
    static_assert(4 * sizeof(float4) + 2 * sizeof(float2) == 5 * sizeof(float4), "the two history sets: five float4 per local pixel");
    PT_ALLOC(ctx, ctx->d_temporal.reserve(5 * np));
    PT_ALLOC(ctx, ctx->d_temporal_var.reserve(np));
    const int out = ctx->temporal_out == 0 ? 1 : 0, prev = 1 - out;
    TemporalArgs a;
    a.cur = ctx->frame_cam;
    a.prev = ctx->temporal_cam;
    a.colors = ctx->d_colors;
    a.tile_spp = ctx->adaptive_frame ? ctx->d_adapt_spp : nullptr;
    a.n_all = ctx->current_sample;
    a.albedo = ctx->d_aov;
    a.nd = ctx->d_aov + ctx->npix;
    a.prev_c = temporal_colour(ctx, prev);
    a.prev_g = temporal_guides(ctx, prev);
    a.prev_nm = temporal_nm(ctx, prev);
    a.out_c = temporal_colour(ctx, out);
    a.out_g = temporal_guides(ctx, out);
    a.out_nm = temporal_nm(ctx, out);
    a.out_v = ctx->d_temporal_var;
    a.W = ctx->W;
    a.H = ctx->local_rows;
    a.has_prev = ctx->temporal_history ? 1 : 0;
    a.max_history = (float)tp->max_history;
    a.normal_cos = tp->normal_cos;
    a.depth_tolerance = tp->depth_tolerance;
    PT_HIP(ctx, launch_temporal(a, ctx->stream));
    ctx->temporal_out = out;
    ctx->temporal_history = true;
    ctx->temporal_cam = ctx->frame_cam;
    ctx->temporal_frame = ctx->frame_serial;
    ctx->temporal_aov = ctx->aov_serial;
    return PT_OK;
}
int pt_read_temporal(pt_context* ctx, float* rgbv, float* n, int64_t npix) {
    PT_NEED_DEVICE(ctx);
    if (npix != ctx->npix) return fail(ctx, PT_EINVAL, "npix must equal the local pixel count");
    if (ctx->temporal_out < 0) return fail(ctx, PT_EINVAL, "pt_read_temporal: pt_temporal_accumulate has not run");
    int rc = PT_OK;
    if (rgbv) {
        std::vector<float> v((size_t)npix);
        if ((rc = read_back(ctx, rgbv, temporal_colour(ctx, ctx->temporal_out), sizeof(float4) * (size_t)npix)) != PT_OK) return rc;
        if ((rc = read_back(ctx, v.data(), ctx->d_temporal_var, sizeof(float) * (size_t)npix)) != PT_OK) return rc;
        for (int64_t i = 0; i < npix; ++i) rgbv[4 * i + 3] = v[(size_t)i];
    }
    if (n) {
        std::vector<float2> nm((size_t)npix);
        if ((rc = read_back(ctx, nm.data(), temporal_nm(ctx, ctx->temporal_out), sizeof(float2) * (size_t)npix)) != PT_OK) return rc;
        for (int64_t i = 0; i < npix; ++i) n[i] = nm[(size_t)i].x;
    }
    return PT_OK;
}
void* pt_device_temporal(pt_context* ctx) { return ctx && ctx->temporal_out >= 0 ? (void*)temporal_colour(ctx, ctx->temporal_out) : nullptr; }
int pt_denoise_temporal(pt_context* ctx, const pt_denoise_variance_params* dp) {
    const int rc = variance_filter_check(ctx, "pt_denoise_temporal", dp);
    if (rc != PT_OK) return rc;
    PT_NEED_DEVICE(ctx);
    if (!ctx->aov_valid || ctx->temporal_out < 0 || ctx->temporal_aov != ctx->aov_serial)
        return fail(ctx, PT_EINVAL, "pt_denoise_temporal: pt_temporal_accumulate has not run on the current guides");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    return atrous_var_iterations(ctx, dp, temporal_colour(ctx, ctx->temporal_out), ctx->d_temporal_var);
}

// ---- variance-gated firefly filter (kernel k_despeckle, pt_despeckle.hip; pinned in include/pt_api.h)
void pt_despeckle_defaults(pt_despeckle_params* p) {
    if (!p) return;
    p->source = PT_DESPECKLE_FRAME;
    p->radius = 2;
    p->rank = 2;
    p->threshold = 4.0f;
    p->floor = 0.0f;
    p->min_rel_sigma = 0.5f;
    p->spread = 1;
}
// the arguments of the firefly filter: "" or what is wrong (pt_despeckle, pt_debug_despeckle)
static std::string despeckle_params_error(const pt_despeckle_params* dp) {
    if (!dp) return "params is NULL";
    if (dp->radius < 1 || dp->radius > 3) return "radius must be 1..3";
    if (dp->rank < 1 || dp->rank > 3) return "rank must be 1..3";
    if (!(dp->threshold >= 1.0f)) return "threshold must be >= 1 (and not NaN)";
    if (!(dp->floor >= 0.0f)) return "floor must be >= 0 (and not NaN)";
    if (!(dp->min_rel_sigma >= 0.0f)) return "min_rel_sigma must be >= 0 (and not NaN)";
    if (dp->spread != 0 && dp->spread != 1) return "spread must be 0 or 1";
    if (dp->source != PT_DESPECKLE_FRAME && dp->source != PT_DESPECKLE_TEMPORAL) return "source must be PT_DESPECKLE_FRAME or PT_DESPECKLE_TEMPORAL";
    return "";
}
// the three parts of d_despeckle: {r, g, b, v}, v, flags per local pixel
static float* despeckle_var(const pt_context* ctx) { return reinterpret_cast<float*>(ctx->d_despeckle + (size_t)std::max<int64_t>(ctx->npix, 1)); }
static int32_t* despeckle_flags(const pt_context* ctx) { return reinterpret_cast<int32_t*>(despeckle_var(ctx) + (size_t)std::max<int64_t>(ctx->npix, 1)); }
static void despeckle_args(const pt_despeckle_params* dp, DespeckleArgs* a) {
    a->rank = dp->rank;
    a->threshold = dp->threshold;
    a->floor_ = dp->floor;
    a->min_rel_sigma = dp->min_rel_sigma;
}
int pt_despeckle(pt_context* ctx, const pt_despeckle_params* dp) {
    if (!ctx) return PT_EINVAL;
    const std::string why = despeckle_params_error(dp);
    if (!why.empty()) return fail(ctx, PT_EINVAL, "pt_despeckle: " + why);
    if (const int rc = need_one_rank(ctx, "pt_despeckle"); rc != PT_OK) return rc;
    PT_NEED_DEVICE(ctx);
    DespeckleArgs a;
    if (dp->source == PT_DESPECKLE_TEMPORAL) {
        if (ctx->temporal_out < 0) return fail(ctx, PT_EINVAL, "pt_despeckle: pt_temporal_accumulate has not run");
        PT_HIP(ctx, hipSetDevice(ctx->device));
        a.c = temporal_colour(ctx, ctx->temporal_out);
        a.v = ctx->d_temporal_var;
    } else {
        const int rc = compute_variance(ctx, "pt_despeckle");          // (checks the moments)
        if (rc != PT_OK) return rc;
        a.c = ctx->d_colors;
        a.v = ctx->d_variance;
    }
    const size_t np = (size_t)std::max<int64_t>(ctx->npix, 1);
    static_assert(sizeof(float4) + sizeof(float) + sizeof(int32_t) == 24, "colour + variance, the variance, the flag: 24 B per local pixel");
    PT_ALLOC(ctx, ctx->d_despeckle.reserve((np * 24 + sizeof(float4) - 1) / sizeof(float4)));
    a.out = ctx->d_despeckle;
    a.out_v = despeckle_var(ctx);
    a.flags = despeckle_flags(ctx);
    a.W = ctx->W;
    a.H = ctx->local_rows;
    despeckle_args(dp, &a);
    ctx->despeckle_valid = false;
    PT_HIP(ctx, launch_despeckle(a, dp->radius, dp->spread, ctx->stream));
    ctx->despeckle_valid = true;
    ctx->despeckle_source = dp->source;
    ctx->despeckle_epoch = ctx->render_epoch;
    ctx->despeckle_frame = ctx->frame_serial;
    ctx->despeckle_temporal = ctx->temporal_frame;
    return PT_OK;
}
int pt_read_despeckled(pt_context* ctx, float* rgbv, int32_t* flags, int64_t npix) {
    PT_NEED_DEVICE(ctx);
    if (npix != ctx->npix) return fail(ctx, PT_EINVAL, "npix must equal the local pixel count");
    if (!ctx->d_despeckle) return fail(ctx, PT_EINVAL, "pt_read_despeckled: pt_despeckle has not run");
    int rc = PT_OK;
    if (rgbv && (rc = read_back(ctx, rgbv, ctx->d_despeckle, sizeof(float4) * (size_t)npix)) != PT_OK) return rc;
    if (flags && (rc = read_back(ctx, flags, despeckle_flags(ctx), sizeof(int32_t) * (size_t)npix)) != PT_OK) return rc;
    return PT_OK;
}
void* pt_device_despeckled(pt_context* ctx) { return ctx ? (void*)ctx->d_despeckle.get() : nullptr; }
int pt_denoise_despeckled(pt_context* ctx, const pt_denoise_variance_params* dp) {
    int rc = variance_filter_check(ctx, "pt_denoise_despeckled", dp);
    if (rc != PT_OK) return rc;
    PT_NEED_DEVICE(ctx);
    if ((rc = need_guides(ctx, "pt_denoise_despeckled")) != PT_OK) return rc;
    if (!ctx->d_despeckle || !ctx->despeckle_valid) return fail(ctx, PT_EINVAL, "pt_denoise_despeckled: pt_despeckle has not run on the scene as uploaded");
    if (ctx->despeckle_epoch != ctx->render_epoch || ctx->despeckle_frame != ctx->frame_serial)
        return fail(ctx, PT_EINVAL, "pt_denoise_despeckled: the despeckled result is stale (a launch has written colors since pt_despeckle)");
    if (ctx->despeckle_source == PT_DESPECKLE_TEMPORAL && ctx->despeckle_temporal != ctx->temporal_frame)
        return fail(ctx, PT_EINVAL, "pt_denoise_despeckled: the despeckled result is stale (a newer pt_temporal_accumulate ran)");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    return atrous_var_iterations(ctx, dp, ctx->d_despeckle, despeckle_var(ctx));
}
int pt_debug_despeckle(pt_context* ctx, const float* rgbv_in, int32_t w, int32_t h, const pt_despeckle_params* dp, float* rgbv_out, int32_t* flags) {
    if (!ctx) return PT_EINVAL;
    pt_despeckle_params p = {};
    if (dp) {
        p = *dp;
        p.source = PT_DESPECKLE_FRAME;       // (ignored)
    }
    const std::string why = despeckle_params_error(dp ? &p : nullptr);
    if (!why.empty()) return fail(ctx, PT_EINVAL, "pt_debug_despeckle: " + why);
    if (w < 1 || w > 4096 || h < 1 || h > 4096) return fail(ctx, PT_EINVAL, "pt_debug_despeckle: w and h must be 1..4096");
    if (!rgbv_in || !rgbv_out || !flags) return fail(ctx, PT_EINVAL, "pt_debug_despeckle: NULL argument");
    PT_NEED_DEVICE(ctx);
    const size_t n = (size_t)w * (size_t)h;
    std::vector<float4> out(n + (n + 3) / 4);        // {r, g, b, v} per pixel, then the flags
    const int rc = debug_round_trip(ctx, rgbv_in, sizeof(float4) * n, out.data(), sizeof(float4) * out.size(), [&](void* d_in, void* d_out) {
        DespeckleArgs a;
        a.c = static_cast<const float4*>(d_in);
        a.v = nullptr;
        a.out = static_cast<float4*>(d_out);
        a.out_v = nullptr;
        a.flags = reinterpret_cast<int32_t*>(a.out + n);
        a.W = w;
        a.H = h;
        despeckle_args(&p, &a);
        return launch_despeckle(a, p.radius, p.spread, ctx->stream);
    });
    if (rc != PT_OK) return rc;
    std::memcpy(rgbv_out, out.data(), sizeof(float4) * n);
    std::memcpy(flags, out.data() + n, sizeof(int32_t) * n);
    return PT_OK;
}

// ---- display stage (kernels k_display_*, pt_display.hip; pinned in include/pt_api.h)
void pt_display_defaults(pt_display_params* p) {
    if (!p) return;
    p->source = PT_DISPLAY_FRAME;
    p->metering = PT_METER_AUTO;
    p->ev = 0.0f;
    p->key = 0.18f;
    p->low_permille = 100;
    p->high_permille = 950;
    p->min_ev = -16.0f;
    p->max_ev = 16.0f;
    p->adapt = 1.0f;
    p->bloom_levels = 4;
    p->bloom_threshold = 1.0f;
    p->bloom_intensity = 0.0f;
    p->curve = PT_CURVE_ACES;
    p->white = std::numeric_limits<float>::infinity();
    p->encoding = PT_ENCODE_SRGB;
}
// the arguments of the display stage in the pinned order: "" or what is wrong (pt_display, pt_debug_display)
static std::string display_params_error(const pt_display_params* dp) {
    if (!dp) return "params is NULL";
    if (dp->source < PT_DISPLAY_FRAME || dp->source > PT_DISPLAY_DESPECKLED) return "source must be PT_DISPLAY_FRAME .. PT_DISPLAY_DESPECKLED";
    if (dp->metering != PT_METER_MANUAL && dp->metering != PT_METER_AUTO) return "metering must be PT_METER_MANUAL or PT_METER_AUTO";
    if (dp->curve < PT_CURVE_LINEAR || dp->curve > PT_CURVE_ACES) return "curve must be PT_CURVE_LINEAR, PT_CURVE_REINHARD or PT_CURVE_ACES";
    if (dp->encoding != PT_ENCODE_SRGB && dp->encoding != PT_ENCODE_LINEAR) return "encoding must be PT_ENCODE_SRGB or PT_ENCODE_LINEAR";
    for (float f : {dp->ev, dp->key, dp->min_ev, dp->max_ev, dp->adapt, dp->bloom_threshold, dp->bloom_intensity, dp->white})
        if (std::isnan(f)) return "a parameter is NaN";
    if (!(dp->key > 0.0f)) return "key must be > 0";
    if (dp->low_permille < 0 || dp->low_permille >= dp->high_permille || dp->high_permille > 1000) return "permille must be 0 <= low < high <= 1000";
    if (dp->min_ev > dp->max_ev) return "min_ev must be <= max_ev";
    if (!(dp->adapt > 0.0f && dp->adapt <= 1.0f)) return "adapt must be in (0, 1]";
    if (dp->bloom_levels < 1 || dp->bloom_levels > kDisplayMaxLevels) return "bloom_levels must be 1..6";
    if (dp->bloom_threshold < 0.0f) return "bloom_threshold must be >= 0";
    if (dp->bloom_intensity < 0.0f) return "bloom_intensity must be >= 0";
    if (!(dp->white > 0.0f)) return "white must be > 0";
    return "";
}
static void display_args(const pt_display_params* dp, DisplayArgs* a) {
    a->metering = dp->metering;
    a->ev = dp->ev;
    a->key = dp->key;
    a->low_permille = dp->low_permille;
    a->high_permille = dp->high_permille;
    a->min_ev = dp->min_ev;
    a->max_ev = dp->max_ev;
    a->adapt = dp->adapt;
    a->levels = dp->bloom_intensity > 0.0f ? dp->bloom_levels : 0;
    a->threshold = dp->bloom_threshold;
    a->intensity = dp->bloom_intensity;
    a->curve = dp->curve;
    a->white = dp->white;
    a->encoding = dp->encoding;
}
// the bytes of d_display: right behind the float4 result
static uint8_t* display_bytes(const pt_context* ctx) { return reinterpret_cast<uint8_t*>(ctx->d_display + (size_t)std::max<int64_t>(ctx->npix, 1)); }
static void display_info_from(const DisplayStat& st, int32_t levels, struct pt_display_info* out) {
    out->exposure = st.exposure;
    out->mean_log2 = st.mean_log2;
    out->n_metered = st.n_metered;
    out->n_dark = st.n_dark;
    out->n_nonfinite = st.n_nonfinite;
    out->levels = levels;
}
int pt_display(pt_context* ctx, const pt_display_params* dp) {
    if (!ctx) return PT_EINVAL;
    const std::string why = display_params_error(dp);
    if (!why.empty()) return fail(ctx, PT_EINVAL, "pt_display: " + why);
    if (const int rc = need_one_rank(ctx, "pt_display"); rc != PT_OK) return rc;
    PT_NEED_DEVICE(ctx);
    DisplayArgs a;
    switch (dp->source) {
    case PT_DISPLAY_DENOISED:
        if (!ctx->d_denoised) return fail(ctx, PT_EINVAL, "pt_display: source DENOISED, but pt_denoise has not run");
        a.c = ctx->d_denoised;
        break;
    case PT_DISPLAY_TEMPORAL:
        if (ctx->temporal_out < 0) return fail(ctx, PT_EINVAL, "pt_display: source TEMPORAL, but pt_temporal_accumulate has not run");
        a.c = temporal_colour(ctx, ctx->temporal_out);
        break;
    case PT_DISPLAY_DESPECKLED:
        if (!ctx->d_despeckle) return fail(ctx, PT_EINVAL, "pt_display: source DESPECKLED, but pt_despeckle has not run");
        a.c = ctx->d_despeckle;
        break;
    default: a.c = ctx->d_colors; break;
    }
    PT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t np = (size_t)std::max<int64_t>(ctx->npix, 1);
    display_args(dp, &a);
    PT_ALLOC(ctx, ctx->d_display.reserve(np + (3 * np + sizeof(float4) - 1) / sizeof(float4)));
    PT_ALLOC(ctx, ctx->d_display_stat.reserve(1));
    if (a.levels > 0) PT_ALLOC(ctx, ctx->d_display_pyr.reserve(display_pyramid_elems(ctx->W, ctx->local_rows, a.levels)));
    a.W = ctx->W;
    a.H = ctx->local_rows;
    a.stat = ctx->d_display_stat;
    a.out = ctx->d_display;
    a.rgb8 = display_bytes(ctx);
    a.pyr = ctx->d_display_pyr;
    a.prev_mode = ctx->display_has_prev ? 1 : 0;
    a.prev_value = 0.0f;
    ctx->display_ran = false;
    ctx->display_has_prev = false;
    PT_HIP(ctx, launch_display(a, ctx->stream));
    ctx->display_ran = true;
    ctx->display_has_prev = true;
    ctx->display_levels = a.levels;
    return PT_OK;
}
int pt_read_display(pt_context* ctx, float* rgba, uint8_t* rgb8, int64_t npix) {
    PT_NEED_DEVICE(ctx);
    if (npix != ctx->npix) return fail(ctx, PT_EINVAL, "npix must equal the local pixel count");
    if (!ctx->display_ran) return fail(ctx, PT_EINVAL, "pt_read_display: pt_display has not run");
    int rc = PT_OK;
    if (rgba && (rc = read_back(ctx, rgba, ctx->d_display, sizeof(float4) * (size_t)npix)) != PT_OK) return rc;
    if (rgb8 && (rc = read_back(ctx, rgb8, display_bytes(ctx), 3 * (size_t)npix)) != PT_OK) return rc;
    return PT_OK;
}
void* pt_device_display(pt_context* ctx) { return ctx && ctx->display_ran ? (void*)ctx->d_display.get() : nullptr; }
int pt_display_info(pt_context* ctx, struct pt_display_info* out) {
    PT_NEED_DEVICE(ctx);
    if (!out) return fail(ctx, PT_EINVAL, "pt_display_info: NULL argument");
    if (!ctx->display_ran) return fail(ctx, PT_EINVAL, "pt_display_info: pt_display has not run");
    DisplayStat st;
    const int rc = read_back(ctx, &st, ctx->d_display_stat, sizeof(st));
    if (rc != PT_OK) return rc;
    display_info_from(st, ctx->display_levels, out);
    return PT_OK;
}
int pt_debug_display_histogram(pt_context* ctx, uint32_t out[256]) {
    PT_NEED_DEVICE(ctx);
    if (!out) return fail(ctx, PT_EINVAL, "pt_debug_display_histogram: NULL argument");
    if (!ctx->display_ran) return fail(ctx, PT_EINVAL, "pt_debug_display_histogram: pt_display has not run");
    return read_back(ctx, out, ctx->d_display_stat, sizeof(uint32_t) * 256);
}
int pt_display_reset(pt_context* ctx) {
    if (!ctx) return PT_EINVAL;
    ctx->display_has_prev = false;
    return PT_OK;
}
int pt_write_display_ppm(pt_context* ctx, const char* path) {
    if (!ctx || !path) return PT_EINVAL;
    PT_NEED_DEVICE(ctx);
    if (!ctx->display_ran) return fail(ctx, PT_EINVAL, "pt_write_display_ppm: pt_display has not run");
    std::vector<uint8_t> bytes(3 * (size_t)ctx->npix);
    const int rc = read_back(ctx, bytes.data(), display_bytes(ctx), bytes.size());
    if (rc != PT_OK) return rc;
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(ctx, PT_EIO, std::string("cannot write ") + path);
    std::fprintf(f, "P6\n%d %d\n255\n", ctx->W, ctx->local_rows);      // (the bytes are top row first already)
    bool ok = std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    ok = (std::fclose(f) == 0) && ok;
    return ok ? PT_OK : fail(ctx, PT_EIO, std::string("cannot write ") + path);
}
int pt_debug_display(pt_context* ctx, const float* rgba_in, int32_t w, int32_t h, const pt_display_params* dp, float prev_exposure, float* rgba_out,
                     uint8_t* rgb8_out, uint32_t* hist, struct pt_display_info* info) {
    if (!ctx) return PT_EINVAL;
    pt_display_params p = {};
    if (dp) {
        p = *dp;
        p.source = PT_DISPLAY_FRAME;         // (ignored)
    }
    const std::string why = display_params_error(dp ? &p : nullptr);
    if (!why.empty()) return fail(ctx, PT_EINVAL, "pt_debug_display: " + why);
    if (w < 1 || w > 4096 || h < 1 || h > 4096) return fail(ctx, PT_EINVAL, "pt_debug_display: w and h must be 1..4096");
    if (!rgba_in || std::isnan(prev_exposure)) return fail(ctx, PT_EINVAL, "pt_debug_display: rgba_in is NULL or prev_exposure is NaN");
    PT_NEED_DEVICE(ctx);
    DisplayArgs a;
    display_args(&p, &a);
    // the output allocation, in float4: the result, its bytes, the DisplayStat, the pyramid
    const size_t n = (size_t)w * (size_t)h, nb = (3 * n + sizeof(float4) - 1) / sizeof(float4), ns = sizeof(DisplayStat) / sizeof(float4);
    static_assert(sizeof(DisplayStat) % sizeof(float4) == 0, "the DisplayStat sits between float4 arrays");
    const size_t back = n + nb + ns;          // what comes back to the host
    std::vector<float4> out(back);
    const int rc = debug_round_trip(ctx, rgba_in, sizeof(float4) * n, out.data(), sizeof(float4) * back, [&](void* d_in, void* d_out) {
        DeviceBuf pyr;                       // (freed when the lambda returns, so the lambda waits for the kernels below)
        if (a.levels > 0) {
            const hipError_t e = pyr.alloc(sizeof(float4) * display_pyramid_elems(w, h, a.levels));
            if (e != hipSuccess) return e;
        }
        a.c = static_cast<const float4*>(d_in);
        a.W = w;
        a.H = h;
        a.out = static_cast<float4*>(d_out);
        a.rgb8 = reinterpret_cast<uint8_t*>(a.out + n);
        a.stat = reinterpret_cast<DisplayStat*>(a.out + n + nb);
        a.pyr = static_cast<float4*>(pyr.p);
        a.prev_mode = prev_exposure > 0.0f ? 2 : 0;
        a.prev_value = prev_exposure;
        hipError_t e = launch_display(a, ctx->stream);
        if (e == hipSuccess && a.levels > 0) e = hipStreamSynchronize(ctx->stream);      // the pyramid must outlive the kernels
        return e;
    });
    if (rc != PT_OK) return rc;
    const DisplayStat* st = reinterpret_cast<const DisplayStat*>(out.data() + n + nb);
    if (rgba_out) std::memcpy(rgba_out, out.data(), sizeof(float4) * n);
    if (rgb8_out) std::memcpy(rgb8_out, out.data() + n, 3 * n);
    if (hist) std::memcpy(hist, st->hist, sizeof(uint32_t) * 256);
    if (info) display_info_from(*st, a.levels, info);
    return PT_OK;
}
int pt_debug_reproject(const pt_camera* cur, const pt_camera* prev, int32_t x, int32_t y, float depth, float out[3]) {
    if (!cur || !prev || !out) return fail(nullptr, PT_EINVAL, "pt_debug_reproject: NULL argument");
    if (!(cur->XM >= 1.0f && cur->XM <= 65535.0f && cur->YM >= 1.0f && cur->YM <= 65535.0f) || x < 0 || y < 0 || x >= (int32_t)cur->XM || y >= (int32_t)cur->YM)
        return fail(nullptr, PT_EINVAL, "pt_debug_reproject: (x, y) must lie in cur's frame");
    if (!reproject(*cur, *prev, y * (int32_t)cur->XM + x, depth, out))
        return fail(nullptr, PT_EINVAL, "pt_debug_reproject: the point is not in front of prev (a <= 0)");
    return PT_OK;
}

}  // extern "C"
