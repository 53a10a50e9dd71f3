// pt_env.cpp -- the environment of pt_render_nee (include/pt_api.h pins the map, the distribution and the estimator): validation, the
// sampling tables (host, double precision, stored as float), the device copies, and the host statements of the lookup and the tables.
// The kernel side is pt_nee.hip (the ENV instances of k_nee).
#include "pt_context.hpp"

namespace ptamd {

// P_env as the kernel uses it: u_sel = m 2^-24 (m < 2^24) is below `select` for ceil(select 2^24) values of m
float env_select(const pt_context* ctx, bool no_lights) {
    if (!ctx->env_set || !ctx->env_dist) return 0.0f;
    if (no_lights) return 1.0f;
    return (float)(std::ceil((double)ctx->env_select * 16777216.0) / 16777216.0);
}

static double env_luminance(const float* c) {      // the weights of option "moments"
    return 0.2126 * (double)c[0] + 0.7152 * (double)c[1] + 0.0722 * (double)c[2];
}

}  // namespace ptamd

extern "C" {

void pt_environment_defaults(pt_environment_params* p) {
    if (!p) return;
    p->scale = 1.0f;
    p->yaw_degrees = 0.0f;
    p->select = 0.5f;
}

int pt_set_environment(pt_context* ctx, const float* rgb, int32_t w, int32_t h, const pt_environment_params* params) {
    if (!ctx) return PT_EINVAL;
    pt_environment_params p;
    pt_environment_defaults(&p);
    if (params) p = *params;
    if (!rgb) return fail(ctx, PT_EINVAL, "pt_set_environment: rgb is NULL");
    if (w < 1 || h < 1 || w > PT_ENV_MAX_WIDTH || h > PT_ENV_MAX_HEIGHT)
        return fail(ctx, PT_EINVAL, "pt_set_environment: the map must be 1 x 1 to " + std::to_string(PT_ENV_MAX_WIDTH) + " x " + std::to_string(PT_ENV_MAX_HEIGHT) + " texels");
    if (!(p.select >= 0.0f && p.select <= 1.0f)) return fail(ctx, PT_EINVAL, "pt_set_environment: select must lie in [0, 1]");
    if (!(p.scale >= 0.0f) || !std::isfinite(p.scale)) return fail(ctx, PT_EINVAL, "pt_set_environment: scale must be finite and >= 0");
    if (!std::isfinite(p.yaw_degrees)) return fail(ctx, PT_EINVAL, "pt_set_environment: yaw_degrees must be finite");
    const size_t n = (size_t)w * (size_t)h;
    for (size_t i = 0; i < 3 * n; ++i)
        if (!(rgb[i] >= 0.0f) || !std::isfinite(rgb[i])) return fail(ctx, PT_EINVAL, "pt_set_environment: texel values must be finite and >= 0");

    // weight lum(texel) Omega(row); the common factor 2 pi / w of Omega only enters p_env
    std::vector<double> band((size_t)h), row_w((size_t)h, 0.0);
    for (int32_t r = 0; r < h; ++r) band[(size_t)r] = std::cos(M_PI * r / h) - std::cos(M_PI * (r + 1) / h);
    std::vector<float> row_cdf((size_t)h), col_cdf(n);
    for (int32_t r = 0; r < h; ++r) {
        double sum = 0.0;
        for (int32_t c = 0; c < w; ++c) sum += env_luminance(rgb + 3 * ((size_t)r * w + c));
        double run = 0.0;
        for (int32_t c = 0; c < w; ++c) {
            run += sum > 0.0 ? env_luminance(rgb + 3 * ((size_t)r * w + c)) : 1.0;
            col_cdf[(size_t)r * w + c] = c + 1 == w ? 1.0f : (float)(run / (sum > 0.0 ? sum : (double)w));
        }
        row_w[(size_t)r] = sum * band[(size_t)r];
    }
    double total = 0.0;
    for (double v : row_w) total += v;
    const bool dist = total > 0.0 && std::isfinite(total);
    double run = 0.0;
    for (int32_t r = 0; r < h; ++r) {
        run += dist ? row_w[(size_t)r] : 1.0;
        row_cdf[(size_t)r] = r + 1 == h ? 1.0f : (float)(run / (dist ? total : (double)h));
    }
    // p_env = P(texel) / Omega(row) with P from the stored cdfs' own steps: the distribution that is sampled
    std::vector<float4> texels(n);
    for (int32_t r = 0; r < h; ++r) {
        const double pr = (double)row_cdf[(size_t)r] - (r ? (double)row_cdf[(size_t)r - 1] : 0.0);
        const double omega = 2.0 * M_PI / w * band[(size_t)r];
        for (int32_t c = 0; c < w; ++c) {
            const size_t i = (size_t)r * w + c;
            const double pc = (double)col_cdf[i] - (c ? (double)col_cdf[i - 1] : 0.0);
            texels[i] = make_float4(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], dist ? (float)(pr * pc / omega) : 0.0f);
        }
    }
    // no map is set while the device copies are replaced: a failed upload leaves the context without an environment, never with the
    // old size over new buffers
    ctx->env_set = false;
    ctx->env_dist = false;
    if (ctx->has_device) {
        PT_HIP(ctx, hipSetDevice(ctx->device));
        PT_HIP(ctx, hipStreamSynchronize(ctx->stream));     // a frame in flight may still read the previous map
        int rc;
        if ((rc = upload_vec(ctx, &ctx->d_env_texels, texels.data(), sizeof(float4) * n)) != PT_OK) return rc;
        if ((rc = upload_vec(ctx, &ctx->d_env_row_cdf, row_cdf.data(), sizeof(float) * (size_t)h)) != PT_OK) return rc;
        if ((rc = upload_vec(ctx, &ctx->d_env_col_cdf, col_cdf.data(), sizeof(float) * n)) != PT_OK) return rc;
    }
    ctx->env_texels.swap(texels);
    ctx->env_row_cdf.swap(row_cdf);
    ctx->env_col_cdf.swap(col_cdf);
    ctx->env_w = w;
    ctx->env_h = h;
    ctx->env_scale = p.scale;
    ctx->env_yaw = (float)((double)p.yaw_degrees * M_PI / 180.0);
    ctx->env_select = p.select;
    ctx->env_dist = dist;
    ctx->env_set = true;
    return PT_OK;
}

int pt_clear_environment(pt_context* ctx) {
    if (!ctx) return PT_EINVAL;
    ctx->env_set = false;          // the buffers stay until the next map or pt_destroy
    ctx->env_dist = false;
    return PT_OK;
}

int pt_env_lookup(int32_t w, int32_t h, float yaw_degrees, const float dir[3], int32_t* row, int32_t* col) {
    if (!dir || !row || !col || w < 1 || h < 1 || !std::isfinite(yaw_degrees) || !std::isfinite(dir[0]) || !std::isfinite(dir[1]) || !std::isfinite(dir[2]))
        return fail(nullptr, PT_EINVAL, "pt_env_lookup: NULL or non-finite argument, or an empty map");
    env_texel(w, h, (float)((double)yaw_degrees * M_PI / 180.0), dir[0], dir[1], dir[2], row, col);
    return PT_OK;
}

int pt_debug_environment(pt_context* ctx, int32_t* w, int32_t* h, float* row_cdf, float* col_cdf, float* pdf, int64_t cap, float* P_env) {
    if (!ctx) return PT_EINVAL;
    if (!ctx->env_set) return fail(ctx, PT_EINVAL, "pt_debug_environment: no environment is set");
    if (cap < 0) return fail(ctx, PT_EINVAL, "pt_debug_environment: cap < 0");
    if (w) *w = ctx->env_w;
    if (h) *h = ctx->env_h;
    const size_t n = (size_t)std::min<int64_t>(cap, (int64_t)ctx->env_w * ctx->env_h), nr = (size_t)std::min<int64_t>(cap, ctx->env_h);
    for (size_t i = 0; i < nr && row_cdf; ++i) row_cdf[i] = ctx->env_row_cdf[i];
    for (size_t i = 0; i < n; ++i) {
        if (col_cdf) col_cdf[i] = ctx->env_col_cdf[i];
        if (pdf) pdf[i] = ctx->env_texels[i].w;
    }
    if (P_env) {
        bool no_lights = true;
        if (ctx->tris_uploaded && ctx->mats_uploaded) {
            const int rc = light_table_ready(ctx);
            if (rc != PT_OK) return rc;
            no_lights = ctx->nee_tri.empty();
        }
        *P_env = env_select(ctx, no_lights);
    }
    return PT_OK;
}

}  // extern "C"
