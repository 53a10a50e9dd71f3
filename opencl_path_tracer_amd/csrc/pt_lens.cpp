// pt_lens.cpp -- the thin lens, host side: pt_set_lens / pt_clear_lens, pt_focus_at and pt_debug_lens.
#include "pt_context.hpp"

extern "C" {

// ---- thin lens (pt_set_lens; kernels: pt_lens.hip, pt_nee.hip; pinned in include/pt_api.h)
void pt_lens_defaults(pt_lens_params* p) {
    if (!p) return;
    p->aperture = 0.0f;
    p->focus_distance = 1.0f;
    p->_pad[0] = p->_pad[1] = 0.0f;
}

static std::string lens_check(const pt_lens_params* p) {
    if (!p) return "params is NULL";
    if (!(p->aperture >= 0.0f && std::isfinite(p->aperture))) return "aperture must be >= 0 and finite";
    if (!(p->focus_distance > 0.0f && std::isfinite(p->focus_distance))) return "focus_distance must be > 0 and finite";
    return "";
}

int pt_set_lens(pt_context* ctx, const pt_lens_params* p) {
    if (!ctx) return PT_EINVAL;
    const std::string why = lens_check(p);
    if (!why.empty()) return fail(ctx, PT_EINVAL, "pt_set_lens: " + why);
    ctx->lens_set = true;
    ctx->lens_aperture = p->aperture;
    ctx->lens_focus = p->focus_distance;
    return PT_OK;
}

int pt_clear_lens(pt_context* ctx) {
    if (!ctx) return PT_EINVAL;
    ctx->lens_set = false;
    ctx->lens_aperture = 0.0f;
    ctx->lens_focus = 1.0f;
    return PT_OK;
}

int pt_focus_at(pt_context* ctx, const pt_camera* cam, int32_t x, int32_t y, float* distance) {
    PT_NEED_DEVICE(ctx);
    if (!distance) return fail(ctx, PT_EINVAL, "pt_focus_at: distance is NULL");
    int rc = check_ready(ctx, cam);
    if (rc != PT_OK) return rc;
    if (x < 0 || x >= ctx->W || y < 0 || y >= ctx->H) return fail(ctx, PT_EINVAL, "pt_focus_at: (x, y) must be a pixel of the frame");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    RenderParams p;
    fill_params(ctx, cam, &p);
    DeviceBuf d_out;
    PT_HIP(ctx, d_out.alloc(sizeof(float)));
    PT_HIP(ctx, launch_focus_at(p, lens_view(*cam, 0.0f, 1.0f), y * ctx->W + x, (float*)d_out.p, ctx->cu_count, ctx->stream));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP(ctx, hipMemcpy(distance, d_out.p, sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_debug_lens(pt_context* ctx, const pt_camera* cam, const pt_lens_params* lens, int64_t n, const int32_t* gid_state, float* out) {
    PT_NEED_DEVICE(ctx);
    if (!cam || n < 0 || (n > 0 && (!gid_state || !out))) return fail(ctx, PT_EINVAL, "pt_debug_lens: camera non-null, n >= 0, both arrays non-null");
    const std::string why = lens_check(lens);
    if (!why.empty()) return fail(ctx, PT_EINVAL, "pt_debug_lens: " + why);
    if (!((int32_t)cam->XM > 0 && (int32_t)cam->YM > 0)) return fail(ctx, PT_EINVAL, "pt_debug_lens: camera XM/YM must be positive");
    if (n == 0) return PT_OK;
    return debug_round_trip(ctx, gid_state, sizeof(int32_t) * 2 * (size_t)n, out, sizeof(float) * 6 * (size_t)n, [&](void* d_in, void* d_out) {
        return launch_debug_lens(*cam, lens_view(*cam, lens->aperture, lens->focus_distance), (const int32_t*)d_in, n, (float*)d_out, ctx->stream);
    });
}

}  // extern "C"
