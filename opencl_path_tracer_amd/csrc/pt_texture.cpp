// pt_texture.cpp -- albedo textures with UV coordinates, host side: the authoring calls (pt_add_texture, pt_set_material_texture,
// pt_set_vertex_uvs and their clears), the textures, bindings and packed uvs on the device for a textured launch (texture_prepare),
// pt_debug_texture and pt_debug_albedo.
#include "pt_context.hpp"

extern "C" {

// ---- albedo textures with UV coordinates (kernels: pt_texture.hip, pt_nee.hip; pinned in include/pt_api.h)
// a float in [0, 65504] as an IEEE half, round to nearest even
static uint16_t float_to_half(float f) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint32_t e = (x >> 23) & 0xffu;
    if (e >= 113) {                                      // a normal half
        const uint32_t m = x & 0x7fffffu, rem = m & 0x1fffu;
        uint32_t h = ((e - 112) << 10) | (m >> 13);
        if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;      // (a carry moves into the exponent as it should)
        return (uint16_t)h;
    }
    if (e < 102) return 0;                               // below 2^-25: zero
    const uint32_t m = (x & 0x7fffffu) | 0x800000u;      // a subnormal half: m 2^(e - 150) in units of 2^-24
    const uint32_t shift = 126 - e, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    uint32_t h = m >> shift;
    if (rem > half || (rem == half && (h & 1u))) ++h;
    return (uint16_t)h;
}
static float half_to_float(uint16_t h) {                // no sign, no inf / NaN: what float_to_half produces
    const uint32_t e = h >> 10, m = h & 0x3ffu;
    return e ? std::ldexp((float)(m | 0x400u), (int)e - 25) : std::ldexp((float)m, -24);
}

void pt_texture_defaults(pt_texture_params* p) {
    if (!p) return;
    p->filter = 1;
    p->srgb = 0;
}

int pt_add_texture(pt_context* ctx, const float* rgb, int32_t w, int32_t h, const pt_texture_params* tp) {
    if (!ctx) return PT_EINVAL;
    pt_texture_params p;
    pt_texture_defaults(&p);
    if (tp) p = *tp;
    if (!rgb || w < 1 || h < 1 || w > PT_TEX_MAX_SIZE || h > PT_TEX_MAX_SIZE)
        return fail(ctx, PT_EINVAL, "pt_add_texture: width and height must lie in [1, 8192]");
    if (ctx->tex_desc.size() >= (size_t)PT_TEX_MAX_COUNT) return fail(ctx, PT_EINVAL, "pt_add_texture: more than 1024 textures");
    if ((p.filter != 0 && p.filter != 1) || (p.srgb != 0 && p.srgb != 1)) return fail(ctx, PT_EINVAL, "pt_add_texture: filter and srgb must be 0 or 1");
    const size_t n = (size_t)w * (size_t)h, first = ctx->tex_texels.size();
    if (first + n > 0x7fffffffull) return fail(ctx, PT_EINVAL, "pt_add_texture: more than 2^31 - 1 texels over all textures");
    std::vector<uint64_t> tex(n);
    for (size_t i = 0; i < n; ++i) {
        uint64_t q = 0;
        for (int c = 0; c < 3; ++c) {
            float v = rgb[3 * i + c];
            if (!(std::isfinite(v) && v >= 0.0f && v <= 65504.0f)) return fail(ctx, PT_EINVAL, "pt_add_texture: a texel is not finite, negative or above 65504");
            if (p.srgb) {
                const double d = (double)v;
                v = (float)(d <= 0.04045 ? d / 12.92 : std::pow((d + 0.055) / 1.055, 2.4));
                if (!(v <= 65504.0f)) return fail(ctx, PT_EINVAL, "pt_add_texture: a texel is above 65504 after the sRGB transfer function");
            }
            q |= (uint64_t)float_to_half(v) << (16 * c);
        }
        tex[i] = q;
    }
    ctx->tex_texels.insert(ctx->tex_texels.end(), tex.begin(), tex.end());
    ctx->tex_desc.push_back(TexDesc{(uint32_t)first, w, h, p.filter});
    ctx->tex_dirty = true;
    post_shading_inputs_changed(ctx);
    return (int)ctx->tex_desc.size() - 1;
}

int pt_clear_textures(pt_context* ctx) {
    if (!ctx) return PT_EINVAL;
    ctx->tex_texels.clear();
    ctx->tex_desc.clear();
    ctx->mat_tex.clear();
    ctx->tex_dirty = true;
    post_shading_inputs_changed(ctx);
    return PT_OK;
}

int pt_set_material_texture(pt_context* ctx, int32_t material, int32_t texture) {
    if (!ctx) return PT_EINVAL;
    if (material < 0 || (size_t)material >= ctx->mats.size()) return fail(ctx, PT_EINVAL, "pt_set_material_texture: material must be the index of a material added so far");
    if (texture < -1 || texture >= (int32_t)ctx->tex_desc.size()) return fail(ctx, PT_EINVAL, "pt_set_material_texture: texture must be -1 (none) or the index of a texture added so far");
    if (ctx->mat_tex.size() <= (size_t)material) ctx->mat_tex.resize((size_t)material + 1, -1);
    ctx->mat_tex[(size_t)material] = texture;
    ctx->tex_dirty = true;
    post_shading_inputs_changed(ctx);
    return PT_OK;
}

int pt_debug_texture(const pt_context* ctx, int32_t texture, float* rgb, int64_t cap, int32_t* w, int32_t* h, int32_t* filter) {
    if (!ctx || texture < 0 || (size_t)texture >= ctx->tex_desc.size() || cap < 0) return PT_EINVAL;
    const TexDesc& d = ctx->tex_desc[(size_t)texture];
    if (w) *w = d.w;
    if (h) *h = d.h;
    if (filter) *filter = d.filter;
    if (!rgb) return PT_OK;
    const size_t n = (size_t)d.w * (size_t)d.h;
    if ((uint64_t)cap < n) return PT_EINVAL;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t q = ctx->tex_texels[d.first + i];
        for (int c = 0; c < 3; ++c) rgb[3 * i + c] = half_to_float((uint16_t)(q >> (16 * c)));
    }
    return PT_OK;
}

static bool uv_has(const float* uv) {
    for (int c = 0; c < 6; ++c)
        if (!(std::fabs(uv[c]) <= 65536.0f)) return false;      // (false for NaN and inf)
    return true;
}

int pt_set_vertex_uvs(pt_context* ctx, int64_t first, int64_t count, const float* uvs) {
    if (!ctx) return PT_EINVAL;
    if (first < 0 || count < 0 || (count > 0 && !uvs) || first + count > (int64_t)ctx->tris.size())
        return fail(ctx, PT_EINVAL, "pt_set_vertex_uvs: [first_triangle, first_triangle + count) must lie inside the triangles added so far");
    if (count == 0) return PT_OK;
    if (ctx->vuvs.size() < (size_t)(first + count) * 6) ctx->vuvs.resize((size_t)(first + count) * 6, std::numeric_limits<float>::quiet_NaN());
    std::memcpy(ctx->vuvs.data() + (size_t)first * 6, uvs, sizeof(float) * 6 * (size_t)count);
    ctx->vuvs_dirty = true;
    post_shading_inputs_changed(ctx);
    return PT_OK;
}

int pt_clear_vertex_uvs(pt_context* ctx) {
    if (!ctx) return PT_EINVAL;
    ctx->vuvs.clear();
    ctx->vuvs_dirty = true;
    post_shading_inputs_changed(ctx);
    return PT_OK;
}

int pt_debug_vertex_uvs(const pt_context* ctx, float* uvs, int32_t* has) {
    if (!ctx) return PT_EINVAL;
    const size_t n = ctx->tris.size(), have = std::min(n, ctx->vuvs.size() / 6);
    for (size_t i = 0; i < n; ++i) {
        const bool h = i < have && uv_has(ctx->vuvs.data() + 6 * i);
        if (has) has[i] = h ? 1 : 0;
        if (uvs)
            for (int c = 0; c < 6; ++c) uvs[6 * i + c] = h ? ctx->vuvs[6 * i + c] : 0.0f;
    }
    return PT_OK;
}
}  // extern "C"
namespace ptamd {
int texture_prepare(pt_context* ctx, TexView* tv, bool force) {
    *tv = TexView{nullptr, nullptr, nullptr, nullptr};
    if (!ctx->textures && !force) return PT_OK;
    PT_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->tex_dirty || !ctx->d_mat_tex) {
        // (every array keeps one readable record; a binding is -1 wherever the material on the device is not of type 0 or 5; only the
        // coated instances and the shaded guides under option coated look a type-5 binding up)
        const size_t nmat = std::max<size_t>((size_t)ctx->mats_on_device, 1), ntex = std::max<size_t>(ctx->tex_desc.size(), 1),
                     ntexel = std::max<size_t>(ctx->tex_texels.size(), 1);
        std::vector<int32_t> bind(nmat, -1);
        for (size_t i = 0; i < std::min<size_t>({(size_t)ctx->mats_on_device, ctx->mat_tex.size(), ctx->mats.size()}); ++i)
            if ((ctx->mats[i].type == 0 || ctx->mats[i].type == 5) && ctx->mat_tex[i] >= 0 && ctx->mat_tex[i] < (int32_t)ctx->tex_desc.size()) bind[i] = ctx->mat_tex[i];
        std::vector<TexDesc> desc(ctx->tex_desc);
        desc.resize(ntex, TexDesc{0, 1, 1, 0});
        ctx->d_mat_tex.reset();
        ctx->d_tex_desc.reset();
        ctx->d_tex_texels.reset();
        static_assert(sizeof(uint2) == sizeof(uint64_t), "a texel is 8 bytes");
        PT_ALLOC(ctx, ctx->d_tex_texels.replace(ntexel));
        PT_ALLOC(ctx, ctx->d_tex_desc.replace(ntex));
        PT_ALLOC(ctx, ctx->d_mat_tex.replace(nmat));
        if (ctx->tex_texels.empty()) PT_HIP(ctx, hipMemsetAsync(ctx->d_tex_texels, 0, sizeof(uint64_t), ctx->stream));
        else PT_HIP(ctx, hipMemcpyAsync(ctx->d_tex_texels, ctx->tex_texels.data(), sizeof(uint64_t) * ctx->tex_texels.size(), hipMemcpyHostToDevice, ctx->stream));
        PT_HIP(ctx, hipMemcpyAsync(ctx->d_tex_desc, desc.data(), sizeof(TexDesc) * ntex, hipMemcpyHostToDevice, ctx->stream));
        PT_HIP(ctx, hipMemcpyAsync(ctx->d_mat_tex, bind.data(), sizeof(int32_t) * nmat, hipMemcpyHostToDevice, ctx->stream));
        PT_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the staging vectors end here, the host vectors may change
        ctx->tex_dirty = false;
    }
    const size_t n = ctx->orig.size();
    if (ctx->vuvs_dirty || !ctx->d_vuvs) {
        PT_ALLOC(ctx, ctx->d_vuvs.reserve(2 * std::max<size_t>(n, 1)));
        // (an empty scene keeps one all-zero record next to its one all-zero packet, which can never be hit)
        if (n == 0) PT_HIP(ctx, hipMemsetAsync(ctx->d_vuvs, 0, sizeof(float4) * 2, ctx->stream));
        const size_t n_src = std::min(ctx->tris.size(), ctx->vuvs.size() / 6);
        DeviceBuf d_src, d_orig;
        hipError_t e = d_src.alloc(sizeof(float) * 6 * n_src);
        if (e == hipSuccess) e = d_orig.alloc(sizeof(int32_t) * n);
        if (e == hipSuccess && n_src) e = hipMemcpyAsync(d_src.p, ctx->vuvs.data(), sizeof(float) * 6 * n_src, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && n) e = hipMemcpyAsync(d_orig.p, ctx->orig.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = launch_pack_vertex_uvs((const float*)d_src.p, (int64_t)n_src, (const int32_t*)d_orig.p, (int32_t)n, ctx->d_vuvs, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // the staging copies end with this block, the host vectors may change
        if (e != hipSuccess) return fail(ctx, PT_EHIP, std::string("vertex uvs: ") + hipGetErrorString(e));
        ctx->vuvs_dirty = false;
    }
    *tv = TexView{ctx->d_vuvs, ctx->d_tex_texels, ctx->d_tex_desc, ctx->d_mat_tex};
    return PT_OK;
}
}  // namespace ptamd
extern "C" {
int pt_debug_albedo(pt_context* ctx, const pt_ray* rays, int64_t n, int32_t* out_tri, float* out_rgbt) {
    PT_NEED_DEVICE(ctx);
    if (!rays || !out_tri || !out_rgbt || n < 0) return fail(ctx, PT_EINVAL, "bad arguments");
    if (!ctx->tris_uploaded || !ctx->mats_uploaded) return fail(ctx, PT_EINVAL, "pt_upload_triangles / pt_upload_materials have not been called");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    const float4* vn = nullptr;
    int rc = smooth_prepare(ctx, &vn);                   // (the normals only when the option asks for them: they do not change the albedo)
    if (rc != PT_OK) return rc;
    TexView tv;
    if ((rc = texture_prepare(ctx, &tv, true)) != PT_OK) return rc;      // (the textures whatever the option says)
    pt_camera cam;
    std::memset(&cam, 0, sizeof cam);
    RenderParams p;
    fill_params(ctx, &cam, &p);
    DeviceBuf d_rays, d_tri, d_out;
    PT_HIP(ctx, d_rays.alloc(sizeof(pt_ray) * (size_t)n));
    PT_HIP(ctx, d_tri.alloc(sizeof(int32_t) * (size_t)n));
    PT_HIP(ctx, d_out.alloc(sizeof(float4) * (size_t)n));
    if (n) PT_HIP(ctx, hipMemcpy(d_rays.p, rays, sizeof(pt_ray) * (size_t)n, hipMemcpyHostToDevice));
    PT_HIP(ctx, launch_debug_albedo(p, vn, tv, (const pt_ray*)d_rays.p, n, (int32_t*)d_tri.p, (float4*)d_out.p, ctx->cu_count, ctx->stream));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n) {
        PT_HIP(ctx, hipMemcpy(out_tri, d_tri.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
        PT_HIP(ctx, hipMemcpy(out_rgbt, d_out.p, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost));
    }
    for (int64_t i = 0; i < n; ++i)
        if (out_tri[i] >= 0) out_tri[i] = ctx->orig[(size_t)out_tri[i]];      // packed -> add order
    return PT_OK;
}

}  // extern "C"
