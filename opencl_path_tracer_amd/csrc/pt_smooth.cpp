// pt_smooth.cpp -- smooth shading from vertex normals, host side: the authoring calls (pt_set_vertex_normals, pt_clear_vertex_normals,
// pt_compute_vertex_normals), the packed normals on the device for a smooth launch (smooth_prepare) and pt_debug_shading_normal.
#include "pt_context.hpp"

extern "C" {

// ---- smooth shading from vertex normals (kernels: pt_smooth.hip, pt_nee.hip; pinned in include/pt_api.h)
static bool vn_has(const float* n) {
    for (int c = 0; c < 3; ++c) {
        const float* v = n + 3 * c;
        if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2])) return false;
        if (v[0] == 0.0f && v[1] == 0.0f && v[2] == 0.0f) return false;
    }
    return true;
}

int pt_set_vertex_normals(pt_context* ctx, int64_t first, int64_t count, const float* normals) {
    if (!ctx) return PT_EINVAL;
    if (first < 0 || count < 0 || (count > 0 && !normals) || first + count > (int64_t)ctx->tris.size())
        return fail(ctx, PT_EINVAL, "pt_set_vertex_normals: [first_triangle, first_triangle + count) must lie inside the triangles added so far");
    if (count == 0) return PT_OK;
    if (ctx->vnormals.size() < (size_t)(first + count) * 9) ctx->vnormals.resize((size_t)(first + count) * 9, 0.0f);
    std::memcpy(ctx->vnormals.data() + (size_t)first * 9, normals, sizeof(float) * 9 * (size_t)count);
    ctx->vnormals_dirty = true;
    post_shading_inputs_changed(ctx);
    return PT_OK;
}

int pt_clear_vertex_normals(pt_context* ctx) {
    if (!ctx) return PT_EINVAL;
    ctx->vnormals.clear();
    ctx->vnormals_dirty = true;
    post_shading_inputs_changed(ctx);
    return PT_OK;
}

int pt_debug_vertex_normals(const pt_context* ctx, float* normals, int32_t* has) {
    if (!ctx) return PT_EINVAL;
    const size_t n = ctx->tris.size(), have = std::min(n, ctx->vnormals.size() / 9);
    for (size_t i = 0; i < n; ++i) {
        const bool h = i < have && vn_has(ctx->vnormals.data() + 9 * i);
        if (has) has[i] = h ? 1 : 0;
        if (normals)
            for (int c = 0; c < 9; ++c) normals[9 * i + c] = i < have ? ctx->vnormals[9 * i + c] : 0.0f;
    }
    return PT_OK;
}

int pt_compute_vertex_normals(pt_context* ctx, int32_t object, float crease_degrees) {
    if (!ctx) return PT_EINVAL;
    const int32_t nobj = (int32_t)ctx->obj_begin.size();
    if (!(crease_degrees >= 0.0f && crease_degrees <= 180.0f)) return fail(ctx, PT_EINVAL, "pt_compute_vertex_normals: crease_degrees must lie in [0, 180]");
    if (object < -1 || object >= nobj) return fail(ctx, PT_EINVAL, "pt_compute_vertex_normals: object must be -1 (all) or the index of a closed object");
    const double cos_crease = std::cos((double)crease_degrees * 3.14159265358979323846 / 180.0) - 1e-12;
    struct Corner { uint32_t key[3]; int32_t tri, c; };
    auto key_of = [](float f) { uint32_t u; if (f == 0.0f) f = 0.0f * 0.0f; std::memcpy(&u, &f, 4); return u; };      // +0 == -0
    for (int32_t o = object < 0 ? 0 : object; o < (object < 0 ? nobj : object + 1); ++o) {
        const size_t b = (size_t)ctx->obj_begin[(size_t)o], e = o + 1 < nobj ? (size_t)ctx->obj_begin[(size_t)o + 1] : (size_t)ctx->tri_shift;
        if (e <= b) continue;
        const size_t m = e - b;
        std::vector<double> fn(m * 3), ang(m * 3);
        std::vector<char> good(m);
        std::vector<Corner> corners(m * 3);
        for (size_t i = 0; i < m; ++i) {
            const pt_triangle& t = ctx->tris[b + i];
            const double N[3] = {t.N.s[0], t.N.s[1], t.N.s[2]};
            const double l = std::sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
            good[i] = std::isfinite(l) && l > 0.0;
            for (int a = 0; a < 3; ++a) fn[3 * i + a] = good[i] ? N[a] / l : 0.0;
            const float* r[3] = {t.r1.s, t.r2.s, t.r3.s};
            for (int c = 0; c < 3; ++c) {
                const float *p0 = r[c], *p1 = r[(c + 1) % 3], *p2 = r[(c + 2) % 3];
                double u[3], v[3], uu = 0.0, vv = 0.0, uv = 0.0;
                for (int a = 0; a < 3; ++a) {
                    u[a] = (double)p1[a] - p0[a];
                    v[a] = (double)p2[a] - p0[a];
                    uu += u[a] * u[a]; vv += v[a] * v[a]; uv += u[a] * v[a];
                }
                const double den = std::sqrt(uu * vv);
                ang[3 * i + c] = den > 0.0 ? std::acos(std::min(1.0, std::max(-1.0, uv / den))) : 0.0;
                corners[3 * i + c] = Corner{{key_of(p0[0]), key_of(p0[1]), key_of(p0[2])}, (int32_t)i, c};
            }
        }
        // corners at the same position, each group in add order (triangle, then corner)
        std::sort(corners.begin(), corners.end(), [](const Corner& x, const Corner& y) {
            if (x.key[0] != y.key[0]) return x.key[0] < y.key[0];
            if (x.key[1] != y.key[1]) return x.key[1] < y.key[1];
            if (x.key[2] != y.key[2]) return x.key[2] < y.key[2];
            return x.tri != y.tri ? x.tri < y.tri : x.c < y.c;
        });
        if (ctx->vnormals.size() < e * 9) ctx->vnormals.resize(e * 9, 0.0f);
        for (size_t g0 = 0; g0 < corners.size();) {
            size_t g1 = g0 + 1;
            while (g1 < corners.size() && std::memcmp(corners[g1].key, corners[g0].key, sizeof corners[g0].key) == 0) ++g1;
            for (size_t k = g0; k < g1; ++k) {
                const Corner& me = corners[k];
                float* out = ctx->vnormals.data() + (b + (size_t)me.tri) * 9 + 3 * (size_t)me.c;
                out[0] = out[1] = out[2] = 0.0f;
                if (!good[(size_t)me.tri]) continue;
                const double* mine = &fn[3 * (size_t)me.tri];
                double acc[3] = {0.0, 0.0, 0.0};
                for (size_t j = g0; j < g1; ++j) {
                    const Corner& ot = corners[j];
                    if (!good[(size_t)ot.tri]) continue;
                    const double* theirs = &fn[3 * (size_t)ot.tri];
                    const double d = mine[0] * theirs[0] + mine[1] * theirs[1] + mine[2] * theirs[2];
                    if (ot.tri != me.tri && !(d >= cos_crease)) continue;
                    const double w = ang[3 * (size_t)ot.tri + (size_t)ot.c];
                    for (int a = 0; a < 3; ++a) acc[a] += w * theirs[a];
                }
                double l = std::sqrt(acc[0] * acc[0] + acc[1] * acc[1] + acc[2] * acc[2]);
                if (!(l > 0.0)) { acc[0] = mine[0]; acc[1] = mine[1]; acc[2] = mine[2]; l = 1.0; }      // (a degenerate corner: the face normal)
                for (int a = 0; a < 3; ++a) out[a] = (float)(acc[a] / l);
            }
            g0 = g1;
        }
        // a triangle with a corner that got nothing has none
        for (size_t i = 0; i < m; ++i)
            if (!good[i]) std::fill_n(ctx->vnormals.data() + (b + i) * 9, 9, 0.0f);
    }
    ctx->vnormals_dirty = true;
    post_shading_inputs_changed(ctx);
    return PT_OK;
}
}  // extern "C"
namespace ptamd {
int smooth_prepare(pt_context* ctx, const float4** vn, bool force) {
    *vn = nullptr;
    if (!ctx->smooth_normals && !force) return PT_OK;
    PT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = ctx->orig.size();
    if (ctx->vnormals_dirty || !ctx->d_vnormals) {
        PT_ALLOC(ctx, ctx->d_vnormals.reserve(3 * std::max<size_t>(n, 1)));
        // (an empty scene keeps one all-zero record next to its one all-zero packet, which can never be hit)
        if (n == 0) PT_HIP(ctx, hipMemsetAsync(ctx->d_vnormals, 0, sizeof(float4) * 3, ctx->stream));
        const size_t n_src = std::min(ctx->tris.size(), ctx->vnormals.size() / 9);
        DeviceBuf d_src, d_orig;
        hipError_t e = d_src.alloc(sizeof(float) * 9 * n_src);
        if (e == hipSuccess) e = d_orig.alloc(sizeof(int32_t) * n);
        if (e == hipSuccess && n_src) e = hipMemcpyAsync(d_src.p, ctx->vnormals.data(), sizeof(float) * 9 * n_src, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && n) e = hipMemcpyAsync(d_orig.p, ctx->orig.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = launch_pack_vertex_normals((const float*)d_src.p, (int64_t)n_src, (const int32_t*)d_orig.p, (int32_t)n, ctx->d_vnormals, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // the staging copies end with this block, the host vectors may change
        if (e != hipSuccess) return fail(ctx, PT_EHIP, std::string("vertex normals: ") + hipGetErrorString(e));
        ctx->vnormals_dirty = false;
    }
    *vn = ctx->d_vnormals;
    return PT_OK;
}
}  // namespace ptamd
extern "C" {
int pt_debug_shading_normal(pt_context* ctx, const pt_ray* rays, int64_t n, int32_t* out_tri, float* out_ns) {
    PT_NEED_DEVICE(ctx);
    if (!rays || !out_tri || !out_ns || n < 0) return fail(ctx, PT_EINVAL, "bad arguments");
    if (!ctx->tris_uploaded) return fail(ctx, PT_EINVAL, "pt_upload_triangles has not been called");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    const float4* vn = nullptr;
    const int rc = smooth_prepare(ctx, &vn, true);      // (the packed normals are built whatever the option says)
    if (rc != PT_OK) return rc;
    pt_camera cam;
    std::memset(&cam, 0, sizeof cam);
    RenderParams p;
    fill_params(ctx, &cam, &p);
    DeviceBuf d_rays, d_tri, d_ns;
    PT_HIP(ctx, d_rays.alloc(sizeof(pt_ray) * (size_t)n));
    PT_HIP(ctx, d_tri.alloc(sizeof(int32_t) * (size_t)n));
    PT_HIP(ctx, d_ns.alloc(sizeof(float4) * (size_t)n));
    if (n) PT_HIP(ctx, hipMemcpy(d_rays.p, rays, sizeof(pt_ray) * (size_t)n, hipMemcpyHostToDevice));
    PT_HIP(ctx, launch_debug_shading_normal(p, vn, (const pt_ray*)d_rays.p, n, (int32_t*)d_tri.p, (float4*)d_ns.p, ctx->cu_count, ctx->stream));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n) {
        PT_HIP(ctx, hipMemcpy(out_tri, d_tri.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
        PT_HIP(ctx, hipMemcpy(out_ns, d_ns.p, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost));
    }
    for (int64_t i = 0; i < n; ++i)
        if (out_tri[i] >= 0) out_tri[i] = ctx->orig[(size_t)out_tri[i]];      // packed -> add order
    return PT_OK;
}

}  // extern "C"
