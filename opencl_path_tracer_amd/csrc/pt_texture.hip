// pt_texture.hip -- albedo textures with UV coordinates (option textures; include/pt_api.h pins the lookup).
//   k_pack_vertex_uvs   one thread per packed triangle, run on the context's stream in front of the first textured launch after the
//                       recorded uvs or the uploaded triangles changed (texture_prepare, pt_host.cpp): gathers the add-order uvs through
//                       the permutation `orig` into two float4 per packed triangle, {u1, v1, u2, v2} and {u3, v3, flag, 0}; flag != 0 iff
//                       all six values are finite and at most 65536 in magnitude (a triangle past the recorded ones has none).
//   k_debug_albedo      pt_debug_albedo: closest hit of a ray, then shading_normal_albedo() (pt_device.hpp), the function the textured
//                       k_nee instances call (pt_nee.hip), so the lookup can be tested without a render.
#include "pt_device.hpp"

namespace ptamd {

__global__ void __launch_bounds__(256) k_pack_vertex_uvs(const float* __restrict__ src, long long n_src, const int* __restrict__ orig, int n, float4* __restrict__ out) {
    const int ti = blockIdx.x * blockDim.x + threadIdx.x;
    if (ti >= n) return;
    const long long o = orig[ti];
    float4 qa = make_float4(0.f, 0.f, 0.f, 0.f), qb = qa;
    if (o >= 0 && o < n_src) {
        float uv[6];
        bool has = true;
        for (int c = 0; c < 6; ++c) {
            uv[c] = src[o * 6 + c];
            has = has && __builtin_fabsf(uv[c]) <= 65536.0f;      // (false for NaN and inf)
        }
        if (has) {
            qa = make_float4(uv[0], uv[1], uv[2], uv[3]);
            qb = make_float4(uv[4], uv[5], 1.0f, 0.0f);
        }
    }
    out[(size_t)ti * 2] = qa;
    out[(size_t)ti * 2 + 1] = qb;
}

hipError_t launch_pack_vertex_uvs(const float* src, int64_t n_src, const int32_t* orig, int32_t n, float4* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pack_vertex_uvs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, (long long)n_src, orig, (int)n, out);
    return hipGetLastError();
}

// persistent blocks, grid-stride over the rays; one ray per lane at a time (as k_debug_shading_normal)
template <int MODE, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_debug_albedo(RenderParams p, const float4* vn, TexView tv, const pt_ray* rays, long long n, int* out_tri, float4* out_rgbt) {
    LaneStack<typename StackOf<MODE>::type> stk;
    SceneView sv;
    setup_traversal<MODE, BLOCK>(p, &sv, &stk);
    WorkCount wc;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
        const float4* r = reinterpret_cast<const float4*>(&rays[i]);
        const float4 a = r[0], b = r[1];
        const f3 P = mk(a.x, a.y, a.z), D = mk(b.x, b.y, b.z);
        float t;
        const int ti = closest_hit<MODE, false>(sv, P, D, stk, &t, &wc);
        float4 res = make_float4(0.f, 0.f, 0.f, -1.0f);
        if (ti >= 0) {
            const float4 c = p.tris[ti * 3 + 2];
            const f3 N = mk(c.y, c.z, c.w);
            const f3 hp = madd(D, t, P);
            const f3 Ng = dot3(D, N) > 0.0f ? -N : N;                     // shade_hit's flip
            const int mati = p.meta[ti].mati;
            const pt_material* __restrict__ m = &p.mats[mati];
            f3 kd = ldf3(m->kd);
            (void)shading_normal_albedo(vn, tv, p.tris, ti, D, hp, N, Ng, m->type, mati, &kd);
            res = make_float4(kd.x, kd.y, kd.z, t);
        }
        out_tri[i] = ti;
        out_rgbt[i] = res;
    }
}

hipError_t launch_debug_albedo(const RenderParams& p, const float4* vn, const TexView& tv, const pt_ray* rays, int64_t n, int32_t* out_tri, float4* out_rgbt,
                               int cu_count, hipStream_t stream) {
    return launch_lanes([](auto s) { return k_debug_albedo<s.mode, s.block>; }, p, n, cu_count, stream, vn, tv, rays, (long long)n, out_tri, out_rgbt);
}

}  // namespace ptamd
