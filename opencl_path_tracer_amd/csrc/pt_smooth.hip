// pt_smooth.hip -- smooth shading from vertex normals (option smooth_normals; include/pt_api.h pins the estimator).
//   k_pack_vertex_normals    one thread per packed triangle, run on the context's stream in front of the first smooth launch after the
//                            recorded normals or the uploaded triangles changed (smooth_prepare, pt_host.cpp): gathers the add-order
//                            normals through the permutation `orig` into 3 float4 {n.xyz, flag} per packed triangle.  Each normal is
//                            divided by its float64 length and rounded once; flag != 0 iff all nine values are finite and no vector is
//                            zero (a triangle past the recorded ones has none).
//   k_debug_shading_normal   pt_debug_shading_normal: closest hit of a ray, then shading_normal() (pt_device.hpp), the function the
//                            smooth k_nee instances call (pt_nee.hip), so the interpolation can be tested without a render.
#include "pt_device.hpp"

namespace ptamd {

__global__ void __launch_bounds__(256) k_pack_vertex_normals(const float* __restrict__ src, long long n_src, const int* __restrict__ orig, int n, float4* __restrict__ out) {
    const int ti = blockIdx.x * blockDim.x + threadIdx.x;
    if (ti >= n) return;
    const long long o = orig[ti];
    float4 q[3] = {make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, 0.f)};
    if (o >= 0 && o < n_src) {
        bool has = true;
        for (int c = 0; c < 3; ++c) {
            const double x = (double)src[o * 9 + c * 3], y = (double)src[o * 9 + c * 3 + 1], z = (double)src[o * 9 + c * 3 + 2];
            const double l = __builtin_sqrt(x * x + y * y + z * z);        // finite for every finite float triple, 0 only for a zero vector
            has = has && l > 0.0 && l < (double)__builtin_inff();
            q[c] = make_float4((float)(x / l), (float)(y / l), (float)(z / l), 1.0f);
        }
        if (!has)
            for (int c = 0; c < 3; ++c) q[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int c = 0; c < 3; ++c) out[(size_t)ti * 3 + c] = q[c];
}

hipError_t launch_pack_vertex_normals(const float* src, int64_t n_src, const int32_t* orig, int32_t n, float4* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pack_vertex_normals, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, (long long)n_src, orig, (int)n, out);
    return hipGetLastError();
}

// persistent blocks, grid-stride over the rays; one ray per lane at a time (as k_debug_closest_hit)
template <int MODE, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_debug_shading_normal(RenderParams p, const float4* vn, const pt_ray* rays, long long n, int* out_tri, float4* out_ns) {
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
        float4 ns = make_float4(0.f, 0.f, 0.f, -1.0f);
        if (ti >= 0) {
            const float4 c = p.tris[ti * 3 + 2];
            const f3 N = mk(c.y, c.z, c.w);
            const f3 hp = madd(D, t, P);
            const f3 Ng = dot3(D, N) > 0.0f ? -N : N;                     // shade_hit's flip
            const f3 s = shading_normal(vn, p.tris, ti, D, hp, N, Ng);
            ns = make_float4(s.x, s.y, s.z, t);
        }
        out_tri[i] = ti;
        out_ns[i] = ns;
    }
}

hipError_t launch_debug_shading_normal(const RenderParams& p, const float4* vn, const pt_ray* rays, int64_t n, int32_t* out_tri, float4* out_ns, int cu_count,
                                       hipStream_t stream) {
    return launch_lanes([](auto s) { return k_debug_shading_normal<s.mode, s.block>; }, p, n, cu_count, stream, vn, rays, (long long)n, out_tri, out_ns);
}

}  // namespace ptamd
