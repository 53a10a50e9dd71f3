// pt_debug.hip -- test entry point of libptamd.so: closest hit of caller-supplied rays through the
// same traversal code (pt_device.hpp) and the same node placement the render kernels use.
#include "pt_device.hpp"

namespace ptamd {

// persistent blocks, grid-stride over the rays; one ray per lane at a time
template <int MODE, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_debug_closest_hit(RenderParams p, const pt_ray* rays, long long n, float* out_t, int* out_tri) {
    LaneStack<typename StackOf<MODE>::type> stk;
    SceneView sv;
    setup_traversal<MODE, BLOCK>(p, &sv, &stk);
    WorkCount wc;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
        const float4* r = reinterpret_cast<const float4*>(&rays[i]);
        const float4 a = r[0], b = r[1];
        float t;
        const int ti = closest_hit<MODE, false>(sv, mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), stk, &t, &wc);
        out_t[i] = ti >= 0 ? t : -1.0f;
        out_tri[i] = ti;
    }
}

hipError_t launch_debug_closest_hit(const RenderParams& p, const pt_ray* rays, int64_t n, float* out_t, int32_t* out_tri, int cu_count, hipStream_t stream) {
    return launch_lanes([](auto s) { return k_debug_closest_hit<s.mode, s.block>; }, p, n, cu_count, stream, rays, (long long)n, out_t, out_tri);
}

}  // namespace ptamd
