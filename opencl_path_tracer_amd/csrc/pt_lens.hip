// pt_lens.hip -- the thin-lens camera of pt_set_lens (include/pt_api.h pins the lens ray).
//   k_debug_lens   pt_debug_lens: one thread per item {gid, S} draws the two LCG values of the sub-pixel position from S and runs
//                  lens_get_ray_xy() (pt_device.hpp), the function the lens instances of k_nee call (pt_nee.hip), so that the ray can be
//                  tested against float64 without a render.  No scene is read.
//   k_focus_at     pt_focus_at: one workgroup of the node mode's per-lane shape stages the tree; lane 0 of its first wave traces the centre
//                  ray of pixel gid with closest_hit and writes the hit's distance along the optical axis, t * dot3(D, f) (+inf: a miss).
#include "pt_device.hpp"

namespace ptamd {

__global__ void __launch_bounds__(256) k_debug_lens(pt_camera cam, LensView lv, const int* __restrict__ in, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int gid = in[i * 2];
    int seed = in[i * 2 + 1];
    const unsigned S = (unsigned)seed;
    const int camX = (int)cam.XM;
    const float rnd1 = lcg_rand(seed), rnd2 = lcg_rand(seed);
    f3 P, D;
    lens_get_ray_xy((float)(gid % camX), (float)(gid / camX), cam, lv, rnd1, rnd2, S, &P, &D);
    float* o = out + i * 6;
    o[0] = P.x;
    o[1] = P.y;
    o[2] = P.z;
    o[3] = D.x;
    o[4] = D.y;
    o[5] = D.z;
}

hipError_t launch_debug_lens(const pt_camera& cam, const LensView& lv, const int32_t* gid_state, int64_t n, float* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_debug_lens, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, cam, lv, (const int*)gid_state, (long long)n, out);
    return hipGetLastError();
}

template <int MODE, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_focus_at(RenderParams p, LensView lv, int gid, float* out) {
    LaneStack<typename StackOf<MODE>::type> stk;
    SceneView sv;
    setup_traversal<MODE, BLOCK>(p, &sv, &stk);
    WorkCount wc;
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    f3 P, D;
    camera_get_ray(gid, p.cam, 0.5f, 0.5f, &P, &D);
    float t;
    const int ti = closest_hit<MODE, false>(sv, P, D, stk, &t, &wc);
    *out = ti < 0 ? __builtin_inff() : t * dot3(D, mk(lv.f[0], lv.f[1], lv.f[2]));
}

hipError_t launch_focus_at(const RenderParams& p, const LensView& lv, int32_t gid, float* out, int cu_count, hipStream_t stream) {
    return launch_lanes([](auto s) { return k_focus_at<s.mode, s.block>; }, p, 1, cu_count, stream, lv, (int)gid, out);
}

}  // namespace ptamd
