// pt_medium.hip -- the homogeneous medium of pt_set_medium (include/pt_api.h pins every operation).
//   k_debug_medium   pt_debug_medium: one thread per item runs medium_clip(), medium_flight(), medium_direction() and
//                    medium_transmittance() (pt_device.hpp), the functions the medium k_nee instances call (pt_nee.hip) for the free
//                    flight of a segment, the scatter vertex's new direction and the transmittance of a light sample, so that they can be
//                    tested against float64 without a render.  No scene is read; the numbers the kernels hash are given.
//   k_debug_grid     pt_debug_grid: one thread per item runs grid_walk() (pt_device.hpp), the walk the grid k_nee instances call for the
//                    free flight and the transmittance through the density grid of pt_set_medium_density
//   k_debug_interior pt_debug_interior: one thread per item runs interior_flight(), interior_absorb() and medium_direction() (pt_device.hpp),
//                    what the interior k_nee instances call on a segment inside a dielectric (pt_set_material_interior, section 5.21)
#include "pt_device.hpp"

namespace ptamd {

// in: 12 floats per item {P.xyz, D.xyz, t, u, u1, u2, limit, spare}; out: 10 per item {a, b, 1 if the segment scatters else 0, d,
// the new direction (unit) from (u1, u2) around D, its p_b, T of the ray (P, D) over [0, limit]}
__global__ void __launch_bounds__(256) k_debug_medium(MediumView mv, const float* __restrict__ in, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* q = in + i * 12;
    const f3 P = mk(q[0], q[1], q[2]), D = mk(q[3], q[4], q[5]);
    float a;
    const float b = medium_clip(mv, P, D, q[6], &a);
    const float d = medium_flight(mv.sigma_t, q[7]);
    float pb;
    const f3 w = normalize3(medium_direction(mv.g, D, q[8], q[9], &pb));
    float* o = out + i * 10;
    o[0] = a;
    o[1] = b;
    o[2] = d < max0(b - a) ? 1.0f : 0.0f;
    o[3] = d;
    o[4] = w.x;
    o[5] = w.y;
    o[6] = w.z;
    o[7] = pb;
    o[8] = medium_transmittance(mv, P, D, q[10]);
    o[9] = 0.0f;
}

hipError_t launch_debug_medium(const MediumView& mv, const float* in, int64_t n, float* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_debug_medium, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, mv, in, (long long)n, out);
    return hipGetLastError();
}

// in: 12 floats per item {P.xyz, D.xyz, t, u, limit, 3 spare}; out: 8 per item {a, b of Clip(P, D, t), 1 if the free flight of u scatters
// in [0, t] else 0, its distance s (-1 without a scatter), the optical depth over [0, t], T over [0, limit], the voxels the free flight
// visited, the linear index of the voxel it scattered in (-1 without)}
__global__ void __launch_bounds__(256) k_debug_grid(MediumView mv, GridView gv, const float* __restrict__ in, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* q = in + i * 12;
    const f3 P = mk(q[0], q[1], q[2]), D = mk(q[3], q[4], q[5]);
    const GridWalk fl = grid_walk<true>(mv, gv, P, D, q[6], -log1pf(-q[7]));
    const float depth = grid_walk<false>(mv, gv, P, D, q[6], __builtin_inff()).acc;
    const float through = grid_walk<false>(mv, gv, P, D, q[8], __builtin_inff()).acc;
    float* o = out + i * 8;
    o[0] = fl.a;
    o[1] = fl.b;
    o[2] = fl.voxel >= 0 ? 1.0f : 0.0f;
    o[3] = fl.s;
    o[4] = depth;
    o[5] = through != 0.0f ? expf(-through) : 1.0f;
    o[6] = (float)fl.visited;
    o[7] = (float)fl.voxel;
}

hipError_t launch_debug_grid(const MediumView& mv, const GridView& gv, const float* in, int64_t n, float* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_debug_grid, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, mv, gv, in, (long long)n, out);
    return hipGetLastError();
}

// in: 12 floats per item {sigma_a.rgb, sigma_s, g, t, u, u1, u2, D.xyz (unit)}; out: 10 per item {the free-flight distance d of u (-1 when
// sigma_s is 0: nothing is drawn), 1 if the segment scatters (d < t) else 0, the length l absorbed over, the absorption factor per channel,
// the new direction (unit) from (u1, u2) around D with g}
__global__ void __launch_bounds__(256) k_debug_interior(const float* __restrict__ in, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* q = in + i * 12;
    const float s = interior_flight(q[3], q[6], q[5]);
    const float l = s >= 0.0f ? s : q[5];
    const f3 f = interior_absorb(mk(q[0], q[1], q[2]), l);
    float pb;
    const f3 w = normalize3(medium_direction(q[4], mk(q[9], q[10], q[11]), q[7], q[8], &pb));
    float* o = out + i * 10;
    o[0] = q[3] > 0.0f ? medium_flight(q[3], q[6]) : -1.0f;
    o[1] = s >= 0.0f ? 1.0f : 0.0f;
    o[2] = l;
    o[3] = f.x;
    o[4] = f.y;
    o[5] = f.z;
    o[6] = w.x;
    o[7] = w.y;
    o[8] = w.z;
    o[9] = 0.0f;
}

hipError_t launch_debug_interior(const float* in, int64_t n, float* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_debug_interior, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in, (long long)n, out);
    return hipGetLastError();
}

}  // namespace ptamd
