// pt_glossy.hip -- the rough metal of option glossy (material type 4; include/pt_api.h pins the vertex).
//   k_debug_glossy   pt_debug_glossy: one thread per item runs lobe_direction_rough() and glossy_pdf_of() (pt_device.hpp), the functions
//                    the glossy k_nee instances call (pt_nee.hip) for the sampled direction and for a light sample, so that the sampler
//                    and the density can be tested against each other and against float64 without a render.  No scene is read.
//   k_debug_coated   pt_debug_coated: the same for the coated diffuse of option coated (material type 5).
//   k_debug_frosted  pt_debug_frosted: the same for the rough dielectric of option frosted (material type 6).
#include "pt_device.hpp"

namespace ptamd {

// in: 9 floats per item {N.xyz, D.xyz, alpha, rnd1, rnd2}; out: 8 per item {w.xyz before normalisation (world), p_b as sampled, G1(w),
// F.x with F0 = 0.04, p_b evaluated again from w, o.z}
__global__ void __launch_bounds__(256) k_debug_glossy(const float* __restrict__ in, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* a = in + i * 9;
    const f3 N = mk(a[0], a[1], a[2]), D = mk(a[3], a[4], a[5]);
    const float alpha = a[6];
    GlossyOut go;
    const f3 F0 = mk(0.04f, 0.04f, 0.04f);
    const f3 d = lobe_direction_rough<false, false>(N, D, true, false, false, alpha, F0, F0, 1.0f, 0.0f, a[7], a[8], &go, nullptr, nullptr);
    // the density of the same direction by the light sample's route: world -> local, h = normalize(o + w)
    f3 Z, X, h;
    tangent_frame(N, &Z, &X);
    const float again = glossy_pdf_of(alpha, to_local(-D, X, Z, N), to_local(normalize3(d), X, Z, N), &h);
    float* o = out + i * 8;
    o[0] = d.x;
    o[1] = d.y;
    o[2] = d.z;
    o[3] = go.pb;
    o[4] = go.g1w;
    o[5] = go.F.x;
    o[6] = again;
    o[7] = go.oz;
}

hipError_t launch_debug_glossy(const float* in, int64_t n, float* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_debug_glossy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in, (long long)n, out);
    return hipGetLastError();
}

// pt_debug_coated: lobe_direction_rough() and coated_pdf_weight_of() (pt_device.hpp), the functions the coated k_nee instances call for
// the sampled direction and for a light sample.  in: 12 floats per item {N.xyz, D.xyz, alpha, F0, kd, rnd1, rnd2, u_sel} (F0 and kd grey);
// out: 10 per item {w.xyz before normalisation (world), ps, 1 if the coat lobe drew w else 0, p_b as sampled, g.x as sampled, p_b and g.x
// evaluated again from normalize(w), o.z}.  One thread per item: item i runs on lane i % 64
__global__ void __launch_bounds__(256) k_debug_coated(const float* __restrict__ in, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* a = in + i * 12;
    const f3 N = mk(a[0], a[1], a[2]), D = mk(a[3], a[4], a[5]);
    const float alpha = a[6];
    const f3 F0 = mk(a[7], a[7], a[7]), kd = mk(a[8], a[8], a[8]);
    GlossyOut go;
    CoatedOut co;
    const f3 d = lobe_direction_rough<false, true>(N, D, false, true, false, alpha, F0, kd, 1.0f, a[11], a[9], a[10], &go, &co, nullptr);
    // the same direction by the light sample's route: world -> local, ps and h = normalize(o + w) from scratch
    f3 Z, X, g;
    tangent_frame(N, &Z, &X);
    const float again = coated_pdf_weight_of(alpha, F0, kd, to_local(-D, X, Z, N), to_local(normalize3(d), X, Z, N), &g);
    float* o = out + i * 10;
    o[0] = d.x;
    o[1] = d.y;
    o[2] = d.z;
    o[3] = co.ps;
    o[4] = co.coat ? 1.0f : 0.0f;
    o[5] = co.pb;
    o[6] = co.g.x;
    o[7] = again;
    o[8] = g.x;
    o[9] = co.oz;
}

hipError_t launch_debug_coated(const float* in, int64_t n, float* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_debug_coated, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in, (long long)n, out);
    return hipGetLastError();
}

// pt_debug_frosted: lobe_direction_rough() and frosted_pdf_weight_of() (pt_device.hpp), the functions the frosted k_nee instances call for
// the sampled direction and for a light sample.  in: 12 floats per item {N.xyz, D.xyz, alpha, F0 (grey), eta, rnd1, rnd2, u_sel}; out: 10
// per item {w.xyz before normalisation (world), Fm, 1 if the vertex reflects else 0, p_b as sampled (0 for a refraction), g.x as sampled,
// p_b and g.x evaluated again from normalize(w) (0, 0 for a refraction), o.z}.  One thread per item: item i runs on lane i % 64
__global__ void __launch_bounds__(256) k_debug_frosted(const float* __restrict__ in, long long n, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* a = in + i * 12;
    const f3 N = mk(a[0], a[1], a[2]), D = mk(a[3], a[4], a[5]);
    const float alpha = a[6], eta = a[8];
    const f3 F0 = mk(a[7], a[7], a[7]);
    GlossyOut go;
    CoatedOut co;
    FrostedOut fo;
    const f3 d = lobe_direction_rough<false, true>(N, D, false, false, true, alpha, F0, F0, eta, a[11], a[9], a[10], &go, &co, &fo);
    // a reflected direction once more by the light sample's route: world -> local, h = normalize(o + w) and the terms from scratch
    float again = 0.0f;
    f3 g = mk(0.f, 0.f, 0.f);
    if (fo.refl) {
        f3 Z, X;
        tangent_frame(N, &Z, &X);
        again = frosted_pdf_weight_of(alpha, F0, eta, to_local(-D, X, Z, N), to_local(normalize3(d), X, Z, N), &g);
    }
    float* o = out + i * 10;
    o[0] = d.x;
    o[1] = d.y;
    o[2] = d.z;
    o[3] = fo.Fm;
    o[4] = fo.refl ? 1.0f : 0.0f;
    o[5] = fo.pb;
    o[6] = fo.g.x;
    o[7] = again;
    o[8] = g.x;
    o[9] = fo.oz;
}

hipError_t launch_debug_frosted(const float* in, int64_t n, float* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_debug_frosted, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in, (long long)n, out);
    return hipGetLastError();
}

}  // namespace ptamd
