// pt_temporal.hip -- temporal accumulation with reprojection (pt_temporal_accumulate; pinned in include/pt_api.h).
//   k_temporal  one lane per local pixel, 32x8 blocks like k_atrous: the pixel's primary hit (its depth guide) is reprojected into the
//               history's view (reproject(), pt_internal.hpp, the statement pt_debug_reproject shares), the history is read from a 2x2
//               bilinear footprint of the previous set -- four taps at most, no LDS: neighbouring lanes read neighbouring taps, so
//               they come from L2 -- and blended with the frame by sample count.  Writes the new set (colour + m2, the guides it was
//               made with, n + material) and the variance of the mean.
#include "pt_device.hpp"

namespace ptamd {

constexpr float kTemporalSnap = 0x1p-10f;     // bilinear weights closer than this to 0 or 1 snap to one tap
constexpr float kTemporalMinWeight = 0.01f;   // history from less than this much bilinear weight is dropped

__global__ void __launch_bounds__(256) k_temporal(TemporalArgs a) {
    const int x = blockIdx.x * 32 + (threadIdx.x & 31);
    const int y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= a.W || y >= a.H) return;
    const size_t ip = (size_t)y * a.W + x;
    const int k = a.tile_spp ? a.tile_spp[(y >> 3) * ((a.W + 7) >> 3) + (x >> 3)] : a.n_all;
    const float4 c = a.colors[ip];
    const float4 g = a.nd[ip];
    const float mat = a.albedo[ip].w;
    // the history at p: the weight-normalised sums over the valid taps of the footprint (hn = 0: none)
    float hn = 0.0f, hm2 = 0.0f;
    f3 hc = mk(0.f, 0.f, 0.f);
    float r[3];
    if (a.has_prev && a.max_history > 0.0f && g.w >= 0.0f && reproject(a.cur, a.prev, (int)ip, g.w, r) &&
        r[0] > -2.0f && r[0] < (float)a.W + 1.0f && r[1] > -2.0f && r[1] < (float)a.H + 1.0f) {   // (no tap in the frame otherwise)
        int x0 = (int)floorf(r[0]), y0 = (int)floorf(r[1]);
        float fx = r[0] - (float)x0, fy = r[1] - (float)y0;
        if (fx < kTemporalSnap) fx = 0.0f;
        else if (fx > 1.0f - kTemporalSnap) { fx = 0.0f; ++x0; }
        if (fy < kTemporalSnap) fy = 0.0f;
        else if (fy > 1.0f - kTemporalSnap) { fy = 0.0f; ++y0; }
        const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
        const f3 np = mk(g.x, g.y, g.z);
        const bool zero_np = g.x == 0.0f && g.y == 0.0f && g.z == 0.0f;
        f3 sc = mk(0.f, 0.f, 0.f);
        float sm2 = 0.0f, sn = 0.0f, sw = 0.0f;
        for (int j = 0; j < 2; ++j) {
            for (int i = 0; i < 2; ++i) {
                const float w = wx[i] * wy[j];
                if (w == 0.0f) continue;                        // neither read nor tested
                const int qx = x0 + i, qy = y0 + j;
                if (qx < 0 || qx >= a.W || qy < 0 || qy >= a.H) continue;
                const size_t iq = (size_t)qy * a.W + qx;
                const float4 gq = a.prev_g[iq];
                const float2 nmq = a.prev_nm[iq];
                if (!(gq.w > 0.0f) || nmq.y != mat) continue;
                const bool zero_nq = gq.x == 0.0f && gq.y == 0.0f && gq.z == 0.0f;
                if (zero_np != zero_nq) continue;
                if (!zero_np && !(dot3(np, mk(gq.x, gq.y, gq.z)) >= a.normal_cos)) continue;
                if (!(fabsf(r[2] - gq.w) <= a.depth_tolerance * gq.w)) continue;
                const float4 cq = a.prev_c[iq];
                sc = madd(mk(cq.x, cq.y, cq.z), w, sc);
                sm2 = fmaf_(cq.w, w, sm2);
                sn = fmaf_(nmq.x, w, sn);
                sw += w;
            }
        }
        if (sw >= kTemporalMinWeight) {
            hc = mk(sc.x / sw, sc.y / sw, sc.z / sw);
            hm2 = sm2 / sw;
            hn = sn / sw;
        }
    }
    // the blend, by samples: n = min(n_h, max_history) + k; no history leaves the frame's own bits
    const float kf = (float)k, nh = fminf(hn, a.max_history);
    float4 o = c;
    float n = kf;
    if (nh > 0.0f) {
        n = nh + kf;
        o = make_float4(fmaf_(nh, hc.x, kf * c.x) / n, fmaf_(nh, hc.y, kf * c.y) / n, fmaf_(nh, hc.z, kf * c.z) / n, fmaf_(nh, hm2, kf * c.w) / n);
    }
    const float mu = luminance(mk(o.x, o.y, o.z));
    a.out_v[ip] = n < 2.0f ? __builtin_inff() : fmaxf(fmaf_(-mu, mu, o.w), 0.0f) / (n - 1.0f);
    a.out_c[ip] = o;
    a.out_g[ip] = g;
    a.out_nm[ip] = make_float2(n, mat);
}

hipError_t launch_temporal(const TemporalArgs& a, hipStream_t stream) {
    if (a.W <= 0 || a.H <= 0) return hipSuccess;
    const dim3 grid((a.W + 31) / 32, (a.H + 7) / 8), block(256);
    hipLaunchKernelGGL(k_temporal, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace ptamd
