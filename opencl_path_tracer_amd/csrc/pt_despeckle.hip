// pt_despeckle.hip -- the variance-gated firefly filter (pt_despeckle; pinned in include/pt_api.h).
//   k_despeckle<R, SPREAD>  16x16 blocks, one lane per pixel of the tile, three phases with a barrier between them:
//     1. the tile's luminance plus a halo is staged in LDS once (not live or outside the frame: NaN, so "live" is l == l everywhere
//        below and an edge is never a clamped coordinate);
//     2. SPREAD: every pixel of the tile plus a ring of R is decided (the tile's lanes take the (16 + 2R)^2 pixels 256 at a time), which
//        needs luminance for a halo of 2R: 28 x 28 floats at R = 3.  A lane keeps the three largest neighbour luminances in registers
//        (compare / select: rank <= 3).  A flagged pixel's share {e / n, l(e / n)} and its scale go to LDS; its colour and variance
//        are the only global reads of this phase, and only candidates (l > T) make them;
//        without SPREAD a lane decides its own pixel only and the halo is R;
//     3. a lane gathers the shares of the flagged pixels of its window in raster order and writes {c' + acc, v' + acc_v}, the variance
//        once more as a plain float array (what k_atrous_var's first iteration reads) and the flag.
//   A ring pixel is decided by every tile whose ring holds it, from the same inputs with the same code: the result does not depend on
//   the tiling.  No atomics; rank and the gate are wave-uniform arguments, R and SPREAD template parameters.
#include "pt_device.hpp"

namespace ptamd {

constexpr int kDsTile = 16;

// the decision of steps 2-3 without the variance gate for the pixel at (cx, cy) of the staged luminance (row length LW): 2 not live,
// 1 l > T, else 0; *T and *K as pinned
template <int R, int LW>
PT_DEV int despeckle_candidate(const float* s_l, int cx, int cy, int rank, float threshold, float floor_, float* l_out, float* T, int* K) {
    const float l = s_l[cy * LW + cx];
    *l_out = l;
    *T = 0.0f;
    *K = 0;
    if (!(l == l)) return 2;
    float t0 = -__builtin_inff(), t1 = t0, t2 = t0;
    int k = 0;
#pragma unroll
    for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const float q = s_l[(cy + dy) * LW + (cx + dx)];
            if (!(q == q)) continue;
            ++k;
            // insert q into t0 >= t1 >= t2 (with multiplicity: a tie takes the next slot)
            const bool g0 = q > t0, g1 = q > t1, g2 = q > t2;
            t2 = g1 ? t1 : (g2 ? q : t2);
            t1 = g0 ? t0 : (g1 ? q : t1);
            t0 = g0 ? q : t0;
        }
    }
    *K = k;
    if (k == 0) return 0;
    const int idx = rank < k ? rank : k;             // the rank-th largest, the smallest of them when K < rank
    const float m = idx == 1 ? t0 : (idx == 2 ? t1 : t2);
    *T = fmaf_(threshold, m, floor_);
    return l > *T ? 1 : 0;
}

PT_DEV bool despeckle_gate(float min_rel_sigma, float l, float v) {
    if (min_rel_sigma == 0.0f || v == __builtin_inff()) return true;
    const float g = min_rel_sigma * l;
    return v >= g * g;
}

template <int R, bool SPREAD>
__global__ void __launch_bounds__(kDsTile * kDsTile) k_despeckle(DespeckleArgs a) {
    constexpr int HL = SPREAD ? 2 * R : R;           // halo of the staged luminance
    constexpr int LW = kDsTile + 2 * HL;
    constexpr int DW = kDsTile + 2 * R;              // SPREAD: the decided region, tile + ring
    constexpr int ND = SPREAD ? DW * DW : 1;
    __shared__ float s_l[LW * LW];
    __shared__ float4 s_share[ND];                   // flagged: {e / n per channel, l(e / n)}
    __shared__ float s_scale[ND];                    // flagged: s = T / l
    __shared__ unsigned char s_flag[ND];
    const int tid = threadIdx.y * kDsTile + threadIdx.x;
    const int bx = blockIdx.x * kDsTile, by = blockIdx.y * kDsTile;
    for (int i = tid; i < LW * LW; i += kDsTile * kDsTile) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gx = bx + lx - HL, gy = by + ly - HL;
        float l = __builtin_nanf("");
        if (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) {
            const float4 c = a.c[(size_t)gy * a.W + gx];
            const float lc = luminance(mk(c.x, c.y, c.z));
            if (fabsf(lc) < __builtin_inff()) l = lc;
        }
        s_l[i] = l;
    }
    __syncthreads();
    if (SPREAD) {
        for (int i = tid; i < DW * DW; i += kDsTile * kDsTile) {
            const int cy = i / DW, cx = i - cy * DW;
            float l, T;
            int K;
            int flag = despeckle_candidate<R, LW>(s_l, cx + R, cy + R, a.rank, a.threshold, a.floor_, &l, &T, &K);
            if (flag == 1) {                         // a candidate is live, so inside the frame
                const size_t ig = (size_t)(by + cy - R) * a.W + (bx + cx - R);
                const float4 c = a.c[ig];
                const float v = a.v ? a.v[ig] : c.w;
                if (despeckle_gate(a.min_rel_sigma, l, v)) {
                    const float s = T / l, n = (float)(K + 1);
                    const f3 e = mk(c.x - c.x * s, c.y - c.y * s, c.z - c.z * s);
                    const f3 sh = mk(e.x / n, e.y / n, e.z / n);
                    s_share[i] = make_float4(sh.x, sh.y, sh.z, luminance(sh));
                    s_scale[i] = s;
                } else {
                    flag = 0;
                }
            }
            s_flag[i] = (unsigned char)flag;
        }
        __syncthreads();
    }
    const int x = bx + threadIdx.x, y = by + threadIdx.y;
    if (x >= a.W || y >= a.H) return;
    const size_t ip = (size_t)y * a.W + x;
    const float4 c = a.c[ip];
    const float v = a.v ? a.v[ip] : c.w;
    int flag;
    float s = 1.0f;
    if (SPREAD) {
        const int i0 = (threadIdx.y + R) * DW + (threadIdx.x + R);
        flag = s_flag[i0];
        if (flag == 1) s = s_scale[i0];
    } else {
        float l, T;
        int K;
        flag = despeckle_candidate<R, LW>(s_l, threadIdx.x + R, threadIdx.y + R, a.rank, a.threshold, a.floor_, &l, &T, &K);
        if (flag == 1) {
            if (despeckle_gate(a.min_rel_sigma, l, v)) s = T / l;
            else flag = 0;
        }
    }
    float4 o = make_float4(c.x, c.y, c.z, v);
    if (flag == 1) o = make_float4(c.x * s, c.y * s, c.z * s, v == __builtin_inff() ? v : (v * s) * s);
    if (SPREAD && flag != 2) {
        const int i0 = (threadIdx.y + R) * DW + (threadIdx.x + R);
        f3 acc = mk(0.f, 0.f, 0.f);
        float acc_v = 0.0f;
#pragma unroll
        for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
            for (int dx = -R; dx <= R; ++dx) {
                const int j = i0 + dy * DW + dx;
                if (s_flag[j] != 1) continue;
                const float4 sh = s_share[j];
                acc = mk(acc.x + sh.x, acc.y + sh.y, acc.z + sh.z);
                acc_v = fmaf_(sh.w, sh.w, acc_v);
            }
        }
        o = make_float4(o.x + acc.x, o.y + acc.y, o.z + acc.z, o.w + acc_v);
    }
    a.out[ip] = o;
    if (a.out_v) a.out_v[ip] = o.w;
    a.flags[ip] = flag;
}

hipError_t launch_despeckle(const DespeckleArgs& a, int32_t radius, int32_t spread, hipStream_t stream) {
    if (a.W <= 0 || a.H <= 0) return hipSuccess;
    const dim3 grid((a.W + kDsTile - 1) / kDsTile, (a.H + kDsTile - 1) / kDsTile), block(kDsTile, kDsTile);
    switch (radius * 2 + (spread ? 1 : 0)) {
    case 2: hipLaunchKernelGGL((k_despeckle<1, false>), grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL((k_despeckle<1, true>), grid, block, 0, stream, a); break;
    case 4: hipLaunchKernelGGL((k_despeckle<2, false>), grid, block, 0, stream, a); break;
    case 5: hipLaunchKernelGGL((k_despeckle<2, true>), grid, block, 0, stream, a); break;
    case 6: hipLaunchKernelGGL((k_despeckle<3, false>), grid, block, 0, stream, a); break;
    case 7: hipLaunchKernelGGL((k_despeckle<3, true>), grid, block, 0, stream, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace ptamd
