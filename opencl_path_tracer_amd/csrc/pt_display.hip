// pt_display.hip -- the display stage (pt_display; pinned in include/pt_api.h).  256-thread blocks throughout.
//   k_display_hist     grid-stride over the frame: a per-block LDS histogram of the live pixels' luminance (bin from the float's bits),
//                      merged into the global one with integer atomics (integer sums do not depend on order)
//   k_display_meter    one wave: a prefix sum over the bins gives every bin's share k_b of the ranks [lo, hi); lane 0 folds S in the
//                      pinned ascending order and writes E, M, K next to the histogram.  The later kernels read E from there
//   k_display_down<B>  one 2x level down, 32 x 8 outputs per block, the 66 x 18 footprint staged in LDS with coordinates clamped while
//                      staging (so an edge is the staged value, never a branch in the taps); B: the source is the frame, and the bright
//                      pass is applied while staging
//   k_display_up       U_k = D_k + up(U_(k+1)) in place over D_k, 32 x 8 outputs per block from an 18 x 6 staged footprint
//   k_display_final<B> 64 x 16 pixels per block, four per lane, a wave on one row: exposure, (B) the last upsample from a 34 x 10 staged
//                      footprint, curve, encoding, the float4 result, and the bytes packed through LDS into whole dwords when W % 4 == 0
//   A staged value is what the clamped coordinate holds and every output sums its taps in one fixed order, so no result depends on the
//   tiling.  No atomics on floats: two runs give the same bits.
#include "pt_device.hpp"

namespace ptamd {

constexpr int kDpThreads = 256;
constexpr float kDpLog2[8] = PT_DISPLAY_LOG2_TABLE;

PT_DEV bool dp_finite(float x) { return fabsf(x) < __builtin_inff(); }
// step 0: live iff r, g, b and l are finite
PT_DEV bool display_live(const float4 c, float* l) {
    *l = luminance(mk(c.x, c.y, c.z));
    return dp_finite(c.x) && dp_finite(c.y) && dp_finite(c.z) && dp_finite(*l);
}
PT_DEV float4 dp_add(const float4 a, const float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, 0.0f); }
PT_DEV float4 dp_scale(float s, const float4 a) { return make_float4(s * a.x, s * a.y, s * a.z, 0.0f); }
PT_DEV int dp_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ void __launch_bounds__(kDpThreads) k_display_hist(const float4* __restrict__ c, int64_t n, DisplayStat* st) {
    __shared__ uint32_t s_h[kDisplayStatCounters - 1];     // 256 bins, n_dark, n_nonfinite
    for (int i = threadIdx.x; i < (int)kDisplayStatCounters - 1; i += kDpThreads) s_h[i] = 0u;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kDpThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kDpThreads) {
        float l;
        int slot = 257;
        if (display_live(c[i], &l)) {
            slot = 256;
            if (l >= 0x1p-16f) {
                const int b = (int)(__float_as_uint(l) >> 20) - 888;
                slot = b < 255 ? b : 255;
            }
        }
        atomicAdd(&s_h[slot], 1u);
    }
    __syncthreads();
    uint32_t* g = st->hist;                                 // (n_dark and n_nonfinite follow the bins)
    for (int i = threadIdx.x; i < (int)kDisplayStatCounters - 1; i += kDpThreads) {
        const uint32_t v = s_h[i];
        if (v) atomicAdd(&g[i], v);
    }
}

__global__ void __launch_bounds__(64) k_display_meter(DisplayArgs a) {
    __shared__ uint32_t s_k[256];
    DisplayStat* st = a.stat;
    const int lane = threadIdx.x;
    uint32_t cnt[4], own = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        cnt[j] = st->hist[4 * lane + j];
        own += cnt[j];
    }
    uint32_t inc = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
    }
    const uint64_t N = __shfl(inc, 63, 64);
    const uint64_t lo = N * (uint64_t)a.low_permille / 1000u, hi = N * (uint64_t)a.high_permille / 1000u;
    uint64_t cum = inc - own;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint64_t b = cum > lo ? cum : lo, e = cum + cnt[j] < hi ? cum + cnt[j] : hi;
        s_k[4 * lane + j] = e > b ? (uint32_t)(e - b) : 0u;
        cum += cnt[j];
    }
    __syncthreads();
    if (lane != 0) return;
    const float prev = a.prev_mode == 1 ? st->exposure : a.prev_value;     // (read before this call's E is written)
    float S = 0.0f;
    uint32_t K = 0u;
    for (int b = 0; b < 256; ++b) {
        const uint32_t k = s_k[b];
        K += k;
        S = fmaf_((float)k, (float)((b >> 3) - 16) + kDpLog2[b & 7], S);
    }
    const float M = K ? S / (float)K : 0.0f;
    float E = exp2f(a.ev);
    if (a.metering == PT_METER_AUTO) {
        if (K) {
            E = a.key * exp2f(a.ev - M);
            const float e_lo = exp2f(a.min_ev), e_hi = exp2f(a.max_ev);
            E = E < e_lo ? e_lo : (E > e_hi ? e_hi : E);
        }
        if (a.prev_mode != 0 && a.adapt < 1.0f) E = exp2f((1.0f - a.adapt) * log2f(prev) + a.adapt * log2f(E));
    }
    st->n_metered = K;
    st->mean_log2 = M;
    st->exposure = E;
}

// step 2: the bright pass of pixel c under exposure E
PT_DEV float4 display_bright(const float4 c, float E, float threshold) {
    float l;
    if (!display_live(c, &l)) return make_float4(0.f, 0.f, 0.f, 0.f);
    const f3 h = mk(E * c.x, E * c.y, E * c.z);
    const float lh = luminance(h);
    if (!(lh > threshold)) return make_float4(0.f, 0.f, 0.f, 0.f);
    const float d = lh - threshold;
    return make_float4((h.x * d) / lh, (h.y * d) / lh, (h.z * d) / lh, 0.0f);
}

constexpr int kDpTileW = 32, kDpTileH = 8;                 // the outputs of one block of k_display_down / k_display_up

template <bool BRIGHT>
__global__ void __launch_bounds__(kDpThreads) k_display_down(const float4* __restrict__ src, int sw, int sh, float4* __restrict__ dst, int dw, int dh,
                                                             const DisplayStat* st, float threshold) {
    constexpr int FW = 2 * kDpTileW + 2, FH = 2 * kDpTileH + 2;
    __shared__ float4 s[FW * FH];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kDpTileW, y0 = blockIdx.y * kDpTileH;
    const int nx = min(kDpTileW, dw - x0), ny = min(kDpTileH, dh - y0);
    const int fw = 2 * nx + 2, fh = 2 * ny + 2;
    const float E = BRIGHT ? st->exposure : 0.0f;
    for (int i = tid; i < fw * fh; i += kDpThreads) {
        const int ly = i / fw, lx = i - ly * fw;
        const int gx = dp_clamp(2 * x0 - 1 + lx, sw - 1), gy = dp_clamp(2 * y0 - 1 + ly, sh - 1);
        float4 v = src[(size_t)gy * sw + gx];
        if (BRIGHT) v = display_bright(v, E, threshold);
        s[ly * FW + lx] = v;
    }
    __syncthreads();
    const int lx = tid % kDpTileW, ly = tid / kDpTileW;
    if (lx >= nx || ly >= ny) return;
    const float a[4] = {0.125f, 0.375f, 0.375f, 0.125f};
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4* row = s + (2 * ly + j) * FW + 2 * lx;
        float4 r = dp_scale(a[0], row[0]);
#pragma unroll
        for (int i = 1; i < 4; ++i) r = dp_add(r, dp_scale(a[i], row[i]));
        acc = j == 0 ? dp_scale(a[0], r) : dp_add(acc, dp_scale(a[j], r));
    }
    dst[(size_t)(y0 + ly) * dw + (x0 + lx)] = acc;
}

// up(src)(x, y) for the target pixel (x, y) of a tile whose staged footprint starts at source (sx0, sy0), row length FW
template <int FW>
PT_DEV float4 display_up_tap(const float4* s, int x, int y, int sx0, int sy0) {
    const int cx = (x >> 1) - sx0, cy = (y >> 1) - sy0;
    const int qx = cx + ((x & 1) ? 1 : -1), qy = cy + ((y & 1) ? 1 : -1);
    const float4 t0 = dp_add(dp_scale(0.75f, s[cy * FW + cx]), dp_scale(0.25f, s[cy * FW + qx]));
    const float4 t1 = dp_add(dp_scale(0.75f, s[qy * FW + cx]), dp_scale(0.25f, s[qy * FW + qx]));
    return dp_add(dp_scale(0.75f, t0), dp_scale(0.25f, t1));
}
// stages the (TW / 2 + 2) x (TH / 2 + 2) footprint of the target tile at (x0, y0), coordinates clamped to the sw x sh source
template <int TW, int TH>
PT_DEV void display_up_stage(float4* s, const float4* __restrict__ src, int sw, int sh, int x0, int y0, int tid) {
    constexpr int FW = TW / 2 + 2, FH = TH / 2 + 2;
    for (int i = tid; i < FW * FH; i += kDpThreads) {
        const int ly = i / FW, lx = i - ly * FW;
        const int gx = dp_clamp(x0 / 2 - 1 + lx, sw - 1), gy = dp_clamp(y0 / 2 - 1 + ly, sh - 1);
        s[i] = src[(size_t)gy * sw + gx];
    }
}

__global__ void __launch_bounds__(kDpThreads) k_display_up(const float4* __restrict__ src, int sw, int sh, float4* dst, int dw, int dh) {
    constexpr int FW = kDpTileW / 2 + 2, FH = kDpTileH / 2 + 2;
    __shared__ float4 s[FW * FH];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kDpTileW, y0 = blockIdx.y * kDpTileH;
    display_up_stage<kDpTileW, kDpTileH>(s, src, sw, sh, x0, y0, tid);
    __syncthreads();
    const int x = x0 + tid % kDpTileW, y = y0 + tid / kDpTileW;
    if (x >= dw || y >= dh) return;
    const size_t ip = (size_t)y * dw + x;
    dst[ip] = dp_add(dst[ip], display_up_tap<FW>(s, x, y, x0 / 2 - 1, y0 / 2 - 1));
}

// step 3 for one channel value v of the curve: clamp (NaN -> 0), encoding
PT_DEV float display_encode(float v, int encoding) {
    v = !(v > 0.0f) ? 0.0f : (v > 1.0f ? 1.0f : v);
    if (encoding == PT_ENCODE_SRGB) v = v < 0.0031308f ? 12.92f * v : 1.055f * powf(v, 1.0f / 2.4f) - 0.055f;
    return v;
}
PT_DEV float display_aces(float x) { return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f); }

constexpr int kDpFinalW = 64, kDpFinalH = 16;

template <bool BLOOM>
__global__ void __launch_bounds__(kDpThreads) k_display_final(DisplayArgs a, const float4* __restrict__ u1, int uw, int uh) {
    constexpr int FW = kDpFinalW / 2 + 2, FH = kDpFinalH / 2 + 2;
    __shared__ float4 s[BLOOM ? FW * FH : 1];
    __shared__ __attribute__((aligned(4))) unsigned char s_b[kDpFinalH * kDpFinalW * 3];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * kDpFinalW, y0 = blockIdx.y * kDpFinalH;
    if (BLOOM) {
        display_up_stage<kDpFinalW, kDpFinalH>(s, u1, uw, uh, x0, y0, tid);
        __syncthreads();
    }
    const float E = a.stat->exposure;
    const float gain = BLOOM ? a.intensity / (float)a.levels : 0.0f;
    const float w2 = a.white * a.white;
#pragma unroll
    for (int q = 0; q < kDpFinalW * kDpFinalH / kDpThreads; ++q) {
        const int lx = tid % kDpFinalW, ly = tid / kDpFinalW + q * (kDpThreads / kDpFinalW);
        const int x = x0 + lx, y = y0 + ly;
        if (x >= a.W || y >= a.H) continue;
        const size_t ip = (size_t)y * a.W + x;
        const float4 c = a.c[ip];
        float l;
        f3 v = mk(0.f, 0.f, 0.f);
        if (display_live(c, &l)) {
            f3 o = mk(E * c.x, E * c.y, E * c.z);
            if (BLOOM) {
                const float4 up = display_up_tap<FW>(s, x, y, x0 / 2 - 1, y0 / 2 - 1);
                o = mk(o.x + gain * up.x, o.y + gain * up.y, o.z + gain * up.z);
            }
            const f3 xx = mk(max0(o.x), max0(o.y), max0(o.z));
            f3 t = xx;
            if (a.curve == PT_CURVE_REINHARD) {
                const float L = luminance(xx);
                const float k = (1.0f + L / w2) / (1.0f + L);
                t = mk(xx.x * k, xx.y * k, xx.z * k);
            } else if (a.curve == PT_CURVE_ACES) {
                t = mk(display_aces(xx.x), display_aces(xx.y), display_aces(xx.z));
            }
            v = mk(display_encode(t.x, a.encoding), display_encode(t.y, a.encoding), display_encode(t.z, a.encoding));
        }
        a.out[ip] = make_float4(v.x, v.y, v.z, 1.0f);
        unsigned char* b = s_b + (ly * kDpFinalW + lx) * 3;
        b[0] = (unsigned char)floorf(255.0f * v.x + 0.5f);
        b[1] = (unsigned char)floorf(255.0f * v.y + 0.5f);
        b[2] = (unsigned char)floorf(255.0f * v.z + 0.5f);
    }
    __syncthreads();
    // the tile's bytes: row y of the frame is row H - 1 - y of the image
    const int nx = min(kDpFinalW, a.W - x0), ny = min(kDpFinalH, a.H - y0);
    if ((a.W & 3) == 0) {                                   // every row segment starts and ends on a dword
        const int nd = nx * 3 / 4;
        for (int i = tid; i < ny * nd; i += kDpThreads) {
            const int ly = i / nd, d = i - ly * nd;
            const size_t off = ((size_t)(a.H - 1 - (y0 + ly)) * a.W + x0) * 3 + (size_t)d * 4;
            *reinterpret_cast<uint32_t*>(a.rgb8 + off) = *reinterpret_cast<const uint32_t*>(s_b + ly * kDpFinalW * 3 + d * 4);
        }
    } else {
        const int nb = nx * 3;
        for (int i = tid; i < ny * nb; i += kDpThreads) {
            const int ly = i / nb, d = i - ly * nb;
            a.rgb8[((size_t)(a.H - 1 - (y0 + ly)) * a.W + x0) * 3 + d] = s_b[ly * kDpFinalW * 3 + d];
        }
    }
}

hipError_t launch_display(const DisplayArgs& a, hipStream_t stream) {
    if (a.W <= 0 || a.H <= 0) return hipSuccess;
    if (a.levels < 0 || a.levels > kDisplayMaxLevels) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(a.stat, 0, sizeof(uint32_t) * kDisplayStatCounters, stream);
    if (e != hipSuccess) return e;
    const int64_t n = (int64_t)a.W * a.H;
    const int hist_blocks = (int)std::min<int64_t>((n + kDpThreads - 1) / kDpThreads, 2048);
    hipLaunchKernelGGL(k_display_hist, dim3(hist_blocks), dim3(kDpThreads), 0, stream, a.c, n, a.stat);
    hipLaunchKernelGGL(k_display_meter, dim3(1), dim3(64), 0, stream, a);
    auto grid = [](int w, int h, int tw, int th) { return dim3((w + tw - 1) / tw, (h + th - 1) / th); };
    float4* lev[kDisplayMaxLevels + 1] = {};
    int lw[kDisplayMaxLevels + 1], lh[kDisplayMaxLevels + 1];
    lw[0] = a.W;
    lh[0] = a.H;
    float4* next = a.pyr;
    for (int k = 1; k <= a.levels; ++k) {
        lw[k] = (lw[k - 1] + 1) / 2;
        lh[k] = (lh[k - 1] + 1) / 2;
        lev[k] = next;
        next += (size_t)lw[k] * lh[k];
        if (k == 1)
            hipLaunchKernelGGL((k_display_down<true>), grid(lw[1], lh[1], kDpTileW, kDpTileH), dim3(kDpThreads), 0, stream, a.c, a.W, a.H, lev[1], lw[1], lh[1],
                               a.stat, a.threshold);
        else
            hipLaunchKernelGGL((k_display_down<false>), grid(lw[k], lh[k], kDpTileW, kDpTileH), dim3(kDpThreads), 0, stream, lev[k - 1], lw[k - 1], lh[k - 1],
                               lev[k], lw[k], lh[k], a.stat, 0.0f);
    }
    for (int k = a.levels - 1; k >= 1; --k)
        hipLaunchKernelGGL(k_display_up, grid(lw[k], lh[k], kDpTileW, kDpTileH), dim3(kDpThreads), 0, stream, lev[k + 1], lw[k + 1], lh[k + 1], lev[k], lw[k], lh[k]);
    const dim3 fg = grid(a.W, a.H, kDpFinalW, kDpFinalH);
    if (a.levels > 0) hipLaunchKernelGGL((k_display_final<true>), fg, dim3(kDpThreads), 0, stream, a, lev[1], lw[1], lh[1]);
    else hipLaunchKernelGGL((k_display_final<false>), fg, dim3(kDpThreads), 0, stream, a, nullptr, 0, 0);
    return hipGetLastError();
}

}  // namespace ptamd
