// pt_adaptive.hip -- the per-round kernels of an adaptive frame (pt_render_adaptive, pt_launch.cpp).
//
//   k_adaptive_tiles   one wave per tile of the active list, one lane per pixel: the noise estimate of every pixel against the
//                      snapshot taken at half the tile's samples, the tile's maximum, the retire decision, and the next snapshot
//   k_adaptive_variance  the same wave per tile for metric PT_ADAPT_VARIANCE (pt_render_adaptive_ex): the variance of every pixel's mean
//                      luminance from colors[].xyz / .w (option "moments"), the tile's root mean square, the retire decision; no snapshot
//   k_compact_tiles    the tiles still active, in ascending frame-tile order (the raster order the schedules' coherence assumes),
//                      into the list the next round's k_render launch reads (RenderParams::tile_list)
//
// The estimate is part of the arithmetic contract: float32, this order, correctly rounded sqrt and divide --
//   d = (|M.r - A.r| + |M.g - A.g|) + |M.b - A.b|,  s = (M.r + M.g) + M.b,  e = d / (1e-4 + sqrt(s))
// so that a CPU replay (tests/adaptive_ref.py) reaches the same decisions bit for bit.  The variance metric's estimate is pinned the
// same way (include/pt_api.h next to pt_render_adaptive_ex; replay in tests/adaptive_variance_ref.py).
#include "pt_internal.hpp"

namespace ptamd {

// mode 0: tile_spp only; 1: + snapshot; 2: + estimate, decision, snapshot of the tiles that stay active.  Mode 0 reads no pixel and neither reads nor writes
// snap, and a null snap is allowed there: the variance metric, which keeps no snapshot, records its counts through it (pt_launch.cpp).
__global__ void __launch_bounds__(256) k_adaptive_tiles(const float4* colors, float4* snap, const int32_t* list, int32_t n_list, int32_t width,
                                                        int32_t rows, int mode, float threshold, int32_t spp, float* tile_err, int32_t* tile_spp,
                                                        uint8_t* active) {
    const int w = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (w >= n_list) return;                                           // (whole waves)
    const int tile = list ? __builtin_amdgcn_readfirstlane(list[w]) : w;
    const int tiles_x = (width + 7) >> 3;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int lane = threadIdx.x & 63;
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    const bool inside = x < width && y < rows;
    const size_t li = (size_t)y * (size_t)width + (size_t)x;
    // a row of a tile = 8 consecutive float4 (128 B); mode 0 records the count only and reads no pixel
    const float4 m = inside && mode != 0 ? colors[li] : make_float4(0.f, 0.f, 0.f, 0.f);
    bool keep = true;
    if (mode == 2) {
        float e = 0.0f;                                                // (lanes outside the frame: ignored -- every estimate is >= 0)
        if (inside) {
            const float4 a = snap[li];
            const float d = (fabsf(m.x - a.x) + fabsf(m.y - a.y)) + fabsf(m.z - a.z);
            const float s = (m.x + m.y) + m.z;
            e = d / (1e-4f + sqrtf(s));
            if (!isfinite(e)) e = __builtin_inff();
        }
        for (int off = 32; off > 0; off >>= 1) e = fmaxf(e, __shfl_xor(e, off, 64));
        const float err = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(e)));   // (every lane holds the maximum)
        keep = !(err < threshold);
        if (lane == 0) {
            tile_err[tile] = err;
            active[tile] = keep ? 1 : 0;
        }
    }
    if (lane == 0) tile_spp[tile] = spp;
    if (mode >= 1 && keep && inside) snap[li] = m;
}

// Metric PT_ADAPT_VARIANCE at boundary spp (>= 2): per pixel v = max(m2 - mu^2, 0) / (spp - 1), pt_read_variance's read-out; tonemapped:
// v / (1 + mu)^4, the variance behind the derivative of Reinhard's L / (1 + L); the tile's estimate is sqrt(sum v / pixels inside),
// the sum by xor butterfly (float add commutes, so every lane ends with the same bits).
__global__ void __launch_bounds__(256) k_adaptive_variance(const float4* colors, const int32_t* list, int32_t n_list, int32_t width, int32_t rows,
                                                           float threshold, int tonemapped, int32_t spp, float* tile_err, int32_t* tile_spp,
                                                           uint8_t* active) {
    const int w = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (w >= n_list) return;                                           // (whole waves)
    const int tile = list ? __builtin_amdgcn_readfirstlane(list[w]) : w;
    const int tiles_x = (width + 7) >> 3;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int lane = threadIdx.x & 63;
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    const bool inside = x < width && y < rows;
    float v = 0.0f;
    if (inside) {
        const float4 m = colors[(size_t)y * (size_t)width + (size_t)x];   // a row of a tile = 8 consecutive float4 (128 B)
        const float mu = __builtin_fmaf(0.0722f, m.z, __builtin_fmaf(0.7152f, m.y, 0.2126f * m.x));
        v = fmaxf(__builtin_fmaf(-mu, mu, m.w), 0.0f) / (float)(spp - 1);
        if (tonemapped) {
            const float d = 1.0f + mu;
            v = v / ((d * d) * (d * d));
        }
    }
    float s = v;
    for (int off = 32; off > 0; off >>= 1) s = s + __shfl_xor(s, off, 64);
    const int n_inside = (min(width - tx * 8, 8)) * (min(rows - ty * 8, 8));      // (a listed tile has pixels: both factors >= 1)
    float e = sqrtf(s / (float)n_inside);
    if (!isfinite(e)) e = __builtin_inff();
    const float err = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(e)));
    if (lane == 0) {
        tile_err[tile] = err;
        active[tile] = !(err < threshold) ? 1 : 0;
        tile_spp[tile] = spp;
    }
}

// One workgroup of 1,024 threads walks the flags in chunks of 4,096 (four per thread): a 4K frame's 129,600 tiles are 32 chunks of
// one read, a wave-level scan, a 16-entry scan through LDS and the scattered writes of the active tiles -- a few tens of microseconds
// once per round.
constexpr int kCompactBlock = 1024;
__global__ void __launch_bounds__(kCompactBlock) k_compact_tiles(const uint8_t* active, int32_t n, int32_t* list, int32_t* count) {
    __shared__ int wave_sum[kCompactBlock / 64];
    __shared__ int chunk_total;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += 4 * kCompactBlock) {
        const int i0 = c0 + 4 * t;
        int f[4];
        for (int k = 0; k < 4; ++k) f[k] = (i0 + k < n && active[i0 + k]) ? 1 : 0;
        const int mine = f[0] + f[1] + f[2] + f[3];
        int incl = mine;                                               // inclusive scan over the wave
        for (int off = 1; off < 64; off <<= 1) {
            const int v = __shfl_up(incl, off, 64);
            if (lane >= off) incl += v;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        if (t == 0) {
            int run = 0;
            for (int k = 0; k < kCompactBlock / 64; ++k) { const int v = wave_sum[k]; wave_sum[k] = run; run += v; }
            chunk_total = run;
        }
        __syncthreads();
        int pos = base + wave_sum[wave] + incl - mine;
        for (int k = 0; k < 4; ++k)
            if (f[k]) list[pos++] = i0 + k;
        base += chunk_total;
        __syncthreads();                                               // (wave_sum / chunk_total are rewritten by the next chunk)
    }
    if (t == 0) *count = base;
}

hipError_t launch_adaptive_tiles(const float4* colors, float4* snap, const int32_t* list, int32_t n_list, int32_t width, int32_t rows, int mode,
                                 float threshold, int32_t spp, float* tile_err, int32_t* tile_spp, uint8_t* active, hipStream_t stream) {
    if (n_list <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_adaptive_tiles, dim3((unsigned)((n_list + 3) / 4)), dim3(256), 0, stream, colors, snap, list, n_list, width, rows, mode,
                       threshold, spp, tile_err, tile_spp, active);
    return hipGetLastError();
}

hipError_t launch_adaptive_variance(const float4* colors, const int32_t* list, int32_t n_list, int32_t width, int32_t rows, float threshold,
                                    int tonemapped, int32_t spp, float* tile_err, int32_t* tile_spp, uint8_t* active, hipStream_t stream) {
    if (n_list <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_adaptive_variance, dim3((unsigned)((n_list + 3) / 4)), dim3(256), 0, stream, colors, list, n_list, width, rows, threshold,
                       tonemapped, spp, tile_err, tile_spp, active);
    return hipGetLastError();
}

hipError_t launch_compact_tiles(const uint8_t* active, int32_t n, int32_t* list, int32_t* count, hipStream_t stream) {
    hipLaunchKernelGGL(k_compact_tiles, dim3(1), dim3(kCompactBlock), 0, stream, active, n, list, count);
    return hipGetLastError();
}

}  // namespace ptamd
