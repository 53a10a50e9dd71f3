// pt_debug.hip -- test entry points of libptamd.so: closest hit of caller-supplied rays through the
// same traversal code (pt_device.hpp) and the same node placement the render kernels use; the IEEE
// divide / sqrt cores of pt_device.hpp against the compiler's expansions on enumerated inputs; the spec math and sampling primitives
// of pt_device.hpp on caller-supplied items; shade_hit itself, the vertex that joins them, on caller-supplied items.
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

// input k of enumeration `fn` (PT_MATH_* in pt_api.h) as one or two bit patterns
__device__ __forceinline__ uint32_t math_hash(unsigned long long k, uint32_t salt) {
    return lowbias32(lowbias32((uint32_t)k ^ salt) + 0x9e3779b9u * ((uint32_t)(k >> 32) + 1u));
}
__device__ __forceinline__ void math_input(int fn, unsigned long long k, uint32_t* a, uint32_t* b) {
    *b = 0x3f800000u;
    if (fn == PT_MATH_SQRT || fn == PT_MATH_RSQRT) {
        *a = (uint32_t)k;
    } else if (fn == PT_MATH_DIV_GRID) {          // every exponent pair x 8 x 8 mantissas x 4 signs
        const uint32_t ea = (uint32_t)(k & 255), eb = (uint32_t)((k >> 8) & 255), ia = (uint32_t)((k >> 16) & 7),
                       ib = (uint32_t)((k >> 19) & 7), sg = (uint32_t)((k >> 22) & 3);
        const uint32_t h = math_hash(k, 0x51ed270bu);
        const uint32_t mant[8] = {0u, 1u, 2u, 0x400000u, 0x7ffffeu, 0x7fffffu, h & 0x7fffffu, (h >> 9) & 0x7fffffu};
        *a = ((sg & 1u) << 31) | (ea << 23) | mant[ia];
        *b = ((sg >> 1) << 31) | (eb << 23) | mant[ib];
    } else if (fn == PT_MATH_DIV_RANDOM) {        // any bit patterns
        *a = math_hash(k, 0x2545f491u);
        *b = math_hash(k, 0x9e3779b9u);
    } else {                                      // PT_MATH_DIV_NORMAL: normal pairs, exponents 2^-63 .. 2^63
        const uint32_t h1 = math_hash(k, 0x68e31da4u), h2 = math_hash(k, 0xb5297a4du);
        *a = (h1 & 0x807fffffu) | ((64u + ((h1 >> 23) & 127u)) << 23);
        *b = (h2 & 0x807fffffu) | ((64u + ((h2 >> 23) & 127u)) << 23);
    }
}
__device__ __forceinline__ bool math_special(float x) { return !(__builtin_fabsf(x) >= 0x1p-126f) || __builtin_isinf(x); }

// out[0] mismatches, out[1] inputs inside the core's window; bad[2 j], bad[2 j + 1]: the first inputs that mismatched.
// A mismatch is a core result (inside the window) or a wave-level result (div_rn / sqrt_rn / rsqrt_rn, whichever path its
// wave took) that differs in any bit from the compiler's expansion, or a window that admits a zero, denormal, inf or NaN.
__global__ void __launch_bounds__(256) k_debug_math(int fn, unsigned long long first, unsigned long long n, unsigned long long* out, uint32_t* bad,
                                                    long long bad_cap) {
    unsigned long long miss = 0, inside = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        uint32_t ua, ub;
        math_input(fn, first + i, &ua, &ub);
        const float a = __uint_as_float(ua), b = __uint_as_float(ub);
        bool win, bad_lane;
        if (fn == PT_MATH_SQRT) {
            const float ref = __builtin_sqrtf(a);
            win = a >= kSqrtWindowLo;
            bad_lane = (win && __float_as_uint(sqrt_core(a)) != __float_as_uint(ref)) || __float_as_uint(sqrt_rn(a)) != __float_as_uint(ref);
        } else if (fn == PT_MATH_RSQRT) {
            const float ref = 1.0f / __builtin_sqrtf(a);
            win = rsqrt_window(a);
            bad_lane = (win && __float_as_uint(rsqrt_core(a)) != __float_as_uint(ref)) || __float_as_uint(rsqrt_rn(a)) != __float_as_uint(ref);
        } else {
            const float ref = a / b, r0 = __builtin_amdgcn_rcpf(b);
            win = div_window(b, r0, a * r0);
            bad_lane = (win && (math_special(a) || math_special(b) || __float_as_uint(div_core(a, b, r0)) != __float_as_uint(ref))) ||
                       __float_as_uint(div_rn(a, b)) != __float_as_uint(ref);
        }
        inside += win;
        if (bad_lane) {
            ++miss;
            const long long j = (long long)atomicAdd(&out[2], 1ull);
            if (j < bad_cap) {
                bad[2 * j] = ua;
                bad[2 * j + 1] = ub;
            }
        }
    }
    atomicAdd(&out[0], miss);
    atomicAdd(&out[1], inside);
}

// PT_MATH_LCG, a kernel of its own so that k_debug_math stays as it is: lcg_rand on seed = the input's low 32 bits against the
// 64-bit multiply and remainder of prog.cl:72-77 written out (for seed >= 0 -- out[1] counts those -- a different formulation of the
// same operation: lcg_rand reduces by the Mersenne modulus by hand).  out[] as in k_debug_math; bad[2 j] = seed, bad[2 j + 1] = the
// new seed lcg_rand left.
__global__ void __launch_bounds__(256) k_debug_math_lcg(unsigned long long first, unsigned long long n, unsigned long long* out, uint32_t* bad,
                                                        long long bad_cap) {
    unsigned long long miss = 0, inside = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const int seed0 = (int)(uint32_t)(first + i);
        int seed = seed0;
        const float rnd = lcg_rand(seed);
        const unsigned long long ref = (unsigned long long)(long long)seed0 * 48271ull % 2147483647ull;
        inside += seed0 >= 0;
        if ((unsigned long long)(uint32_t)seed != ref || __float_as_uint(rnd) != __float_as_uint((float)ref / 2147483648.0f)) {
            ++miss;
            const long long j = (long long)atomicAdd(&out[2], 1ull);
            if (j < bad_cap) {
                bad[2 * j] = (uint32_t)seed0;
                bad[2 * j + 1] = (uint32_t)seed;
            }
        }
    }
    atomicAdd(&out[0], miss);
    atomicAdd(&out[1], inside);
}

hipError_t launch_debug_math(int fn, unsigned long long first, unsigned long long n, unsigned long long* out, uint32_t* bad, long long bad_cap, int cu_count,
                             hipStream_t stream) {
    const unsigned long long blocks = std::min<unsigned long long>((n + 255) / 256, (unsigned long long)cu_count * 32);
    if (blocks == 0) return hipSuccess;
    if (fn == PT_MATH_LCG) hipLaunchKernelGGL(k_debug_math_lcg, dim3((unsigned)blocks), dim3(256), 0, stream, first, n, out, bad, bad_cap);
    else hipLaunchKernelGGL(k_debug_math, dim3((unsigned)blocks), dim3(256), 0, stream, fn, first, n, out, bad, bad_cap);
    return hipGetLastError();
}

// pt_debug_spec: function FN (PT_SPEC_* in pt_api.h) of pt_device.hpp on item i = the thread's index; spec_words_in(FN) words in and
// spec_words_out(FN) out per item, floats as their bit patterns.
// Item layout, which the callers' wave tests depend on: one thread per item, blocks of 256, no grid-stride loop -- item i runs on lane
// i % 64 of wave i / 64, and the lanes of the last wave past n have left before any wave-level vote (wave_all) is taken.
template <int FN>
__global__ void __launch_bounds__(256) k_debug_spec(const uint32_t* __restrict__ in, long long n, uint32_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t* a = in + i * spec_words_in(FN);
    uint32_t* o = out + i * spec_words_out(FN);
    const auto f = [a](int k) { return __uint_as_float(a[k]); };
    const auto v = [a](int k) { return mk(__uint_as_float(a[k]), __uint_as_float(a[k + 1]), __uint_as_float(a[k + 2])); };
    if constexpr (FN == PT_SPEC_SINCOS || FN == PT_SPEC_SINCOS_SK) {
        float s, c;
        spec_sincos<FN == PT_SPEC_SINCOS_SK>(f(0), &s, &c);
        o[0] = __float_as_uint(s);
        o[1] = __float_as_uint(c);
    } else if constexpr (FN == PT_SPEC_POW || FN == PT_SPEC_POW_SK) {
        o[0] = __float_as_uint(spec_pow<FN == PT_SPEC_POW_SK>(f(0), f(1)));
    } else if constexpr (FN == PT_SPEC_POW5) {
        o[0] = __float_as_uint(spec_pow5(f(0)));
    } else if constexpr (FN == PT_SPEC_LCG) {
        int seed = (int)a[0];
        const float rnd = lcg_rand(seed);
        o[0] = (uint32_t)seed;
        o[1] = __float_as_uint(rnd);
    } else if constexpr (FN == PT_SPEC_FRESNEL) {
        const f3 F = fresnel(v(0), v(3), v(6));
        o[0] = __float_as_uint(F.x);
        o[1] = __float_as_uint(F.y);
        o[2] = __float_as_uint(F.z);
    } else {                                      // the new ray of a diffuse hit at P with normal N, as shade_hit builds it
        constexpr bool SK = FN == PT_SPEC_DIFFUSE_SK || FN == PT_SPEC_DIFFUSE_REC_SK;
        const f3 P = v(0), N = v(3);
        const float rnd1 = f(6), rnd2 = f(7);
        f3 d;
        if constexpr (FN == PT_SPEC_DIFFUSE_REC || FN == PT_SPEC_DIFFUSE_REC_SK) {
            f3 Z, X;
            tangent_frame(N, &Z, &X);
            const float4 frame[2] = {make_float4(Z.x, Z.y, Z.z, X.x), make_float4(X.y, X.z, 0.0f, 0.0f)};      // ShadeRec::frame[o]
            d = diffuse_direction_rec<SK>(N, frame, rnd1, rnd2);
        } else {
            d = diffuse_direction<SK>(N, rnd1, rnd2);
        }
        const f3 D = normalize3(d), O = madd(N, 0.001f, P);
        o[0] = __float_as_uint(O.x);
        o[1] = __float_as_uint(O.y);
        o[2] = __float_as_uint(O.z);
        o[3] = 0u;
        o[4] = __float_as_uint(D.x);
        o[5] = __float_as_uint(D.y);
        o[6] = __float_as_uint(D.z);
        o[7] = 0u;
    }
}

hipError_t launch_debug_spec(int fn, const uint32_t* in, int64_t n, uint32_t* out, hipStream_t stream) {
    using Kernel = void (*)(const uint32_t*, long long, uint32_t*);
    static const Kernel kernels[] = {k_debug_spec<PT_SPEC_SINCOS>,      k_debug_spec<PT_SPEC_SINCOS_SK>,  k_debug_spec<PT_SPEC_POW>,
                                     k_debug_spec<PT_SPEC_POW_SK>,      k_debug_spec<PT_SPEC_POW5>,       k_debug_spec<PT_SPEC_LCG>,
                                     k_debug_spec<PT_SPEC_DIFFUSE>,     k_debug_spec<PT_SPEC_DIFFUSE_SK>, k_debug_spec<PT_SPEC_DIFFUSE_REC>,
                                     k_debug_spec<PT_SPEC_DIFFUSE_REC_SK>, k_debug_spec<PT_SPEC_FRESNEL>};
    if (fn < 0 || fn > PT_SPEC_FRESNEL) return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(kernels[fn], dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in, (long long)n, out);
    return hipGetLastError();
}

// pt_debug_shade: shade_hit<SK, REC> (NoShadeHook) on item i = the thread's index, kShadeWordsIn words in and kShadeWordsOut out per
// item (layout in pt_api.h), floats as their bit patterns.  The host has checked every ti against p.n_tris.
// Item layout as in k_debug_spec, which the callers' wave tests depend on: one thread per item, blocks of 256, no grid-stride loop --
// item i runs on lane i % 64 of wave i / 64, and the lanes past n have left before shade_hit takes any wave-level vote.
template <bool SK, bool REC>
__global__ void __launch_bounds__(256) k_debug_shade(RenderParams p, const uint32_t* __restrict__ in, long long n, uint32_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t* a = in + i * kShadeWordsIn;
    uint32_t* o = out + i * kShadeWordsOut;
    const auto v = [a](int k) { return mk(__uint_as_float(a[k]), __uint_as_float(a[k + 1]), __uint_as_float(a[k + 2])); };
    const auto put = [o](int k, f3 w) {
        o[k] = __float_as_uint(w.x);
        o[k + 1] = __float_as_uint(w.y);
        o[k + 2] = __float_as_uint(w.z);
    };
    f3 P = v(0), D = v(3);
    const float t = __uint_as_float(a[6]);
    const int ti = (int)a[7];
    int seed = (int)a[8];
    bool inside = a[9] != 0u;
    PathRegs st;
    st.fL = v(10);
    st.fB = v(13);
    st.fS = v(16);
    st.fR = v(19);
    st.color = v(22);
    shade_hit<SK, REC>(P, D, st, seed, inside, p, p.tris, p.meta, ti, t);
    put(0, P);
    put(3, D);
    o[6] = (uint32_t)seed;
    o[7] = inside ? 1u : 0u;
    put(8, st.fL);
    put(11, st.fB);
    put(14, st.fS);
    put(17, st.fR);
    put(20, st.color);
}

hipError_t launch_debug_shade(const RenderParams& p, int instance, const uint32_t* in, int64_t n, uint32_t* out, hipStream_t stream) {
    using Kernel = void (*)(RenderParams, const uint32_t*, long long, uint32_t*);
    static const Kernel kernels[] = {k_debug_shade<false, false>, k_debug_shade<true, false>, k_debug_shade<false, true>, k_debug_shade<true, true>};
    if (instance < 0 || instance > (PT_SHADE_SK | PT_SHADE_REC)) return hipErrorInvalidValue;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(kernels[instance], dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p, in, (long long)n, out);
    return hipGetLastError();
}

}  // namespace ptamd
