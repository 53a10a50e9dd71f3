// pt_device.hpp -- gfx950 device code shared by the kernel translation units of libptamd.so
// (pt_kernels.hip: megakernel; pt_wavefront.hip: stream-compacted variant; pt_debug.hip: test entry
// points).  Everything here is __device__ __forceinline__, except the host launcher of the per-lane
// traversal kernels (launch_lanes).
//
// Arithmetic: compiled with -ffp-contract=off; the only fused operations are the explicit fma calls,
// placed as DESIGN.md section 3 prescribes, so that results can be compared bit for bit with the CPU
// oracle (-fno-slp-vectorize: packed f32 ops cost what two scalar ones do, plus the shuffles).  '/'
// and sqrt are IEEE (hipcc default for HIP), sin/cos/pow are the double-precision polynomial routines
// below.  Box tests are NOT part of that contract: they are conservative (padded boxes, widened
// slabs) and only ever cull what the exact triangle test would reject.
#pragma once

#include "pt_internal.hpp"

#include <algorithm>

// A/B switch of the slab test for nodes read from global memory (1: one fma per plane, planes picked
// by the sign of the direction; 0: round 1's (plane - P) * inv with min/max)
#ifndef PT_GLOBAL_SLAB_FMA
#define PT_GLOBAL_SLAB_FMA 1
#endif
// A/B switch of the 4-wide node visit (1: round 3's form -- decode, then slab test; 0: round 4's, see wide_step)
#ifndef PT_WIDE_STEP_V1
#define PT_WIDE_STEP_V1 0
#endif
// A/B switches: Trav::round ends a phase early when few lanes are still in it (see round()), per node path
#ifndef PT_PHASE_SWITCH_GLOBAL
#define PT_PHASE_SWITCH_GLOBAL 1
#endif
#ifndef PT_PHASE_SWITCH_LDS
#define PT_PHASE_SWITCH_LDS 1
#endif
#ifndef PT_WIDE_PREDICATED_STORES
#define PT_WIDE_PREDICATED_STORES 1
#endif

namespace ptamd {

// ---------------------------------------------------------------------------- small math
struct f3 {
    float x, y, z;
};
#define PT_DEV __device__ __forceinline__

PT_DEV f3 mk(float x, float y, float z) { f3 r; r.x = x; r.y = y; r.z = z; return r; }
PT_DEV f3 ldf3(const pt_float3& p) { return mk(p.s[0], p.s[1], p.s[2]); }
PT_DEV f3 operator+(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
PT_DEV f3 operator-(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
PT_DEV f3 operator*(f3 a, f3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
PT_DEV f3 operator*(f3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
PT_DEV f3 operator-(f3 a) { return mk(-a.x, -a.y, -a.z); }
PT_DEV float fmaf_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
PT_DEV double fmad_(double a, double b, double c) { return __builtin_fma(a, b, c); }
// u*s + w, one fma per component
PT_DEV f3 madd(f3 u, float s, f3 w) { return mk(fmaf_(u.x, s, w.x), fmaf_(u.y, s, w.y), fmaf_(u.z, s, w.z)); }
PT_DEV float dot3(f3 a, f3 b) { return fmaf_(a.z, b.z, fmaf_(a.y, b.y, a.x * b.x)); }
PT_DEV f3 cross3(f3 a, f3 b) {
    return mk(fmaf_(a.y, b.z, -(a.z * b.y)), fmaf_(a.z, b.x, -(a.x * b.z)), fmaf_(a.x, b.y, -(a.y * b.x)));
}
// ---- IEEE divide and sqrt without the range handling their operands here almost never need
// hipcc expands a correctly rounded f32 a / b (denormals kept) into
//   d = v_div_scale(b, b, a)   n = v_div_scale(a, b, a) -> VCC   r = v_rcp(d)   e = fma(-d, r, 1)   r = fma(e, r, r)
//   q = n * r   e = fma(-d, q, n)   q = fma(e, r, q)   e = fma(-d, q, n)   q = v_div_fmas(e, r, q) [VCC]   v_div_fixup(q, b, a)
// By the ISA definitions, v_div_scale returns its first operand unchanged and clears VCC unless a or b is zero, inf, NaN
// or denormal, exp(a) - exp(b) >= 96, 1/b or a/b is denormal, or a's biased exponent is <= 23; with VCC clear v_div_fmas
// is v_fma; v_div_fixup returns |q| with the sign of a * b unless an operand is zero, inf or NaN, a is not finite or the
// quotient underflows past 2^-150.  div_window() below admits only pairs where none of that applies (|b| and |1/b| at
// most 2^40, so b is normal; the quotient between 2^-40 and 2^40, so a is normal, within 2^81 of b, and neither zero
// nor inf) -- and there the core sequence, which is what is left, gives the same bits as '/'.  The sqrt expansion is
//   s = v_sqrt(x') on x' = x < 2^-96 ? x * 2^32 : x, then s -/+ 1 ulp when fma(-(s -/+ 1 ulp), s, x') is <= 0 / > 0,
//   then * 2^-16 if x was scaled, then x' itself if x' is +-0 or +inf;
// for x >= 2^-96 neither scale applies and +inf comes out of the core as inf, so the core alone is exact.
// Callers take the core when every active lane of the wave is in the window (one uniform branch) and the compiler's
// expansion otherwise: both give the same bits, so lanes never see which one ran.  tests/test_gpu_fast_math.py checks
// each core against the expansion on every input of its window edges (pt_debug_math).
constexpr float kDivWindow = 0x1p40f, kDivWindowLo = 0x1p-40f, kSqrtWindowLo = 0x1p-96f;
// A/B switch: 0 picks core or expansion once per wave (a ballot, one uniform branch); 1 per lane (a wave with lanes on both
// sides runs both under exec masks).  profiles/fastmath/README.md compares them.
#ifndef PT_FASTMATH_PER_LANE
#define PT_FASTMATH_PER_LANE 0
#endif
PT_DEV bool wave_all(bool c) { return PT_FASTMATH_PER_LANE ? c : __builtin_amdgcn_ballot_w64(!c) == 0; }
// r0 = v_rcp(b), q0 = a * r0 (both as the caller may already hold them)
PT_DEV bool div_window(float b, float r0, float q0) {
    return __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(b), __builtin_fabsf(r0)), __builtin_fabsf(q0)) <= kDivWindow &&
           __builtin_fabsf(q0) >= kDivWindowLo;
}
PT_DEV float div_core(float a, float b, float r0) {
    const float r = fmaf_(fmaf_(-b, r0, 1.0f), r0, r0);
    float q = a * r;
    q = fmaf_(fmaf_(-b, q, a), r, q);
    return fmaf_(fmaf_(-b, q, a), r, q);
}
PT_DEV float sqrt_core(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float sm = __int_as_float(__float_as_int(s) - 1), sp = __int_as_float(__float_as_int(s) + 1);
    const float t = fmaf_(-sm, s, x) <= 0.0f ? sm : s;
    return fmaf_(-sp, s, x) > 0.0f ? sp : t;
}
// a / b, bit for bit
PT_DEV float div_rn(float a, float b) {
    const float r0 = __builtin_amdgcn_rcpf(b);
    if (wave_all(div_window(b, r0, a * r0))) return div_core(a, b, r0);
    return a / b;
}
// sqrtf(x), bit for bit
PT_DEV float sqrt_rn(float x) {
    if (wave_all(x >= kSqrtWindowLo)) return sqrt_core(x);
    return __builtin_sqrtf(x);
}
// 1.0f / sqrtf(x), two roundings, bit for bit: for finite x >= 2^-96 the root b lies in [2^-48, 2^64].  With numerator 1
// none of the scaling conditions above applies there (exp(1) - exp(b) <= 48 < 96; 1/b >= 2^-64 is normal, so is 1/b as the
// quotient; exp(1) = 127 > 23) and v_div_fixup has no special case to take, so the divide core is exact on the whole
// range -- a wider range than div_window's, which has to bound a general numerator.  One compare pair covers both cores.
PT_DEV bool rsqrt_window(float x) { return x >= kSqrtWindowLo && x < __builtin_inff(); }
PT_DEV float rsqrt_core(float x) {
    const float s = sqrt_core(x);
    return div_core(1.0f, s, __builtin_amdgcn_rcpf(s));
}
PT_DEV float rsqrt_rn(float x) {
    if (wave_all(rsqrt_window(x))) return rsqrt_core(x);
    return 1.0f / __builtin_sqrtf(x);
}
PT_DEV f3 normalize3(f3 a) {
    const float s = rsqrt_rn(dot3(a, a));
    return a * s;
}
PT_DEV float max0(float c) { return c > 0.0f ? c : 0.0f; }

// ---- spec math: double polynomials, rounded once to float
// The polynomial coefficients are 64-bit literals, which no gfx950 VALU instruction can encode: left alone, the compiler
// keeps each in a VGPR pair for the whole kernel (hoisted out of every loop) and, in the instances with 72-96 VGPRs,
// spills them -- ten 8-byte scratch reloads per lane in front of every cosine-sampled direction, each wave with its own
// copy of the same constants (~180 KB per CU fighting the nodes for L1 / L2).  KC<true>() pins a coefficient to a scalar
// register pair at its point of use instead: two s_mov_b32 with literal operands, then v_fma_f64 reads the pair directly.
// SK = false leaves the constants to the compiler: the 128-VGPR instance (whole tree in LDS) has room for them and is
// 1 % faster that way (profiles/r03/d_*).
template <bool SK, unsigned long long BITS>
PT_DEV double kc_bits() {
    if (SK) {
        // (the literal is written by the asm itself: with the constant as an INPUT of an empty asm the compiler hoisted its
        // materialisation out of the sample loop, ran out of scalar registers and kept it in VGPR lanes -- two v_readlane and two
        // v_writelane per use, ~50 VALU instructions per cosine-sampled direction, profiles/r03/y_*)
        unsigned lo, hi;
        asm volatile("s_mov_b32 %0, %2\n\ts_mov_b32 %1, %3" : "=s"(lo), "=s"(hi) : "i"((unsigned)(BITS & 0xffffffffull)), "i"((unsigned)(BITS >> 32)));
        return __longlong_as_double((long long)(((unsigned long long)hi << 32) | (unsigned long long)lo));
    }
    return __builtin_bit_cast(double, BITS);
}
#define KC_(SK, x) kc_bits<SK, __builtin_bit_cast(unsigned long long, (double)(x))>()
// a * b + K.  (Left to the compiler, a Horner step becomes v_fmac_f64 with the constant as the accumulator -- which has to be a VGPR
// pair: two v_mov_b32 from the scalar pair per step, 46 per cosine-sampled direction.  v_fma_f64 takes the pair as it is.)
template <bool SK, unsigned long long BITS>
PT_DEV double fmad_k(double a, double b) {
    if (SK) {
        const double k = kc_bits<SK, BITS>();
        double r;
        asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(k));
        return r;
    }
    return fmad_(a, b, __builtin_bit_cast(double, BITS));
}
#define FMADK(SK, a, b, x) fmad_k<SK, __builtin_bit_cast(unsigned long long, (double)(x))>(a, b)
template <bool SK>
PT_DEV void spec_sincos(float theta, float* s, float* c) {
    const double t = (double)theta;
    const int q = (int)fmad_(t, KC_(SK, 0.63661977236758138), 0.5);
    const double qd = (double)q;
    double r = fmad_(qd, KC_(SK, -1.5707963267948966), t);
    r = fmad_(qd, KC_(SK, -6.123233995736766e-17), r);
    const double z = r * r;
    double ps = KC_(SK, 1.6059043836821613e-10);
    ps = FMADK(SK, ps, z, -2.505210838544172e-08);
    ps = FMADK(SK, ps, z, 2.7557319223985893e-06);
    ps = FMADK(SK, ps, z, -0.0001984126984126984);
    ps = FMADK(SK, ps, z, 0.008333333333333333);
    ps = FMADK(SK, ps, z, -0.16666666666666666);
    const double sr = fmad_(r * z, ps, r);
    double pc = KC_(SK, -1.1470745597729725e-11);
    pc = FMADK(SK, pc, z, 2.08767569878681e-09);
    pc = FMADK(SK, pc, z, -2.755731922398589e-07);
    pc = FMADK(SK, pc, z, 2.48015873015873e-05);
    pc = FMADK(SK, pc, z, -0.001388888888888889);
    pc = FMADK(SK, pc, z, 0.041666666666666664);
    pc = fmad_(pc, z, -0.5);
    const double cr = fmad_(z, pc, 1.0);
    const int k = q & 3;
    const double sv = (k == 0) ? sr : (k == 1) ? cr : (k == 2) ? -sr : -cr;
    const double cv = (k == 0) ? cr : (k == 1) ? -sr : (k == 2) ? -cr : sr;
    *s = (float)sv;
    *c = (float)cv;
}

PT_DEV float spec_pow5(float x) {
    const float x2 = x * x;
    const float x4 = x2 * x2;
    return x4 * x;
}

template <bool SK>
PT_DEV float spec_pow(float x, float y) {
    if (y == 0.0f) return 1.0f;
    if (x != x || y != y) return __builtin_nanf("");
    if (x < 0.0f) return __builtin_nanf("");
    if (x == 0.0f) return y > 0.0f ? 0.0f : __builtin_inff();
    if (__builtin_isinf(x)) return y > 0.0f ? __builtin_inff() : 0.0f;
    const double xd = (double)x;
    unsigned long long bits = (unsigned long long)__double_as_longlong(xd);
    int e = (int)((bits >> 52) & 0x7ff) - 1023;
    bits = (bits & 0x000fffffffffffffull) | 0x3ff0000000000000ull;
    double m = __longlong_as_double((long long)bits);
    if (m > KC_(SK, 1.4142135623730951)) { m = m * 0.5; e += 1; }
    const double f = m - 1.0;
    const double sdiv = f / (2.0 + f);
    const double z = sdiv * sdiv;
    double p = KC_(SK, 0.10526315789473684);
    p = FMADK(SK, p, z, 0.11764705882352941);
    p = FMADK(SK, p, z, 0.13333333333333333);
    p = FMADK(SK, p, z, 0.15384615384615385);
    p = FMADK(SK, p, z, 0.18181818181818182);
    p = FMADK(SK, p, z, 0.22222222222222221);
    p = FMADK(SK, p, z, 0.2857142857142857);
    p = FMADK(SK, p, z, 0.4);
    p = FMADK(SK, p, z, 0.66666666666666663);
    p = fmad_(p, z, 2.0);
    const double lnm = sdiv * p;
    const double lg2 = fmad_(lnm, KC_(SK, 1.4426950408889634), (double)e);
    const double w = (double)y * lg2;
    if (!(w > -126.0)) return 0.0f;
    if (w >= 128.0) return __builtin_inff();
    const double nd = __builtin_floor(w + 0.5);
    const double g = (w - nd) * KC_(SK, 0.6931471805599453);
    double q = KC_(SK, 2.08767569878681e-09);
    q = FMADK(SK, q, g, 2.505210838544172e-08);
    q = FMADK(SK, q, g, 2.755731922398589e-07);
    q = FMADK(SK, q, g, 2.7557319223985893e-06);
    q = FMADK(SK, q, g, 2.48015873015873e-05);
    q = FMADK(SK, q, g, 0.0001984126984126984);
    q = FMADK(SK, q, g, 0.001388888888888889);
    q = FMADK(SK, q, g, 0.008333333333333333);
    q = FMADK(SK, q, g, 0.041666666666666664);
    q = FMADK(SK, q, g, 0.16666666666666666);
    q = fmad_(q, g, 0.5);
    q = fmad_(q, g, 1.0);
    q = fmad_(q, g, 1.0);
    const unsigned long long sb = (unsigned long long)((long long)nd + 1023) << 52;
    const double sc = __longlong_as_double((long long)sb);
    return (float)(q * sc);
}

// ---- LCG, prog.cl:72-77: n = (ulong)seed * 48271 % 2147483647.
// For seed >= 0 the product is < 2^47 and the modulus is the Mersenne number 2^31 - 1:
// n = hi * 2^31 + lo = hi + lo (mod M) with hi < 2^16, so one conditional subtraction finishes it
// (8 32-bit instructions instead of the ~30 of a 64-bit multiply and remainder).  A negative seed
// (only possible for a seed the caller uploaded; every output is in [0, M)) sign-extends to 64 bits
// as in the reference and takes the generic path.
PT_DEV float lcg_rand(int& seed) {
    unsigned n;
    if (seed >= 0) {
        const unsigned s = (unsigned)seed;
        const unsigned plo = s * 48271u, phi = __umulhi(s, 48271u);
        const unsigned t = (plo & 0x7fffffffu) + ((phi << 1) | (plo >> 31));
        n = min(t, t - 2147483647u);
    } else {
        unsigned long long w = (unsigned long long)(long long)seed;
        w = (w * 48271ull) % 2147483647ull;
        n = (unsigned)w;
    }
    seed = (int)n;
    return (float)n / 2147483648.0f;
}

// ---------------------------------------------------------------------------- pixel map
// One wave covers an 8x8 pixel tile of the LOCAL frame (width x local_rows).
struct PixelId {
    int li;   // local pixel index (buffer index), -1 = none
    int gid;  // global pixel id (what prog.cl calls id)
};
PT_DEV PixelId pixel_of_wave(const RenderParams& p, int wave) {
    const int lane = threadIdx.x & 63;
    const int tiles_x = (p.width + 7) >> 3;
    const int ty = wave / tiles_x, tx = wave - ty * tiles_x;
    const int x = tx * 8 + (lane & 7);
    const int lrow = ty * 8 + (lane >> 3);
    PixelId r;
    if (x >= p.width || lrow >= p.local_rows) {
        r.li = -1;
        r.gid = 0;
        return r;
    }
    const int grow = global_row(p, lrow);
    r.li = lrow * p.width + x;
    r.gid = grow * p.width + x;
    return r;
}

// Tile t of a launch -> tile of the local frame: t itself, or the t-th entry of an adaptive frame's list of active tiles
// (p.tile_list, pt_render_adaptive).  t is wave-uniform and so is the answer (scalar registers); a t past the list -- the last
// workgroup of a non-persistent grid -- becomes the first tile below the frame, which has no pixels.
PT_DEV int frame_tile(const RenderParams& p, int t) {
    if (!p.tile_list) return t;
    if (t >= p.n_tiles) return ((p.width + 7) >> 3) * ((p.local_rows + 7) >> 3);
    return __builtin_amdgcn_readfirstlane(p.tile_list[t]);
}

PT_DEV PixelId pixel_of_thread(const RenderParams& p) {
    return pixel_of_wave(p, (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
}

// ---------------------------------------------------------------------------- camera, prog.cl:82-92
// (px, py) = (float)(id % X), (float)(id / X): fixed per pixel, so the render kernel computes them once
PT_DEV void camera_get_ray_xy(float px, float py, const pt_camera& cam, float rnd1, float rnd2, f3* P, f3* D) {
    const int X = (int)cam.XM;
    const int Y = (int)cam.YM;
    const float x = px + rnd1;
    const float y = py + rnd2;
    const f3 right = ldf3(cam.right) * ((2.0f * x) / (float)X - 1.0f);
    const f3 up = ldf3(cam.up) * ((2.0f * y) / (float)Y - 1.0f);
    const f3 pp = (ldf3(cam.lookat) + right) + up;
    const f3 eye = ldf3(cam.eye);
    *P = eye;
    *D = normalize3(pp - eye);
}
PT_DEV void camera_get_ray(int id, const pt_camera& cam, float rnd1, float rnd2, f3* P, f3* D) {
    const int X = (int)cam.XM;
    camera_get_ray_xy((float)(id % X), (float)(id / X), cam, rnd1, rnd2, P, D);
}
// The thin-lens ray of the same sub-pixel position (pt_set_lens; include/pt_api.h pins every operation): from a point of the lens disc,
// drawn from two hash values of segment -1 of the complemented key S, through the point in focus on the pinhole ray.  The lens
// instances of k_nee and k_debug_lens call this one function.
PT_DEV void lens_get_ray_xy(float px, float py, const pt_camera& cam, const LensView& lv, float rnd1, float rnd2, unsigned S, f3* P, f3* D) {
    const int X = (int)cam.XM;
    const int Y = (int)cam.YM;
    const float x = px + rnd1;
    const float y = py + rnd2;
    const f3 right = ldf3(cam.right) * ((2.0f * x) / (float)X - 1.0f);
    const f3 up = ldf3(cam.up) * ((2.0f * y) / (float)Y - 1.0f);
    const f3 pp = (ldf3(cam.lookat) + right) + up;
    const f3 eye = ldf3(cam.eye);
    const f3 d = pp - eye;
    const f3 Q = madd(d, lv.focus / dot3(d, mk(lv.f[0], lv.f[1], lv.f[2])), eye);
    const float u1 = (float)(nee_rand(~S, -1, 0) >> 8) * 5.9604644775390625e-08f, u2 = (float)(nee_rand(~S, -1, 1) >> 8) * 5.9604644775390625e-08f;
    const float r = __builtin_sqrtf(u1);
    float sn, cs;
    spec_sincos<false>((float)(6.283185307179586 * (double)u2), &sn, &cs);
    const f3 O = madd(mk(lv.Uh[0], lv.Uh[1], lv.Uh[2]), lv.aperture * (r * sn), madd(mk(lv.Rh[0], lv.Rh[1], lv.Rh[2]), lv.aperture * (r * cs), eye));
    *P = O;
    *D = normalize3(Q - O);
}

// ---------------------------------------------------------------------------- traversal
// dynamic LDS of every traversal kernel: [per-lane stacks][staged nodes][big-triangle list] (setup_traversal)
extern __shared__ __attribute__((aligned(16))) unsigned char pt_lds_raw[];

// Where the BVH nodes are read from (template parameter of Trav and of the kernels):
//   kNodesLds      every node is staged in LDS by the workgroup (stage_nodes), re-laid out for the
//                  ray (swizzled box quads, 16-bit child references, 16-bit stack entries).  Scenes
//                  of up to ~1,000 nodes (Cornell box: 941).
//   kNodesGlobal   nodes are read from global memory (L1/L2) as the host packed them.
//   kNodesTreelet  the top `treelet` nodes of a large tree -- the host re-indexes the tree so that
//                  the nodes with the largest boxes are nodes [0, treelet) -- are staged in LDS AS THEY
//                  ARE, the rest stays in global memory, and a visit reads its node through a generic
//                  (flat) pointer that each lane points at its LDS copy or at global memory: one
//                  instruction stream for both, no divergence between lanes above and below the cut.
//                  References stay 32-bit.  MESH-100k / MESH-1M (50 k / 505 k nodes).
struct SceneView {
    const float4* nodes;       // global memory, host layout (unused by kNodesLds)
    const float4* lds_nodes;   // staged copy (kNodesLds: all nodes; kNodesTreelet: nodes [0, treelet))
    const float4* tris;        // packets, global memory
    const TriMeta* meta;       // global memory
    unsigned treelet;          // kNodesTreelet: node indices below this are read from lds_nodes
    int n_flat;                // packets [0, n_flat): big triangles kept out of the tree, tested first (flat_pass)
    const float4* lds_flat;    // their packets, staged in LDS
    int n_fbox;                // their distinct padded boxes (the halves of a wall share one) ...
    const char* lds_fbox;      // ... 48 B each: per axis {lo, hi, hi, lo} (planes picked by address, like a staged node)
    const unsigned* lds_fmask; // ... and which listed triangles each one covers
    unsigned fpair;            // bit i: listed triangles i and i + 1 are a coplanar pair with the same N and r1 words in lds_flat, i its
                               // head (pt_builder.cpp plan_flat_pairs); wave-uniform, read by kNodesLds only
    // kNodesWide: the lane's stack continues in global memory past its LDS entries (a 4-wide traversal can have three
    // children pending per level, far more than it usually has; LDS holds what keeps six waves per SIMD resident)
    // (all three wave-uniform, i.e. scalar registers: which entry an address is, and whose, is read off the address
    // itself -- the stacks start at LDS offset 0, entry k of lane l at (k * BLOCK + l) * 4 -- so that no per-lane
    // pointer rides through the traversal)
    // phase switching of Trav::round (wave-uniform): the node phase ends early when at most node_min_lanes lanes still descend
    // and another lane holds a leaf; the leaf phase when at most leaf_min_lanes lanes still hold leaves and another has a node
    int node_min_lanes, leaf_min_lanes;
    int lds_entries;           // entries per lane in LDS
    unsigned* ovf;             // entry (lds_entries + j) of lane l of this workgroup = ovf[j * ovf_stride + l]
    unsigned ovf_stride;
};

struct WorkCount {
    unsigned nodes, tris;     // per-lane visits / tests
    unsigned wnodes, wtris;   // wave-level executions of the two bodies (counted by the first active lane)
    unsigned wshade, wtrips, wrounds;   // wave-level executions of shade_hit, of the segment loop body, of Trav::round
    unsigned low[6];                    // ... of those that ran for at most 8 lanes: node body, triangle body, its exact part, shade_hit, the
                                        // big-triangle list's exact tests (all of them in low[5])
};
// counting instances: one more execution of body `which` (first active lane only), noting whether it ran for at most 8 lanes
PT_DEV void count_low(WorkCount* wc, int which) {
    const unsigned long long m = __ballot(1);
    if ((int)(threadIdx.x & 63) == __ffsll((long long)m) - 1 && __popcll(m) <= 8) wc->low[which]++;
}
PT_DEV bool first_active_lane() {
    const unsigned long long m = __ballot(1);
    return (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1;
}

// prog.cl:94-112 on one packet; returns t (> 0) or -1.  `limit` is the current closest t: a
// triangle whose t is clearly larger can neither win nor tie, so it is dropped before the exact
// (IEEE-divide) evaluation.  Both early-outs are conservative: whatever the exact test would
// accept with t <= best_t passes them (t > 0 needs num and den of the same non-zero sign; the
// reciprocal estimate is within 2 ulp and the margin is 16 ulp).
// QUOT picks how the two early-outs are evaluated (same accepted set up to harmless extras):
//   true : from the estimated quotient alone, q = num * rcp(den): not negative and not above the
//          limit (q = 0, -0 and NaN pass and are sorted out by the exact evaluation) -- fewest VALU
//          instructions, +2.7 % on the VALU-bound LDS node path;
//   false: four sign compares first, the reciprocal only for same-sign pairs -- 3 % faster on the
//          L1/L2 node path, where the 8-clock v_rcp on every test costs more than it saves.
template <bool QUOT>
PT_DEV float tri_test(const float4 a, const float4 b, const float4 c, f3 P, f3 Vd, float limit, WorkCount* wc = nullptr) {
    const f3 r1 = mk(a.x, a.y, a.z), r2 = mk(a.w, b.x, b.y), r3 = mk(b.z, b.w, c.x), N = mk(c.y, c.z, c.w);
    const float num = dot3(r1 - P, N), den = dot3(Vd, N);
    float res = -1.0f;
    bool cand;
    if (QUOT) {
        const float q = num * __builtin_amdgcn_rcpf(den);
        cand = !(q < 0.0f) && !(q > limit);
    } else {
        const bool same_sign = (num > 0.0f && den > 0.0f) || (num < 0.0f && den < 0.0f);
        cand = same_sign && num * __builtin_amdgcn_rcpf(den) <= limit;
    }
    if (cand) {
        if (wc) { count_low(wc, 2); if (first_active_lane()) wc->low[5]++; }
        // num / den (div_rn).  Under QUOT the rcp and the quotient estimate here are the early-out's, merged by the compiler
        // (same operands, and the early-out's dominate); under !QUOT the early-out's rcp ran inside the `&&` and is evaluated again
        const float r0 = __builtin_amdgcn_rcpf(den);
        const float t = wave_all(div_window(den, r0, num * r0)) ? div_core(num, den, r0) : num / den;
        const f3 pt = madd(Vd, t, P);
        const float c1 = dot3(cross3(r2 - r1, pt - r1), N);
        const float c2 = dot3(cross3(r3 - r2, pt - r2), N);
        const float c3 = dot3(cross3(r1 - r3, pt - r3), N);
        const bool ok = !(t < 0.0f) && (c1 >= 0.0f) && (c2 >= 0.0f) && (c3 >= 0.0f) && (t > 0.0f);
        res = ok ? t : -1.0f;
    }
    return res;
}

// tri_test<QUOT> on the two halves of a wall at once: packets pk[0..2] (A) and pk[3..5] (B) whose N words and r1 words are the
// same (the host's pairing, plan_flat_pairs).  Everything tri_test derives from r1, N and the ray -- num, den, the early-out,
// the reciprocal, the quotient t and the point pt -- is the same IEEE operations on the same bits for both, so it is evaluated
// once; only the edge functions differ, each written exactly as in tri_test.  *tA / *tB: what tri_test returns for A / B when
// both are called with this `limit`.  (Called one after the other, B would see the limit A's hit leaves behind: a smaller one,
// which can only turn a B that no longer wins or ties into an early -1 -- the caller's keep-closest logic ignores it either way.)
// B's words are read after A's edge functions, so that the two triangles' corners need not be live together.
template <bool QUOT>
PT_DEV void tri_test_pair(const float4* pk, f3 P, f3 Vd, float limit, WorkCount* wc, float* tA, float* tB) {
    const float4 a = pk[0], b = pk[1], c = pk[2];
    const f3 r1 = mk(a.x, a.y, a.z), r2 = mk(a.w, b.x, b.y), r3 = mk(b.z, b.w, c.x), N = mk(c.y, c.z, c.w);
    const float num = dot3(r1 - P, N), den = dot3(Vd, N);
    float resA = -1.0f, resB = -1.0f;
    bool cand;
    if (QUOT) {
        const float q = num * __builtin_amdgcn_rcpf(den);
        cand = !(q < 0.0f) && !(q > limit);
    } else {
        const bool same_sign = (num > 0.0f && den > 0.0f) || (num < 0.0f && den < 0.0f);
        cand = same_sign && num * __builtin_amdgcn_rcpf(den) <= limit;
    }
    if (cand) {
        if (wc) { count_low(wc, 2); if (first_active_lane()) wc->low[5]++; }
        const float r0 = __builtin_amdgcn_rcpf(den);
        const float t = wave_all(div_window(den, r0, num * r0)) ? div_core(num, den, r0) : num / den;
        const f3 pt = madd(Vd, t, P);
        const bool front = !(t < 0.0f) && (t > 0.0f);
        {
            const float c1 = dot3(cross3(r2 - r1, pt - r1), N);
            const float c2 = dot3(cross3(r3 - r2, pt - r2), N);
            const float c3 = dot3(cross3(r1 - r3, pt - r3), N);
            resA = (front && (c1 >= 0.0f) && (c2 >= 0.0f) && (c3 >= 0.0f)) ? t : -1.0f;
        }
        {
            const float w = pk[3].w, x = pk[5].x;
            const float4 e = pk[4];
            const f3 s2 = mk(w, e.x, e.y), s3 = mk(e.z, e.w, x);
            const float c1 = dot3(cross3(s2 - r1, pt - r1), N);
            const float c2 = dot3(cross3(s3 - s2, pt - s2), N);
            const float c3 = dot3(cross3(r1 - s3, pt - s3), N);
            resB = (front && (c1 >= 0.0f) && (c2 >= 0.0f) && (c3 >= 0.0f)) ? t : -1.0f;
        }
    }
    *tA = resA;
    *tB = resB;
}

// Per-lane traversal stack in LDS, laid out [entry][lane] (consecutive lanes -> consecutive
// banks).  Entry 0 holds a "finished" sentinel, so popping never has to test for an empty stack.
template <class T>
struct LaneStack {
    T* base;        // already offset by the lane
    int stride;     // entries are `stride` elements apart
};

enum : int { kVisitLds = 0, kVisitGlobal = 1, kVisitFlat = 2 };      // Trav::node_step

template <int MODE> struct StackOf { typedef unsigned type; };
template <> struct StackOf<kNodesLds> { typedef unsigned short type; };

// Closest hit over the whole scene; ties in t go to the lower encounter rank (the triangle the
// reference's traversal, prog.cl:113-184, meets first).
// While-while traversal, one "round" at a time: every lane first descends through interior nodes
// until it holds a leaf (or has finished), then all lanes holding leaves intersect them.  The
// per-lane state survives between rounds so that a flat loop can hand a finished lane its next ray
// while the others keep going (wf_intersect).
//
// Node references (`cur`, child slots, stack entries):
//   kNodesGlobal / kNodesTreelet   as the host packs them: >= 0 interior index, < 0 leaf
//                                  ~(first << 3 | count - 1), kDone finished; 32-bit stack entries
//   kNodesLds                      re-encoded to 16 bits by stage_nodes(): < 0x7fff interior index,
//                                  0x7fff finished, 0x8000 | (first << 3 | count - 1) leaf -- nothing
//                                  to encode or decode on a push or pop; 16-bit stack entries
template <int MODE>
struct Trav {
    typedef typename StackOf<MODE>::type StackT;
    static constexpr bool kRef16 = MODE == kNodesLds;
    static constexpr bool kDefer = MODE != kNodesLds;     // see node_step
    static constexpr bool kPhaseSwitch = MODE == kNodesLds ? (PT_PHASE_SWITCH_LDS != 0) : (PT_PHASE_SWITCH_GLOBAL != 0);   // see round()
    static constexpr int kDone = kRef16 ? 0x7fff : 0x7fffffff;
    f3 P, D, inv;
    float best_t;
    int best;      // packed triangle index of the closest hit so far, -1 none
    char* tos;     // top of this lane's stack (entry 0 = sentinel kDone), as a byte address
    int stride;    // bytes between entries
    int cur;
    int pend;      // round(): a leaf met during the node phase and not yet intersected (0: none)
    int onx, ony, onz;   // kNodesLds only: byte offset of the entry-plane pair of each axis inside a staged node; 8 / 24 / 40 = direction
                         // negative.  The other modes read the sign bits of `inv` where they need them (ox / oy / oz, negx / negy /
                         // negz): three registers fewer across a traversal, at the same instruction count
    f3 cn, cf;           // -(P * inv) widened down / up (entry / exit distance = fma(plane, inv, c))

    PT_DEV static bool is_node(int c) { return kRef16 ? c < 0x7fff : (unsigned)c < 0x7fffffffu; }
    PT_DEV static bool is_leaf(int c) { return kRef16 ? c > 0x7fff : c < 0; }
    PT_DEV static int leaf_bits(int c) { return kRef16 ? (c & 0x7fff) : ~c; }

    PT_DEV void begin(f3 P_, f3 D_, const LaneStack<StackT> stk) {
        setup(P_, D_);
        restart(stk);
    }
    // the traversal state proper: {best_t, best, tos, cur} (+ the stack itself); everything setup() computes can
    // be recomputed from the ray, which is what lets a suspended traversal resume from four saved values
    PT_DEV void restart(const LaneStack<StackT> stk) {
        best_t = __builtin_inff();
        best = -1;
        tos = reinterpret_cast<char*>(stk.base);
        stride = stk.stride * (int)sizeof(StackT);
        *reinterpret_cast<StackT*>(tos) = (StackT)kDone;
        cur = 0;        // the root is always an interior node
        pend = 0;
    }
    PT_DEV void setup(f3 P_, f3 D_) {
        P = P_;
        D = D_;
        inv = mk(__builtin_amdgcn_rcpf(D_.x), __builtin_amdgcn_rcpf(D_.y), __builtin_amdgcn_rcpf(D_.z));
        if (kRef16) {
            onx = __float_as_int(inv.x) < 0 ? 8 : 0;
            ony = __float_as_int(inv.y) < 0 ? 24 : 16;
            onz = __float_as_int(inv.z) < 0 ? 40 : 32;
        }
        // Distance to a plane as ONE fma: plane * inv - P * inv.  The product P * inv is rounded
        // (half an ulp of |P * inv|, which can dwarf the distance itself), so the entry constant
        // is lowered and the exit constant raised by 4 such half-ulps: entry distances come out
        // too small, exit distances too large, never the other way round.  inf - inf = NaN
        // (direction component 0 or underflowing) is ignored by max3/min3: that slab counts as
        // entered, which only costs work.  This needs the entry / exit plane of an axis to be picked
        // by the SIGN of the direction (by address in LDS, by select for nodes from global memory):
        // with min/max picking them a NaN would be replaced by the other plane's distance and cull
        // real hits (tests/test_gpu_parity.py::test_closest_hit_adversarial_rays).
        const float px = P.x * inv.x, py = P.y * inv.y, pz = P.z * inv.z;
        const float k22 = 2.3841858e-07f;    // 2^-22
        const float ex = __builtin_fabsf(px) * k22, ey = __builtin_fabsf(py) * k22, ez = __builtin_fabsf(pz) * k22;
        cn = mk(-(px + ex), -(py + ey), -(pz + ez));
        cf = mk(-(px - ex), -(py - ey), -(pz - ez));
    }
    PT_DEV bool negx() const { return __float_as_int(inv.x) < 0; }
    PT_DEV bool negy() const { return __float_as_int(inv.y) < 0; }
    PT_DEV bool negz() const { return __float_as_int(inv.z) < 0; }
    PT_DEV int ox() const { return kRef16 ? onx : (negx() ? 8 : 0); }
    PT_DEV int oy() const { return kRef16 ? ony : (negy() ? 24 : 16); }
    PT_DEV int oz() const { return kRef16 ? onz : (negz() ? 40 : 32); }
    PT_DEV void idle() { cur = kDone; }
    PT_DEV bool done() const { return cur == kDone; }

    // One interior-node visit: slab-test both children, descend into the nearer hit one, push the
    // other.  The visit is ONE basic block with one stack round trip: the top of the stack is fetched
    // together with the node (it is the next node if neither child is hit), and the far child is
    // stored above the top unconditionally; only the stack pointer moves conditionally.
    //
    // KIND = kVisitLds: the node is read from the staged copy, whose box quads are swizzled to
    // {L.lo, R.lo, L.hi, R.hi}: the entry / exit planes of both children are picked by ADDRESS from
    // the sign of the ray direction -- 7 8-byte LDS reads, no select (v_min/v_max/v_cndmask are
    // 4-cycle ops on gfx950, tools/micro/exec_ops.hip; the adds that form the addresses are 2-cycle
    // ops).  kVisitGlobal / kVisitFlat: the node comes as four 16-byte loads {L.lo, L.hi, R.lo, R.hi}
    // (narrow per-lane global loads cost per instruction and lane, not per byte: 7 of them ran at
    // 0.74-0.80x, profiles/r01/r_*) and the planes are picked by 12 selects; kVisitFlat loads through a
    // generic pointer that is the lane's LDS copy for nodes of the treelet and global memory below it.
    //
    // DEFER (nodes from global memory): when the nearer child is a leaf and no leaf is pending, the
    // leaf is remembered and the descent goes on with the other child or the stack; round()
    // intersects it after the node phase.  A lane then goes through about half as many node-phase /
    // leaf-phase alternations, each of which the whole wave waits out -- at the price of 3 % more
    // node visits (the pending leaf cannot prune yet).  Measured: L1/L2 node path +5..8 %, LDS node
    // path +-0 (the 5 extra VALU instructions per visit cost what the saved alternations bring).
    template <bool COUNT, bool DEFER, int KIND>
    PT_DEV void node_step(const SceneView& sv, WorkCount* wc) {
        const float kWiden = 1.0000005f;   // > 4 ulp: covers rcp + fma (begin() covers P * inv)
        const int top = (int)*reinterpret_cast<const StackT*>(tos);
        float ln, lf, rn, rf;
        int li, ri;
        if (COUNT) { wc->nodes++; if (first_active_lane()) wc->wnodes++; count_low(wc, 0); }
        if (KIND == kVisitLds) {
            const char* nb = reinterpret_cast<const char*>(sv.lds_nodes) + (unsigned)cur * (unsigned)kLdsNodeBytes;
            const float2 ex = *reinterpret_cast<const float2*>(nb + onx), xx = *reinterpret_cast<const float2*>(nb + (onx ^ 8));
            const float2 ey = *reinterpret_cast<const float2*>(nb + ony), xy = *reinterpret_cast<const float2*>(nb + (ony ^ 8));
            const float2 ez = *reinterpret_cast<const float2*>(nb + onz), xz = *reinterpret_cast<const float2*>(nb + (onz ^ 8));
            const unsigned chw = *reinterpret_cast<const unsigned*>(nb + 48);       // left | right << 16
            ln = fmaxf(fmaxf(fmaf_(ex.x, inv.x, cn.x), fmaf_(ey.x, inv.y, cn.y)), fmaf_(ez.x, inv.z, cn.z));
            rn = fmaxf(fmaxf(fmaf_(ex.y, inv.x, cn.x), fmaf_(ey.y, inv.y, cn.y)), fmaf_(ez.y, inv.z, cn.z));
            lf = fminf(fminf(fmaf_(xx.x, inv.x, cf.x), fmaf_(xy.x, inv.y, cf.y)), fmaf_(xz.x, inv.z, cf.z)) * kWiden;
            rf = fminf(fminf(fmaf_(xx.y, inv.x, cf.x), fmaf_(xy.y, inv.y, cf.y)), fmaf_(xz.y, inv.z, cf.z)) * kWiden;
            li = (int)(chw & 0xffffu);
            ri = (int)(chw >> 16);
        } else {
            // (unsigned 32-bit byte offsets: scalar base + vector offset addressing, no 64-bit address
            // math; pt_add_triangles caps the scene so that they cannot wrap)
            const unsigned off = (unsigned)cur << 6;
            float4 qx, qy, qz, qr;
            if (KIND == kVisitFlat) {
                const char* nb = ((unsigned)cur < sv.treelet ? reinterpret_cast<const char*>(sv.lds_nodes) : reinterpret_cast<const char*>(sv.nodes)) + off;
                qx = *reinterpret_cast<const float4*>(nb);
                qy = *reinterpret_cast<const float4*>(nb + 16);
                qz = *reinterpret_cast<const float4*>(nb + 32);
                qr = *reinterpret_cast<const float4*>(nb + 48);
            } else {
                const char* nb = reinterpret_cast<const char*>(sv.nodes);
                qx = *reinterpret_cast<const float4*>(nb + off);
                qy = *reinterpret_cast<const float4*>(nb + (off + 16u));
                qz = *reinterpret_cast<const float4*>(nb + (off + 32u));
                qr = *reinterpret_cast<const float4*>(nb + (off + 48u));
            }
#if PT_GLOBAL_SLAB_FMA
            const bool sx = negx(), sy = negy(), sz = negz();
            const float lnx = sx ? qx.y : qx.x, lfx = sx ? qx.x : qx.y, rnx = sx ? qx.w : qx.z, rfx = sx ? qx.z : qx.w;
            const float lny = sy ? qy.y : qy.x, lfy = sy ? qy.x : qy.y, rny = sy ? qy.w : qy.z, rfy = sy ? qy.z : qy.w;
            const float lnz = sz ? qz.y : qz.x, lfz = sz ? qz.x : qz.y, rnz = sz ? qz.w : qz.z, rfz = sz ? qz.z : qz.w;
            ln = fmaxf(fmaxf(fmaf_(lnx, inv.x, cn.x), fmaf_(lny, inv.y, cn.y)), fmaf_(lnz, inv.z, cn.z));
            rn = fmaxf(fmaxf(fmaf_(rnx, inv.x, cn.x), fmaf_(rny, inv.y, cn.y)), fmaf_(rnz, inv.z, cn.z));
            lf = fminf(fminf(fmaf_(lfx, inv.x, cf.x), fmaf_(lfy, inv.y, cf.y)), fmaf_(lfz, inv.z, cf.z)) * kWiden;
            rf = fminf(fminf(fmaf_(rfx, inv.x, cf.x), fmaf_(rfy, inv.y, cf.y)), fmaf_(rfz, inv.z, cf.z)) * kWiden;
#else
            // (plane - P) * inv with min/max picking the planes: ~2 ulp per distance, covered by the
            // 4-ulp widening (a NaN here is replaced by the other plane's finite distance, which is safe
            // only in this subtract-then-multiply form)
            const float lx0 = (qx.x - P.x) * inv.x, lx1 = (qx.y - P.x) * inv.x;
            const float rx0 = (qx.z - P.x) * inv.x, rx1 = (qx.w - P.x) * inv.x;
            const float ly0 = (qy.x - P.y) * inv.y, ly1 = (qy.y - P.y) * inv.y;
            const float ry0 = (qy.z - P.y) * inv.y, ry1 = (qy.w - P.y) * inv.y;
            const float lz0 = (qz.x - P.z) * inv.z, lz1 = (qz.y - P.z) * inv.z;
            const float rz0 = (qz.z - P.z) * inv.z, rz1 = (qz.w - P.z) * inv.z;
            ln = fmaxf(fmaxf(fminf(lx0, lx1), fminf(ly0, ly1)), fminf(lz0, lz1));
            lf = fminf(fminf(fmaxf(lx0, lx1), fmaxf(ly0, ly1)), fmaxf(lz0, lz1)) * kWiden;
            rn = fmaxf(fmaxf(fminf(rx0, rx1), fminf(ry0, ry1)), fminf(rz0, rz1));
            rf = fminf(fminf(fmaxf(rx0, rx1), fmaxf(ry0, ry1)), fmaxf(rz0, rz1)) * kWiden;
#endif
            li = __float_as_int(qr.x);
            ri = __float_as_int(qr.y);
        }
        const float lim = best_t * kWiden;
        const bool hl = (lf >= ln) && (lf >= 0.0f) && (ln <= lim);
        const bool hr = (rf >= rn) && (rf >= 0.0f) && (rn <= lim);
        const bool lfirst = ln <= rn;      // (its own statement: inside the expression below it comes back as a branch)
        const bool take_left = hl && (!hr || lfirst);
        const bool both = hl && hr, none = !(hl || hr);
        const int other = take_left ? ri : li;
        *reinterpret_cast<StackT*>(tos + stride) = (StackT)other;
        const int next = take_left ? li : ri;
        if (DEFER) {
            const bool cap = !none && is_leaf(next) && pend == 0;
            pend = cap ? next : pend;
            const bool usetop = none || (cap && !both);
            cur = usetop ? top : (cap ? other : next);
            tos += (both && !cap) ? stride : (usetop ? -stride : 0);
        } else {
            cur = none ? top : next;
            tos += both ? stride : (none ? -stride : 0);
        }
    }

    // One visit of a 4-wide node (Node4q, pt_internal.hpp; built by pt_wide.cpp): ONE 64-byte fetch decides what two
    // BVH2 levels decide.  The child planes are bytes on the node's own grid; a plane decodes as
    // fma((float)q, step, origin) -- the very expression the host checked to lie outside the child's box -- and then
    // goes through the same slab test as a BVH2 plane (entry / exit picked by the direction sign, here by selecting
    // the WORD that holds the four children's bytes: 6 selects for 24 planes).  The children that are hit are sorted
    // by entry distance (5 compare-exchanges); the nearest is visited next, the others are stored above the top of
    // the stack farthest first.  All three stores are unconditional (a child that was missed lands above the new
    // top, where it is never read), so the stack has room for top + 3 at every visit (wide_stack_entries()).
    // stack entry at address `at`, which may lie past the lane's LDS entries (kNodesWide only)
    PT_DEV int entry_of(const char* at) const {      // which stack entry an address is (stride = BLOCK x 4 B, a power of two)
        return (int)((unsigned)(at - reinterpret_cast<const char*>(pt_lds_raw)) >> (31 - __builtin_clz(stride)));
    }
    PT_DEV unsigned lane_of(const char* at) const {  // whose: the thread index inside the workgroup
        return ((unsigned)(at - reinterpret_cast<const char*>(pt_lds_raw)) & (unsigned)(stride - 1)) >> 2;
    }
    PT_DEV int stack_get(const SceneView& sv, const char* at) const {
        const int j = MODE == kNodesWide ? entry_of(at) - sv.lds_entries : -1;
        if (j < 0) return (int)*reinterpret_cast<const StackT*>(at);
        return (int)sv.ovf[(size_t)j * sv.ovf_stride + lane_of(at)];
    }
    PT_DEV void stack_put(const SceneView& sv, char* at, int v) const {
        const int j = MODE == kNodesWide ? entry_of(at) - sv.lds_entries : -1;
        if (j < 0) *reinterpret_cast<StackT*>(at) = (StackT)v;
        else sv.ovf[(size_t)j * sv.ovf_stride + lane_of(at)] = (unsigned)v;
    }

#if PT_WIDE_STEP_V1
    template <bool COUNT>
    PT_DEV void wide_step(const SceneView& sv, WorkCount* wc) {
        const float kWiden = 1.0000005f;
        // does any lane of the wave come within three entries of the end of its LDS part?  (rare: then every stack
        // access of this visit goes through the checked accessors)
        const bool tight = __ballot(entry_of(tos) + 3 >= sv.lds_entries) != 0;
        const int top = tight ? stack_get(sv, tos) : (int)*reinterpret_cast<const StackT*>(tos);
        if (COUNT) { wc->nodes++; if (first_active_lane()) wc->wnodes++; count_low(wc, 0); }
        const char* nb = reinterpret_cast<const char*>(sv.nodes);
        const unsigned off = (unsigned)cur << 6;
        const float4 h = *reinterpret_cast<const float4*>(nb + off);
        const uint4 qa = *reinterpret_cast<const uint4*>(nb + (off + 16u));
        const uint2 qb = *reinterpret_cast<const uint2*>(nb + (off + 32u));
        const int4 rf = *reinterpret_cast<const int4*>(nb + (off + 48u));
        const unsigned eb = (unsigned)__float_as_int(h.w);
        const float sx = __int_as_float((int)((eb & 0xffu) << 23)), sy = __int_as_float((int)(((eb >> 8) & 0xffu) << 23));
        const float sz = __int_as_float((int)(((eb >> 16) & 0xffu) << 23));
        const bool ngx = negx(), ngy = negy(), ngz = negz();
        const unsigned enx = ngx ? qa.y : qa.x, exx = ngx ? qa.x : qa.y;
        const unsigned eny = ngy ? qa.w : qa.z, exy = ngy ? qa.z : qa.w;
        const unsigned enz = ngz ? qb.y : qb.x, exz = ngz ? qb.x : qb.y;
        const float lim = best_t * kWiden;
        float key[4];
        int ref[4] = {rf.x, rf.y, rf.z, rf.w};
        int n = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float pnx = fmaf_((float)((enx >> (8 * k)) & 0xffu), sx, h.x), pfx = fmaf_((float)((exx >> (8 * k)) & 0xffu), sx, h.x);
            const float pny = fmaf_((float)((eny >> (8 * k)) & 0xffu), sy, h.y), pfy = fmaf_((float)((exy >> (8 * k)) & 0xffu), sy, h.y);
            const float pnz = fmaf_((float)((enz >> (8 * k)) & 0xffu), sz, h.z), pfz = fmaf_((float)((exz >> (8 * k)) & 0xffu), sz, h.z);
            const float tn = fmaxf(fmaxf(fmaf_(pnx, inv.x, cn.x), fmaf_(pny, inv.y, cn.y)), fmaf_(pnz, inv.z, cn.z));
            const float tf = fminf(fminf(fmaf_(pfx, inv.x, cf.x), fmaf_(pfy, inv.y, cf.y)), fmaf_(pfz, inv.z, cf.z)) * kWiden;
            // (no test for "no child": its box is inverted and its reference a harmless leaf -- pt_wide.cpp; a "hit" at
            // tn = +inf is a ray parallel to a slab it is outside of: sorting it among the misses drops it, rightly)
            const bool hit = (tf >= tn) && (tf >= 0.0f) && (tn <= lim);
            key[k] = hit ? tn : __builtin_inff();
            n += key[k] < __builtin_inff() ? 1 : 0;
        }
#define PT_CSWAP(a, b)                                                                        \
        {                                                                                     \
            const bool sw = key[a] > key[b];                                                  \
            const float ka = sw ? key[b] : key[a], kb = sw ? key[a] : key[b];                 \
            const int ra = sw ? ref[b] : ref[a], rb = sw ? ref[a] : ref[b];                   \
            key[a] = ka; key[b] = kb; ref[a] = ra; ref[b] = rb;                               \
        }
        PT_CSWAP(0, 1) PT_CSWAP(2, 3) PT_CSWAP(0, 2) PT_CSWAP(1, 3) PT_CSWAP(1, 2)
#undef PT_CSWAP
        // the nearest child is a leaf and no leaf is pending: remember it (round() intersects it after the node phase)
        // and go on with the next child -- fewer node-phase / leaf-phase alternations, as in node_step
        const bool cap = n > 0 && is_leaf(ref[0]) && pend == 0;
        pend = cap ? ref[0] : pend;
        ref[0] = cap ? ref[1] : ref[0];
        ref[1] = cap ? ref[2] : ref[1];
        ref[2] = cap ? ref[3] : ref[2];
        n -= cap ? 1 : 0;
        // child j (1 <= j < n) goes to entry top + (n - j): popped nearest first; a missed child (j >= n) to top + j
        char* const a1 = tos + (1 < n ? n - 1 : 1) * stride;
        char* const a2 = tos + (2 < n ? n - 2 : 2) * stride;
        char* const a3 = tos + (3 < n ? n - 3 : 3) * stride;
        if (!tight) {
            *reinterpret_cast<StackT*>(a1) = (StackT)ref[1];
            *reinterpret_cast<StackT*>(a2) = (StackT)ref[2];
            *reinterpret_cast<StackT*>(a3) = (StackT)ref[3];
        } else {
            stack_put(sv, a1, ref[1]);
            stack_put(sv, a2, ref[2]);
            stack_put(sv, a3, ref[3]);
        }
        cur = n > 0 ? ref[0] : top;
        tos += (n > 0 ? n - 1 : -1) * stride;
    }

#else
    // Round 4: the visit re-counted in CLOCKS (tools/micro/exec_ops.hip: v_fma / v_mul / v_add 2.4-2.9 per wave
    // instruction, v_cvt / v_cmp / v_cndmask / v_min3 / v_max3 / v_lshlrev 4.2-4.4, a VOP2 v_cndmask on a VCC the SALU wrote 21):
    //  * decode and slab test are ONE fma per plane: t = q * (step * inv) + (origin * inv - P * inv).  step is a power of
    //    two, so step * inv is exact; the second term costs one rounding per axis and side, taken once per node (6 fma)
    //    instead of once per plane (24 fma saved).  The plane the host checked, fl(q * step + origin), no longer exists:
    //    the effective plane is the real number q * step + origin, at most half an ulp of the coordinate off it --
    //    1 / 170 of what padded_bounds() adds to every triangle's box (1e-5 of the coordinate), and the new rounding of
    //    (origin * inv + c) is one more half-ulp of P * inv out of the four that c is widened by (setup());
    //  * the three exponent bytes become step factors with one SDWA shift each (byte select in the instruction);
    //  * hit <=> max(tn, 0) <= min(tf, lim): one compare, whose VCC feeds the select of the key AND the count of hit
    //    children (three compares joined on the SALU ended in a 21-clock select);
    //  * the pushes are predicated stores at tos + (n - j): no address selects.
    PT_DEV static float exp_byte_step(unsigned eb, int which) {      // 2^(byte - 127): byte << 23
        unsigned r;
        if (which == 0) asm("v_lshlrev_b32_sdwa %0, 23, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(r) : "v"(eb));
        else if (which == 1) asm("v_lshlrev_b32_sdwa %0, 23, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(r) : "v"(eb));
        else asm("v_lshlrev_b32_sdwa %0, 23, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(r) : "v"(eb));
        return __int_as_float((int)r);
    }
    template <bool COUNT>
    PT_DEV void wide_step(const SceneView& sv, WorkCount* wc) {
        const float kWiden = 1.0000005f;
        // does any lane of the wave come within three entries of the end of its LDS part?  (rare: then every stack
        // access of this visit goes through the checked accessors)
        const bool tight = __ballot(entry_of(tos) + 3 >= sv.lds_entries) != 0;
        const int top = tight ? stack_get(sv, tos) : (int)*reinterpret_cast<const StackT*>(tos);
        if (COUNT) { wc->nodes++; if (first_active_lane()) wc->wnodes++; count_low(wc, 0); }
        const char* nb = reinterpret_cast<const char*>(sv.nodes);
        const unsigned off = (unsigned)cur << 6;
        const float4 h = *reinterpret_cast<const float4*>(nb + off);
        const uint4 qa = *reinterpret_cast<const uint4*>(nb + (off + 16u));
        const uint2 qb = *reinterpret_cast<const uint2*>(nb + (off + 32u));
        const int4 rf = *reinterpret_cast<const int4*>(nb + (off + 48u));
        const unsigned eb = (unsigned)__float_as_int(h.w);
        const float ax = exp_byte_step(eb, 0) * inv.x, ay = exp_byte_step(eb, 1) * inv.y, az = exp_byte_step(eb, 2) * inv.z;
        const float bnx = fmaf_(h.x, inv.x, cn.x), bny = fmaf_(h.y, inv.y, cn.y), bnz = fmaf_(h.z, inv.z, cn.z);
        const float bfx = fmaf_(h.x, inv.x, cf.x), bfy = fmaf_(h.y, inv.y, cf.y), bfz = fmaf_(h.z, inv.z, cf.z);
        const bool ngx = negx(), ngy = negy(), ngz = negz();
        const unsigned enx = ngx ? qa.y : qa.x, exx = ngx ? qa.x : qa.y;
        const unsigned eny = ngy ? qa.w : qa.z, exy = ngy ? qa.z : qa.w;
        const unsigned enz = ngz ? qb.y : qb.x, exz = ngz ? qb.x : qb.y;
        const float lim = best_t * kWiden;
        float key[4];
        int ref[4] = {rf.x, rf.y, rf.z, rf.w};
        int n = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float tnx = fmaf_((float)((enx >> (8 * k)) & 0xffu), ax, bnx), tfx = fmaf_((float)((exx >> (8 * k)) & 0xffu), ax, bfx);
            const float tny = fmaf_((float)((eny >> (8 * k)) & 0xffu), ay, bny), tfy = fmaf_((float)((exy >> (8 * k)) & 0xffu), ay, bfy);
            const float tnz = fmaf_((float)((enz >> (8 * k)) & 0xffu), az, bnz), tfz = fmaf_((float)((exz >> (8 * k)) & 0xffu), az, bfz);
            // entry clamped to the ray's origin: then "exit >= entry" includes "exit >= 0", and lim >= 0 always
            const float tn = fmaxf(fmaxf(fmaxf(tnx, tny), tnz), 0.0f);
            const float tf = fminf(fminf(fminf(tfx, tfy), tfz) * kWiden, lim);
            // (no test for "no child": its box is inverted and its reference a harmless leaf -- pt_wide.cpp.  A child
            // "hit" at tn = +inf -- a ray parallel to a slab it is outside of -- sorts among the misses; should it be
            // pushed, or a miss in its place, the visit that follows is wasted work, not a wrong answer.)
            const bool hit = tn <= tf;
            key[k] = hit ? tn : __builtin_inff();
            n += hit ? 1 : 0;
        }
#define PT_CSWAP(a, b)                                                                        \
        {                                                                                     \
            const bool sw = key[a] > key[b];                                                  \
            const float ka = sw ? key[b] : key[a], kb = sw ? key[a] : key[b];                 \
            const int ra = sw ? ref[b] : ref[a], rb = sw ? ref[a] : ref[b];                   \
            key[a] = ka; key[b] = kb; ref[a] = ra; ref[b] = rb;                               \
        }
        PT_CSWAP(0, 1) PT_CSWAP(2, 3) PT_CSWAP(0, 2) PT_CSWAP(1, 3) PT_CSWAP(1, 2)
#undef PT_CSWAP
        // the nearest child is a leaf and no leaf is pending: remember it (round() intersects it after the node phase)
        // and go on with the next child -- fewer node-phase / leaf-phase alternations, as in node_step
        const bool cap = n > 0 && is_leaf(ref[0]) && pend == 0;
        pend = cap ? ref[0] : pend;
        ref[0] = cap ? ref[1] : ref[0];
        ref[1] = cap ? ref[2] : ref[1];
        ref[2] = cap ? ref[3] : ref[2];
        n -= cap ? 1 : 0;
#if PT_WIDE_PREDICATED_STORES
        // child j (1 <= j < n) goes to entry top + (n - j): popped nearest first; a missed child is not stored
        char* const a3 = tos + (n - 3) * stride;        // child 3's entry; children 2 and 1 one and two entries above it
        if (!tight) {
            if (1 < n) *reinterpret_cast<StackT*>(a3 + 2 * stride) = (StackT)ref[1];
            if (2 < n) *reinterpret_cast<StackT*>(a3 + stride) = (StackT)ref[2];
            if (3 < n) *reinterpret_cast<StackT*>(a3) = (StackT)ref[3];
        } else {
            if (1 < n) stack_put(sv, a3 + 2 * stride, ref[1]);
            if (2 < n) stack_put(sv, a3 + stride, ref[2]);
            if (3 < n) stack_put(sv, a3, ref[3]);
        }
#else
        // child j (1 <= j < n) goes to entry top + (n - j): popped nearest first; a missed child (j >= n) to top + j, above the
        // new top, where it is never read -- all three stores are unconditional (no branch in the visit)
        char* const a1 = tos + (1 < n ? n - 1 : 1) * stride;
        char* const a2 = tos + (2 < n ? n - 2 : 2) * stride;
        char* const a3 = tos + (3 < n ? n - 3 : 3) * stride;
        if (!tight) {
            *reinterpret_cast<StackT*>(a1) = (StackT)ref[1];
            *reinterpret_cast<StackT*>(a2) = (StackT)ref[2];
            *reinterpret_cast<StackT*>(a3) = (StackT)ref[3];
        } else {
            stack_put(sv, a1, ref[1]);
            stack_put(sv, a2, ref[2]);
            stack_put(sv, a3, ref[3]);
        }
#endif
        cur = n > 0 ? ref[0] : top;
        tos += (n > 0 ? n - 1 : -1) * stride;
    }

#endif
    // exact test of packed triangle ti against the ray, keeping the closest (ties: lower rank)
    template <bool COUNT>
    PT_DEV void tri_step(const SceneView& sv, int ti, WorkCount* wc) {
        const char* tb = reinterpret_cast<const char*>(sv.tris);
        const unsigned off = (unsigned)ti * 48u;
        const float4 a = *reinterpret_cast<const float4*>(tb + off), b = *reinterpret_cast<const float4*>(tb + (off + 16u)), c = *reinterpret_cast<const float4*>(tb + (off + 32u));
        tri_update<COUNT>(sv, a, b, c, ti, wc);
    }
    template <bool COUNT>
    PT_DEV void tri_update(const SceneView& sv, const float4 a, const float4 b, const float4 c, int ti, WorkCount* wc) {
        if (COUNT) { wc->tris++; if (first_active_lane()) wc->wtris++; count_low(wc, 1); }
        const float t = tri_test<MODE == kNodesLds>(a, b, c, P, D, best_t * 1.000002f, COUNT ? wc : nullptr);
        keep_closest(sv, t, ti);
    }
    PT_DEV void keep_closest(const SceneView& sv, float t, int ti) {
        if (t > 0.0f) {
            bool better = t < best_t;
            if (t == best_t && best >= 0) better = sv.meta[ti].rank < sv.meta[best].rank;
            if (better) { best_t = t; best = ti; }
        }
    }
    // the pair of listed triangles ti, ti + 1 (packets pk[0..5] of the LDS copy): one evaluation, then A and B in list order --
    // the order in which tri_update meets them one by one, so a tie between the halves (a hit on the diagonal) goes the same way
    template <bool COUNT>
    PT_DEV void pair_update(const SceneView& sv, const float4* pk, int ti, WorkCount* wc) {
        if (COUNT) { wc->tris += 2; if (first_active_lane()) wc->wtris++; count_low(wc, 1); }
        float tA, tB;
        tri_test_pair<MODE == kNodesLds>(pk, P, D, best_t * 1.000002f, COUNT ? wc : nullptr, &tA, &tB);
        keep_closest(sv, tA, ti);
        keep_closest(sv, tB, ti + 1);
    }

    // The big-triangle list (the host keeps walls, floors ... out of the tree: pt_builder.cpp build_and_pack), tested
    // at the start of every traversal; what it finds prunes the tree from its first node visit.  Two passes:
    //  1. every lane slab-tests the DISTINCT padded boxes of the listed triangles (the two halves of a wall share
    //     one: 6 boxes for the Cornell box's 12 triangles, grouped by the host) -- a wave-uniform loop at full lane
    //     utilisation, 14 VALU + 4 LDS reads per box, planes picked by address from the direction signs exactly as
    //     for a staged node -- and notes the triangles of the boxes it touches in a bit mask (the same
    //     conservative cull a leaf box performs in the tree);
    //  2. each lane runs the exact test only on ITS candidates (2-6 of the 12 in the Cornell box: a wall is two
    //     triangles with one box, and a ray may cross the planes of a few walls), packets read from the LDS copy
    //     at a per-lane address.
    // Same exact test and tie-break as in a leaf, so the closest hit is unchanged.  (Testing all 12 exactly on
    // every lane cost 984 VALU per pass, a third of the kernel's instructions; this form ~600.)
    template <bool COUNT>
    PT_DEV void flat_pass(const SceneView& sv, WorkCount* wc) {
        const float kWiden = 1.0000005f;
        unsigned mask = 0;
        const int fx = ox(), fy = oy(), fz = oz();
#pragma clang loop unroll(disable) vectorize(disable)      // (unrolled x8 it spills 40 registers around the loop)
        for (int i = 0; i < sv.n_fbox; ++i) {
            const char* bb = sv.lds_fbox + i * 48;
            const float2 x = *reinterpret_cast<const float2*>(bb + fx);      // (entry plane, exit plane) of the axis
            const float2 y = *reinterpret_cast<const float2*>(bb + fy);
            const float2 z = *reinterpret_cast<const float2*>(bb + fz);
            const float tn = fmaxf(fmaxf(fmaf_(x.x, inv.x, cn.x), fmaf_(y.x, inv.y, cn.y)), fmaf_(z.x, inv.z, cn.z));
            const float tf = fminf(fminf(fmaf_(x.y, inv.x, cf.x), fmaf_(y.y, inv.y, cf.y)), fmaf_(z.y, inv.z, cf.z)) * kWiden;
            mask |= ((tf >= tn) && (tf >= 0.0f)) ? sv.lds_fmask[i] : 0u;
        }
        // 1b. (VALU-bound LDS node path only: +1.9 % there, -1 % on the paths that wait for memory) of those, keep the
        //     triangles whose plane lies ahead: the first early-out of the exact test (same predicate, so nothing the
        //     exact test would accept is dropped), 11 VALU + 2 LDS reads per candidate.  A ray leaving a wall still
        //     touches that wall's box -- two candidates per lane that only lengthen pass 2, whose every iteration costs
        //     the wave a full exact test as long as ONE lane has a live candidate.
        unsigned keep = mask;
        if (MODE == kNodesLds) {
            keep = 0;
            const float limit = best_t * 1.000002f;
#pragma clang loop unroll(disable)
            while (mask != 0) {
                const int i = __ffs((int)mask) - 1;
                // the head of a pair whose partner is a candidate too (they share the box, so always): the partner's r1 and N are
                // the head's words, its q the same bits -- one evaluation decides both
                const unsigned grp = (1u | ((((sv.fpair & (mask >> 1)) >> i) & 1u) << 1)) << i;
                mask &= ~grp;
                const float4* pk = sv.lds_flat + i * 3;
                const float4 a = pk[0], c = pk[2];
                const f3 N = mk(c.y, c.z, c.w);
                const float q = dot3(mk(a.x, a.y, a.z) - P, N) * __builtin_amdgcn_rcpf(dot3(D, N));
                keep |= (!(q < 0.0f) && !(q > limit)) ? grp : 0u;              // tri_test<true>'s early-out
            }
        }
        //  2. the exact test on what is left: a pair in ONE iteration (half the iterations for a wall, each of which costs the wave
        //     its full length as long as one lane has a candidate; one divide and one pt for both halves -- tri_test_pair)
#pragma clang loop unroll(disable)
        while (keep != 0) {
            const int i = __ffs((int)keep) - 1;
            const float4* pk = sv.lds_flat + i * 3;
            if (MODE == kNodesLds && (((sv.fpair & (keep >> 1)) >> i) & 1u) != 0) {
                keep &= ~(3u << i);
                pair_update<COUNT>(sv, pk, i, wc);
            } else {       // a single triangle, or a head whose partner was not kept
                keep &= keep - 1;
                tri_update<COUNT>(sv, pk[0], pk[1], pk[2], i, wc);
            }
        }
    }

    // One round: a node phase (every lane descends until it holds a leaf or has finished), then a leaf phase (the lanes holding
    // leaves intersect them and pop).  Round 4: a phase ENDS EARLY when few lanes are still in it and another lane is waiting for
    // the other phase -- the stragglers simply go on in the next round, next to the lanes that come back.  What a while-while
    // loop loses is its tails: half of all node-body executions ran for four lanes or fewer, and a VALU instruction with at most
    // 8 active lanes costs 3-4 times what it costs with 9 to 64 (tools/micro/exec_ops.hip).  MESH-100k 841 -> 980 Msamples/s,
    // MESH-1M 297 -> 353 at node_min_lanes = 8 (profiles/r04/).  The traversal state allows it as it is: round() can be entered
    // with a node, a leaf or a pending leaf in hand.
    template <bool COUNT>
    PT_DEV void step(const SceneView& sv, WorkCount* wc) {
        if (MODE == kNodesLds) node_step<COUNT, false, kVisitLds>(sv, wc);
        else if (MODE == kNodesGlobal) node_step<COUNT, true, kVisitGlobal>(sv, wc);
        else if (MODE == kNodesWide) wide_step<COUNT>(sv, wc);
        else node_step<COUNT, true, kVisitFlat>(sv, wc);
    }
    template <bool COUNT>
    PT_DEV void round(const SceneView& sv, WorkCount* wc) {
        // Every lane that enters a phase takes at least one step of it (so a round always makes progress, whatever the two
        // thresholds are); after that the phase ends for everybody as soon as at most `min_lanes` lanes are still in it AND some
        // lane has left it -- with a leaf to intersect, a node to visit, or a finished ray for the caller to replace.
        if (kPhaseSwitch) {
            const unsigned long long entered = __ballot(is_node(cur));
            if (is_node(cur)) {
                for (;;) {
                    step<COUNT>(sv, wc);
                    const bool live = is_node(cur);
                    if (!live) break;
                    const unsigned long long lm = __ballot(live);
                    if (lm != entered && __popcll(lm) <= sv.node_min_lanes) break;
                }
            }
        } else {
            while (is_node(cur)) step<COUNT>(sv, wc);
        }
        if (kDefer && pend != 0) {            // met first, so nearer: intersect it first
            const int v = leaf_bits(pend);
            const int first = v >> 3, count = (v & 7) + 1;
            for (int j = 0; j < count; ++j) tri_step<COUNT>(sv, first + j, wc);
            pend = 0;
        }
        if (kPhaseSwitch) {
            const unsigned long long entered = __ballot(is_leaf(cur));
            if (is_leaf(cur)) {
                for (;;) {
                    leaf_step<COUNT>(sv, wc);
                    const bool live = is_leaf(cur);
                    if (!live) break;
                    const unsigned long long lm = __ballot(live);
                    if (lm != entered && __popcll(lm) <= sv.leaf_min_lanes) break;
                }
            }
        } else {
            while (is_leaf(cur)) leaf_step<COUNT>(sv, wc);
        }
    }
    template <bool COUNT>
    PT_DEV void leaf_step(const SceneView& sv, WorkCount* wc) {
        const int popped = stack_get(sv, tos);     // in flight during the triangle tests
        const int v = leaf_bits(cur);
        const int first = v >> 3, count = (v & 7) + 1;
        for (int j = 0; j < count; ++j) tri_step<COUNT>(sv, first + j, wc);
        cur = popped;
        tos -= stride;
    }
};

template <int MODE, bool COUNT>
PT_DEV int closest_hit(const SceneView& sv, f3 P, f3 D, const LaneStack<typename StackOf<MODE>::type> stk, float* t_out, WorkCount* wc) {
    Trav<MODE> tr;
    tr.begin(P, D, stk);
    tr.template flat_pass<COUNT>(sv, wc);
    while (!tr.done()) tr.template round<COUNT>(sv, wc);
    *t_out = tr.best_t;
    return tr.best;
}

// ---------------------------------------------------------------------------- BSDF sampling
// prog.cl:186-218
// The tangent frame of the cosine lobe around N (prog.cl:205-212): Z, X.  A pure function of N, in two steps so that the inline
// path of diffuse_direction can take ONE wave-uniform branch for this root and its own two; tangent_frame() is the whole of it.
PT_DEV float frame_l2(f3 N, bool* yaxis) {
    const float E = 0.001f;
    *yaxis = __builtin_fabsf(N.x) <= E && __builtin_fabsf(N.z) <= E;
    const float other = *yaxis ? N.y : N.x;
    return fmaf_(N.z, N.z, other * other);
}
PT_DEV void frame_from_rl(f3 N, bool yaxis, float rl, f3* Z, f3* X) {      // rl = 1 / sqrt(frame_l2(N)), IEEE
    *Z = yaxis ? mk(0.0f, -N.z * rl, N.y * rl) : mk(-N.z * rl, 0.0f, N.x * rl);
    *X = cross3(N, *Z);
}
PT_DEV void tangent_frame(f3 N, f3* Z, f3* X) {
    bool yaxis;
    const float l2 = frame_l2(N, &yaxis);
    frame_from_rl(N, yaxis, rsqrt_rn(l2), Z, X);
}
// prog.cl:213-218 up to the normalisation (shade_hit does it): the direction in the frame (Z, X) of N
template <bool SK>
PT_DEV f3 lobe_direction(f3 N, f3 Z, f3 X, float r, float z, float rnd2) {      // r = sqrt(rnd1), z = sqrt(1 - rnd1), IEEE
    const float theta = (float)(6.283185307179586 * (double)rnd2);
    float sn, cs;
    spec_sincos<SK>(theta, &sn, &cs);
    const float x = r * cs, y = r * sn;
    f3 d = X * x;
    d = madd(N, z, d);
    d = madd(Z, y, d);
    return d;
}
template <bool SK>
PT_DEV f3 diffuse_direction(f3 N, float rnd1, float rnd2) {       // prog.cl:205-218 up to the normalisation (shade_hit does it)
    bool yaxis;
    const float l2 = frame_l2(N, &yaxis);
    // the three roots and the divide below are IEEE; one uniform branch picks the cores for all of them or the compiler's
    // expansions.  sqrt_core needs rnd1 >= 2^-96 and 1 - rnd1 >= 2^-96; the latter holds for every float rnd1 < 1 (1 - rnd1
    // is then at least 2^-24)
    float rl, r, z;
    if (wave_all(rsqrt_window(l2) && rnd1 >= kSqrtWindowLo && rnd1 < 1.0f)) {
        rl = rsqrt_core(l2);
        r = sqrt_core(rnd1);
        z = sqrt_core(1.0f - rnd1);
    } else {
        rl = 1.0f / __builtin_sqrtf(l2);
        r = __builtin_sqrtf(rnd1);
        z = __builtin_sqrtf(1.0f - rnd1);
    }
    f3 Z, X;
    frame_from_rl(N, yaxis, rl, &Z, &X);
    return lobe_direction<SK>(N, Z, X, r, z, rnd2);
}
// the same with the frame of N read from the triangle's shading record (ShadeRec::frame of the orientation the flip chose):
// what is left of the wave-level window are the rnd1 conditions
template <bool SK>
PT_DEV f3 diffuse_direction_rec(f3 N, const float4* frame, float rnd1, float rnd2) {
    const float4 fa = frame[0], fb = frame[1];
    float r, z;
    if (wave_all(rnd1 >= kSqrtWindowLo && rnd1 < 1.0f)) {
        r = sqrt_core(rnd1);
        z = sqrt_core(1.0f - rnd1);
    } else {
        r = __builtin_sqrtf(rnd1);
        z = __builtin_sqrtf(1.0f - rnd1);
    }
    return lobe_direction<SK>(N, mk(fa.x, fa.y, fa.z), mk(fa.w, fb.x, fb.y), r, z, rnd2);
}

// prog.cl:219-222
PT_DEV f3 fresnel(f3 F0, f3 N, f3 D) {
    const float cosa = __builtin_fabsf(dot3(N, D));
    const float p5 = spec_pow5(1.0f - cosa);
    return mk(fmaf_(1.0f - F0.x, p5, F0.x), fmaf_(1.0f - F0.y, p5, F0.y), fmaf_(1.0f - F0.z, p5, F0.z));
}

// ---- rough metal, material type 4 under option glossy (GGX with visible-normal sampling; include/pt_api.h pins every operation)
// All vectors are local to the frame (X, Z, N) that frame_from_rl builds: v = (v.X, v.Z, v.N), so v.z is the cosine to the normal.
PT_DEV float glossy_D(float alpha, f3 h) {
    const float a2 = alpha * alpha;
    const float d = fmaf_(a2, h.z * h.z, fmaf_(h.y, h.y, h.x * h.x));
    return a2 / (3.14159265358979323846f * (d * d));
}
PT_DEV float glossy_G1(float alpha, f3 v) {
    if (!(v.z > 0.0f)) return 0.0f;
    return (2.0f * v.z) / (v.z + __builtin_sqrtf(fmaf_(alpha * alpha, fmaf_(v.y, v.y, v.x * v.x), v.z * v.z)));
}
// p_b of the direction whose half vector with o is h: the ONE statement of the density -- the sampler, the light sample and W_b go through it
PT_DEV float glossy_pdf(float alpha, f3 o, f3 h) {
    if (!(o.z > 0.0f)) return 0.0f;
    return (glossy_G1(alpha, o) * glossy_D(alpha, h)) / (4.0f * o.z);
}
// p_b of a given unit direction w (the light sample's); *h = normalize(o + w)
PT_DEV float glossy_pdf_of(float alpha, f3 o, f3 w, f3* h) {
    *h = normalize3(o + w);
    return glossy_pdf(alpha, o, *h);
}
// the weight g(w) = F G1(w) the vertex multiplies factor_S by; the ray direction in the frame is -o
PT_DEV f3 glossy_weight(float alpha, f3 F0, f3 o, f3 h, f3 w) { return fresnel(F0, h, -o) * glossy_G1(alpha, w); }
PT_DEV f3 to_local(f3 v, f3 X, f3 Z, f3 N) { return mk(dot3(v, X), dot3(v, Z), dot3(v, N)); }
// visible-normal sampling (Heitz 2018) from the disc point (t1, t2) = sqrt(rnd1) (cos, sin)(2 pi rnd2): the half vector h and the
// reflected direction w = 2 (o.h) h - o, both local
PT_DEV f3 glossy_sample(float alpha, f3 o, float t1, float t2, f3* h_out) {
    const f3 Vh = normalize3(mk(alpha * o.x, alpha * o.y, o.z));
    const float l2 = fmaf_(Vh.y, Vh.y, Vh.x * Vh.x);
    f3 T1 = mk(1.0f, 0.0f, 0.0f);
    if (l2 > 0.0f) {
        const float l = __builtin_sqrtf(l2);
        T1 = mk(-Vh.y / l, Vh.x / l, 0.0f);
    }
    const f3 T2 = cross3(Vh, T1);
    const float q = 0.5f * (1.0f + Vh.z);
    t2 = fmaf_(q, t2, (1.0f - q) * __builtin_sqrtf(max0(fmaf_(-t1, t1, 1.0f))));
    const float t3 = __builtin_sqrtf(max0(fmaf_(-t2, t2, fmaf_(-t1, t1, 1.0f))));
    const f3 Nh = madd(Vh, t3, madd(T2, t2, T1 * t1));
    const f3 h = normalize3(mk(alpha * Nh.x, alpha * Nh.y, max0(Nh.z)));
    *h_out = h;
    return madd(h, 2.0f * dot3(o, h), -o);
}
// what the sampled glossy vertex leaves behind
struct GlossyOut {
    f3 F;            // g(w) = F g1w, as glossy_weight states it
    float g1w;
    float pb;        // p_b as sampled
    float wz;        // w.z: the path ends unless it is > 0
    float oz;        // (pt_debug_glossy)
};

// ---- coated diffuse, material type 5 under option coated (a diffuse base under a rough dielectric coat; include/pt_api.h pins every
// operation).  Local vectors as above; D, G1, glossy_pdf, glossy_weight and fresnel are the rough metal's.
constexpr float kOneOverPi = 0.318309886183790672f;
PT_DEV f3 coated_F(f3 F0, float c) { return fresnel(F0, mk(0.0f, 0.0f, 1.0f), mk(0.0f, 0.0f, -c)); }      // F(c): fresnel's |dot3| is |c|
// the probability of the coat lobe at the vertex seen along o with albedo kd'
PT_DEV float coated_ps(f3 F0, f3 kd, f3 o) {
    const f3 Fo = coated_F(F0, o.z);
    const float fm = ((Fo.x + Fo.y) + Fo.z) / 3.0f;
    const float km = ((kd.x + kd.y) + kd.z) / 3.0f;
    const float s = fmaf_(1.0f - fm, km, fm);
    const float ps = s > 0.0f ? fm / s : 0.5f;
    return ps < 0.1f ? 0.1f : ps > 0.9f ? 0.9f : ps;
}
// p_b of the local direction w whose half vector with o is h, the mixture of the two lobes -- the ONE statement of the density: the
// sampler (whichever lobe drew w), the light sample and W_b go through it.  *g = (spec(w) + diff(w)) / p_b(w), 0 unless p_b > 0
PT_DEV float coated_pdf_weight(float alpha, f3 F0, f3 kd, float ps, f3 o, f3 h, f3 w, f3* g) {
    const float pg = glossy_pdf(alpha, o, h);
    const float c = max0(w.z);
    const float pb = fmaf_(ps, pg, ((1.0f - ps) * c) * kOneOverPi);
    const f3 spec = glossy_weight(alpha, F0, o, h, w) * pg;
    const f3 Fo = coated_F(F0, o.z), Fw = coated_F(F0, c);
    const f3 diff = ((mk(1.0f - Fo.x, 1.0f - Fo.y, 1.0f - Fo.z) * mk(1.0f - Fw.x, 1.0f - Fw.y, 1.0f - Fw.z)) * kd) * (c * (c * kOneOverPi));
    const float ip = pb > 0.0f ? 1.0f / pb : 0.0f;
    *g = (spec + diff) * ip;
    return pb;
}
// the same for a given unit direction w (the light sample's): ps and h = normalize(o + w) from scratch
PT_DEV float coated_pdf_weight_of(float alpha, f3 F0, f3 kd, f3 o, f3 w, f3* g) {
    return coated_pdf_weight(alpha, F0, kd, coated_ps(F0, kd, o), o, normalize3(o + w), w, g);
}
// what the sampled coated vertex leaves behind
struct CoatedOut {
    f3 g;            // g(w)
    float pb;        // p_b as sampled (the mixture)
    float wz;        // w.z: the path ends unless it is > 0
    float ps;        // (pt_debug_coated)
    float oz;
    bool coat;       // the coat lobe drew w
};

// ---- rough dielectric, material type 6 under option frosted (GGX reflection and refraction through one visible-normal half vector;
// include/pt_api.h pins every operation).  Local vectors as above; D, G1, glossy_pdf, glossy_sample and fresnel are the rough metal's.
// the Fresnel terms at half vector h: c = o.h, F (Schlick), type 2's discriminant and the mean Fm; total internal reflection makes F and Fm 1
struct FrostedTerms {
    f3 F;
    float Fm, c, disc;
};
PT_DEV FrostedTerms frosted_terms(f3 F0, float eta, f3 o, f3 h) {
    FrostedTerms t;
    t.c = dot3(o, h);
    t.F = fresnel(F0, h, -o);
    t.disc = 1.0f - (fmaf_(-t.c, t.c, 1.0f) / eta) / eta;
    t.Fm = ((t.F.x + t.F.y) + t.F.z) / 3.0f;
    if (t.disc <= 0.0f) {
        t.Fm = 1.0f;
        t.F = mk(1.0f, 1.0f, 1.0f);
    }
    return t;
}
// p_b and the weight g(w) of the local direction w whose half vector with o is h -- the ONE statement of both: the sampler (either lobe),
// the light sample and W_b go through it.  refl: w is the reflected direction (p_b = Fm p_glossy(h), g = F G1(w) / Fm); else the refracted
// one, which no light sample reaches (p_b reads 0, g = (1 - F) G1 of w mirrored to the upper side / (1 - Fm))
PT_DEV float frosted_pdf_weight(float alpha, const FrostedTerms& t, bool refl, f3 o, f3 h, f3 w, f3* g) {
    const f3 Fs = refl ? t.F : mk(1.0f - t.F.x, 1.0f - t.F.y, 1.0f - t.F.z);
    const float den = refl ? t.Fm : 1.0f - t.Fm;
    *g = (Fs * glossy_G1(alpha, mk(w.x, w.y, refl ? w.z : -w.z))) * (1.0f / den);
    return refl ? t.Fm * glossy_pdf(alpha, o, h) : 0.0f;
}
// the same for a given unit direction w above the surface (the light sample's): h = normalize(o + w) and the terms from scratch
PT_DEV float frosted_pdf_weight_of(float alpha, f3 F0, float eta, f3 o, f3 w, f3* g) {
    const f3 h = normalize3(o + w);
    return frosted_pdf_weight(alpha, frosted_terms(F0, eta, o, h), true, o, h, w, g);
}
// what the sampled frosted vertex leaves behind
struct FrostedOut {
    f3 g;            // g(w)
    float pb;        // p_b as sampled (0 for a refraction)
    float wz;        // w.z: the path ends unless it is > 0 (reflection) or < 0 (refraction)
    float Fm;        // (pt_debug_frosted)
    float oz;
    bool refl;       // the vertex reflects
};
// what the metal's sampled direction w (half vector h) leaves behind
PT_DEV void glossy_out(float alpha, f3 F0, f3 o, f3 h, f3 w, GlossyOut* out) {
    out->pb = glossy_pdf(alpha, o, h);
    out->g1w = glossy_G1(alpha, w);
    out->F = fresnel(F0, h, -o);
    out->wz = w.z;
    out->oz = o.z;
}
// The direction (before normalisation) of a lobe vertex in the instances with rough materials: diffuse_direction's frame, roots, sincos
// and world sum, shared by the lanes of every kind; only the local coordinates in between differ.  gl: a type-4 vertex (the metal); ct: a
// type-5 one (coated; u_sel chooses its lobe against ps); fr: a type-6 one (frosted; u_sel chooses reflection against Fm).  The metal, the
// coat lobe and the frosted vertex share one visible-normal draw, the cosine lobes sqrt(1 - rnd1); a refracting lane only replaces the
// reflected direction by type 2's refracted one around h, and the Fresnel terms, G1 and the weight are one sequence for both of its lobes.
// A diffuse lane gets diffuse_direction's bits.  Without COAT (ct and fr false, co and fo unread) the metal is the only rough kind and
// has one block of its own: the glossy instances compile to other code from the general arm.
template <bool SK, bool COAT>
PT_DEV f3 lobe_direction_rough(f3 N, f3 D, bool gl, bool ct, bool fr, float alpha, f3 F0, f3 kd, float eta, float u_sel, float rnd1, float rnd2,
                               GlossyOut* out, CoatedOut* co, FrostedOut* fo) {
    bool yaxis;
    const float l2 = frame_l2(N, &yaxis);
    float rl, r;
    if (wave_all(rsqrt_window(l2) && rnd1 >= kSqrtWindowLo && rnd1 < 1.0f)) {
        rl = rsqrt_core(l2);
        r = sqrt_core(rnd1);
    } else {
        rl = 1.0f / __builtin_sqrtf(l2);
        r = __builtin_sqrtf(rnd1);
    }
    f3 Z, X;
    frame_from_rl(N, yaxis, rl, &Z, &X);
    const float theta = (float)(6.283185307179586 * (double)rnd2);
    float sn, cs;
    spec_sincos<SK>(theta, &sn, &cs);
    float x = r * cs, y = r * sn, z = 0.0f;
    if constexpr (!COAT) {
        if (gl) {
            const f3 o = to_local(-D, X, Z, N);
            f3 h;
            const f3 w = glossy_sample(alpha, o, x, y, &h);
            glossy_out(alpha, F0, o, h, w, out);
            x = w.x;
            y = w.y;
            z = w.z;
        } else {
            z = sqrt_rn(1.0f - rnd1);
        }
    } else {
        f3 o = mk(0.f, 0.f, 1.f), h = o;
        float ps = 0.0f;
        bool vis = gl || fr;   // the lane samples visible normals: a metal, a frosted vertex, or the coat lobe of a coated vertex
        if (gl || ct || fr) o = to_local(-D, X, Z, N);
        if (ct) {
            ps = coated_ps(F0, kd, o);
            vis = u_sel < ps;
        }
        if (vis) {
            const f3 w = glossy_sample(alpha, o, x, y, &h);
            x = w.x;
            y = w.y;
            z = w.z;
        } else {
            z = sqrt_rn(1.0f - rnd1);
        }
        if (gl) glossy_out(alpha, F0, o, h, mk(x, y, z), out);
        if (ct) {
            const f3 w = mk(x, y, z);
            if (!vis) h = normalize3(o + w);
            co->pb = coated_pdf_weight(alpha, F0, kd, ps, o, h, w, &co->g);
            co->wz = z;
            co->ps = ps;
            co->oz = o.z;
            co->coat = vis;
        }
        if (fr) {
            const FrostedTerms t = frosted_terms(F0, eta, o, h);
            const bool refl = u_sel < t.Fm;
            if (!refl) {       // type 2's refracted direction with h for the normal (the ray direction in the frame is -o)
                const f3 w = madd(h, t.c / eta - sqrt_rn(t.disc), mk(-o.x / eta, -o.y / eta, -o.z / eta));
                x = w.x;
                y = w.y;
                z = w.z;
            }
            fo->pb = frosted_pdf_weight(alpha, t, refl, o, h, mk(x, y, z), &fo->g);
            fo->wz = z;
            fo->Fm = t.Fm;
            fo->oz = o.z;
            fo->refl = refl;
        }
    }
    f3 d = X * x;
    d = madd(N, z, d);
    d = madd(Z, y, d);
    return d;
}

// ---------------------------------------------------------------------------- path state + shading
// The path state of prog.cl:307-316: ray (P, D), LCG state and inside-glass flag are plain local variables of the
// caller; the four factors and the colour travel as one PathRegs.  (Round 3 also tried them in global memory behind the
// same accessors for the 72 / 80-VGPR kernel instances -- [field][lane of the grid], a segment moving only what its
// material touches: 1.5-3.6 % slower than letting the allocator spill, profiles/r03/c_*.)
struct PathRegs {
    f3 fL, fB, fS, fR, color;
    PT_DEV void reset() {
        fL = mk(1.f, 1.f, 1.f);
        fB = fL;
        fS = fL;
        fR = fL;
        color = mk(0.f, 0.f, 0.f);
    }
    PT_DEV f3 L() const { return fL; }
    PT_DEV f3 B() const { return fB; }
    PT_DEV f3 S() const { return fS; }
    PT_DEV f3 R() const { return fR; }
    PT_DEV f3 C() const { return color; }
    PT_DEV void setL(f3 v) { fL = v; }
    PT_DEV void setB(f3 v) { fB = v; }
    PT_DEV void setS(f3 v) { fS = v; }
    PT_DEV void setR(f3 v) { fR = v; }
    PT_DEV void setC(f3 v) { color = v; }
};

// ---- homogeneous medium (pt_set_medium; include/pt_api.h pins every operation).  The view is wave-uniform: lo, hi, sigma_t and g are scalar
// operands of the lanes' arithmetic.
// Clip: the part [*a, b] of [0, t] of the ray (P, D) inside the medium's box, by slabs; b is returned, and the length inside is max0(b - *a)
PT_DEV float medium_clip(const MediumView& mv, f3 P, f3 D, float t, float* a_out) {
    float a = 0.0f, b = t;
    const float p[3] = {P.x, P.y, P.z}, dd[3] = {D.x, D.y, D.z};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const float inv = 1.0f / dd[ax];
        if (__builtin_fabsf(inv) < __builtin_inff()) {
            const float t0 = (mv.lo[ax] - p[ax]) * inv, t1 = (mv.hi[ax] - p[ax]) * inv;
            const float nr = t0 < t1 ? t0 : t1, fr = t0 < t1 ? t1 : t0;
            a = nr > a ? nr : a;
            b = fr < b ? fr : b;
        } else if (!(p[ax] >= mv.lo[ax] && p[ax] <= mv.hi[ax])) {
            b = -__builtin_inff();       // parallel to the slab and outside it
        }
    }
    *a_out = a;
    return b;
}
// the free-flight distance of the unit number u in [0, 1): log1pf keeps its relative precision for a small u, where logf(1 - u) -- the
// hardware's log2 scaled -- only has an absolute one
PT_DEV float medium_flight(float sigma_t, float u) { return -log1pf(-u) / sigma_t; }
// Henyey-Greenstein's density of the cosine c between the direction of travel before and after the vertex
PT_DEV float medium_hg(float g, float c) {
    const float g2 = g * g;
    const float q = (1.0f + g2) - (2.0f * g) * c;
    return (1.0f - g2) / (12.566370614359172f * (q * __builtin_sqrtf(q)));
}
// the direction (before normalisation) that (u1, u2) draw from it around the unit direction D, and its *pb
PT_DEV f3 medium_direction(float g, f3 D, float u1, float u2, float* pb) {
    float c;
    if (__builtin_fabsf(g) < 1e-3f) {
        c = 1.0f - 2.0f * u1;
    } else {
        const float g2 = g * g;
        const float r = (1.0f - g2) / ((1.0f - g) + (2.0f * g) * u1);
        c = ((1.0f + g2) - r * r) / (2.0f * g);
    }
    *pb = medium_hg(g, c);
    const float s = __builtin_sqrtf(max0(1.0f - c * c));
    const float phi = 6.28318530717958647692f * u2;
    f3 Z, X;
    tangent_frame(D, &Z, &X);
    return madd(D, c, madd(Z, s * sinf(phi), X * (s * cosf(phi))));
}
// ---- area lights (pt_set_area_lights; pinned in include/pt_api.h): what the area-light instances of k_nee and
// k_debug_area_light both call
// the direction that (u1, u2) draw uniformly from the cone with 1 - cos(half angle) = q around the unit axis A, in medium_direction's frame
PT_DEV f3 area_cone(f3 A, float q, float u1, float u2) {
    const float c = 1.0f - u1 * q;
    const float s = __builtin_sqrtf(max0(1.0f - c * c));
    const float phi = 6.28318530717958647692f * u2;
    f3 Z, X;
    tangent_frame(A, &Z, &X);
    return madd(A, c, madd(Z, s * sinf(phi), X * (s * cosf(phi))));
}
// the sphere q0 = {C, R} seen from o: q = 1 - cos(theta_m) without cancellation, or -1 when o is not outside it (or d^2 is not finite);
// *c = C - o, *d2 = c.c, *R2 = R R
PT_DEV float area_sphere_q(const float4 q0, f3 o, f3* c, float* d2, float* R2) {
    *c = mk(q0.x, q0.y, q0.z) - o;
    *d2 = dot3(*c, *c);
    *R2 = q0.w * q0.w;
    if (!(*d2 < __builtin_inff() && *d2 > *R2)) return -1.0f;
    const float s2 = *R2 / *d2;
    const float cm = __builtin_sqrtf(max0(1.0f - s2));
    return s2 / (1.0f + cm);
}
// the sample of that sphere: false if rejected; else *w the direction, *pw its density 1 / (2 pi q), *ts the cut b - sqrt(max(0, b^2 - (d^2 - R^2)))
PT_DEV bool area_sphere_sample(const float4 q0, f3 o, float u1, float u2, f3* w, float* pw, float* ts) {
    f3 c;
    float d2, R2;
    const float q = area_sphere_q(q0, o, &c, &d2, &R2);
    if (!(q > 0.0f)) return false;
    *w = area_cone(normalize3(c), q, u1, u2);
    *pw = 1.0f / (6.28318530717958647692f * q);
    const float b = dot3(c, *w);
    *ts = b - __builtin_sqrtf(max0(fmaf_(b, b, -(d2 - R2))));
    return true;
}
// the nearest sphere of the set along (o, d) with 0 < t < tmax whose outside holds o, but for sphere `skip` (-1: none is skipped): its record
// index and *t, or -1.  The trip count and the record addresses are wave-uniform (the view is a kernel argument): the records come through
// scalar loads, and the lanes' arithmetic is plain FMA
PT_DEV int area_sphere_hit(const AreaLightsView& v, f3 o, f3 d, float tmax, int skip, float* t) {
    int best = -1;
    float bt = tmax;
    const float4* __restrict__ rec = v.rec;
    for (int j = 0; j < v.n_sphere; ++j) {
        const float4 q0 = rec[3 * j];
        const f3 c = mk(q0.x, q0.y, q0.z) - o;
        const float d2 = dot3(c, c), b = dot3(c, d);
        const float R2 = q0.w * q0.w;
        const float disc = fmaf_(b, b, -(d2 - R2));        // (the sample's cut, in the same operations)
        const float tj = b - __builtin_sqrtf(max0(disc));
        if (d2 > R2 && disc >= 0.0f && tj > 0.0f && tj < bt && j != skip) {
            bt = tj;
            best = j;
        }
    }
    *t = bt;
    return best;
}
// the suns of the set whose disc holds the unit direction d: bit j - n_sphere of the mask for record j
PT_DEV unsigned long long area_sun_mask(const AreaLightsView& v, f3 d) {
    unsigned long long mask = 0;
    const float4* __restrict__ rec = v.rec;
    for (int j = v.n_sphere; j < v.n; ++j) {
        const float4 q0 = rec[3 * j];
        if (dot3(d, mk(q0.x, q0.y, q0.z)) >= q0.w) mask |= 1ull << (j - v.n_sphere);
    }
    return mask;
}
// T of the ray (o, w) cut at `limit`: 1 exactly when no part of it lies in the box
PT_DEV float medium_transmittance(const MediumView& mv, f3 o, f3 w, float limit) {
    float a;
    const float b = medium_clip(mv, o, w, limit, &a);
    const float l = max0(b - a);
    return l > 0.0f ? expf(-(mv.sigma_t * l)) : 1.0f;
}

// ---- interiors of dielectrics (pt_set_material_interior; include/pt_api.h pins every operation): the medium bound to
// the type-2 or type-6 material a path inside it will leave through, read per lane from the launch's table
// the free flight of the unit number u on a segment whose hit is at t: the distance of the scatter vertex, or -1 when the segment reaches its
// hit (sigma_s = 0 draws nothing)
PT_DEV float interior_flight(float sigma_s, float u, float t) {
    if (!(sigma_s > 0.0f)) return -1.0f;
    const float d = medium_flight(sigma_s, u);
    return d < t ? d : -1.0f;
}
// Beer-Lambert over the length l, per channel; a channel without absorption is exactly 1
PT_DEV f3 interior_absorb(f3 sigma_a, float l) {
    return mk(sigma_a.x != 0.0f ? expf(-(sigma_a.x * l)) : 1.0f, sigma_a.y != 0.0f ? expf(-(sigma_a.y * l)) : 1.0f,
              sigma_a.z != 0.0f ? expf(-(sigma_a.z * l)) : 1.0f);
}

// ---- density grid of the medium (pt_set_medium_density; include/pt_api.h pins every operation): regular tracking
// through gv.n[0] x gv.n[1] x gv.n[2] piecewise-constant voxels of the medium's box, which is finite wherever this is called.
// Walk(P, D, t, tau): a 3-D DDA over the part [a, b] of [0, t] inside the box that accumulates the optical depth `acc` voxel by voxel and
// stops in the voxel where it reaches tau.  FLIGHT = false is the walk with tau = +inf (no voxel can reach it): the test is compiled out.
// The view and the box are wave-uniform (scalar operands); a lane carries three tnext, three tdelta, three indices and their steps, t_cur
// and acc.  The loop is counted -- n[0] + n[1] + n[2] + 3 trips at most, more than any straight line visits -- so no rounding can
// keep a lane in it, and every index is tested against the grid before the next load.  One scattered 4-byte load per trip; no divide
// in the loop but the one that decides a scatter, taken only where the depth left is within a factor two of the voxel's.
struct GridWalk {
    float a, b;          // Clip(P, D, t)
    float s;             // the scatter distance (t_cur + d), or -1
    float acc;           // the optical depth accumulated before the walk ended
    int visited;         // voxels visited
    int voxel;           // the linear index of the voxel the walk scattered in, or -1
};
template <bool FLIGHT>
PT_DEV GridWalk grid_walk(const MediumView& mv, const GridView& gv, f3 P, f3 D, float t, float tau) {
    GridWalk w;
    w.b = medium_clip(mv, P, D, t, &w.a);
    w.s = -1.0f;
    w.acc = 0.0f;
    w.visited = 0;
    w.voxel = -1;
    if (!(max0(w.b - w.a) > 0.0f)) return w;
    const float p[3] = {P.x, P.y, P.z}, dd[3] = {D.x, D.y, D.z};
    float tn[3], td[3];
    int ix[3], st[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const float inv = 1.0f / dd[ax];                                    // (Clip's own reciprocal)
        const float top = (float)(gv.n[ax] - 1);
        float g = __builtin_floorf((fmaf_(dd[ax], w.a, p[ax]) - mv.lo[ax]) * gv.inv_cell[ax]);
        g = g > 0.0f ? g : 0.0f;                                            // (a NaN lands on 0)
        g = g < top ? g : top;
        ix[ax] = (int)g;
        if (__builtin_fabsf(inv) < __builtin_inff()) {
            const bool up = inv > 0.0f;
            const int kb = ix[ax] + (up ? 1 : 0);                           // the plane the ray leaves the voxel through
            const float plane = kb == gv.n[ax] ? mv.hi[ax] : mv.lo[ax] + (float)kb * gv.cell[ax];
            st[ax] = up ? 1 : -1;
            tn[ax] = (plane - p[ax]) * inv;
            td[ax] = gv.cell[ax] * __builtin_fabsf(inv);
        } else {                                                            // parallel to the planes: the axis never steps
            st[ax] = 0;
            tn[ax] = __builtin_inff();
            td[ax] = 0.0f;
        }
    }
    float tx = tn[0], ty = tn[1], tz = tn[2];
    int i = ix[0], j = ix[1], k = ix[2];
    float tc = w.a, acc = 0.0f;
    const int trips = gv.n[0] + gv.n[1] + gv.n[2] + 3;
    for (int trip = 0; trip < trips; ++trip) {
        const int idx = (k * gv.n[1] + j) * gv.n[0] + i;                    // in the grid: clamped at entry, tested after every step
        const float sigma = mv.sigma_t * gv.rho[idx];
        ++w.visited;
        float te = ty < tx ? ty : tx;
        te = tz < te ? tz : te;
        te = w.b < te ? w.b : te;
        const float seg = max0(te - tc);
        if constexpr (FLIGHT) {
            // d < seg needs tau - acc < sigma seg up to rounding: where even twice that is not reached the divide is skipped, its answer known
            const float left = tau - acc;
            if (sigma > 0.0f && left < 2.0f * (sigma * seg)) {
                const float d = left / sigma;
                if (d < seg) {
                    w.s = tc + d;
                    w.voxel = idx;
                    break;
                }
            }
        }
        acc = acc + sigma * seg;
        if (te >= w.b) break;
        if (tx <= ty && tx <= tz) {
            i += st[0];
            tx += td[0];
            if ((unsigned)i >= (unsigned)gv.n[0]) break;
        } else if (ty <= tz) {
            j += st[1];
            ty += td[1];
            if ((unsigned)j >= (unsigned)gv.n[1]) break;
        } else {
            k += st[2];
            tz += td[2];
            if ((unsigned)k >= (unsigned)gv.n[2]) break;
        }
        tc = te;
    }
    w.acc = acc;
    return w;
}

// The light hook of shade_hit: three points in the segment body where k_nee (pt_nee.hip) adds next-event estimation.  Every
// statement that touches the hook sits under `if constexpr (HOOK::active)`, so the default instantiation (k_render, wf_shade)
// compiles exactly as without it -- plain empty inline methods change k_render's register allocation.
// A hook with `smooth` set also supplies the shading normal (option smooth_normals, pinned in include/pt_api.h): shading_normal()
// below, the specular vertex with its fall-back to the geometric normal (spec_vertex), and the geometric normal for the offsets.
// Every statement that does so sits under `if constexpr (HOOK::smooth)`.
// A hook with `textured` set (it has `smooth` too) also supplies the albedo of a type-0 vertex (option textures, pinned in
// include/pt_api.h): shading_normal_albedo() below, one evaluation of the barycentric weights for the normal and the uv; every
// statement that does so sits under `if constexpr (HOOK::textured)`.
// A hook with `glossy` set (it has `textured` too) makes rough materials lobe vertices (all pinned in include/pt_api.h): type 4, the rough
// metal of option glossy; with `coated` also type 5, the coated diffuse; with `frosted` (it has `lens`) also type 6, the rough dielectric,
// whose refracted direction leaves through the surface, so the vertex may toggle `inside` and step off along -Ng.  The hook's lobe_vertex()
// draws the direction (lobe_direction_rough() above, in place of diffuse_direction) and keeps the vertex's p_b; whether type 4 or 5 is
// live in a launch is the hook's answer (metal_live(), coat_live(); with `lights` also type 6: frost_live()).  The preview colour, light_sample, lobe_vertex, leaves_surface and end_vertex are
// one call each for every hook: what a hook's flags do not cover in their arguments it does not read.
// A hook with `medium` set (it has `lights`) may send a lane in at a scatter vertex of the medium instead of a hit (hook->scatters(); hp is
// then the vertex, ti is not read): the lane joins the lobe vertices for the one call of light_sample() -- so a wave that holds surface and
// scatter vertices runs one shadow traversal -- with type -1, and does nothing else here: no preview colour, no LCG draw, no new ray (the
// caller draws the direction from the phase function).
struct NoShadeHook {
    static constexpr bool active = false;
    static constexpr bool smooth = false;
    static constexpr bool textured = false;
    static constexpr bool glossy = false;
    static constexpr bool coated = false;
    static constexpr bool lens = false;
    static constexpr bool frosted = false;
    static constexpr bool lights = false;
    static constexpr bool medium = false;
};

// The interpolated shading normal of a hit at hp = madd(D, t, P) on packed triangle ti (include/pt_api.h pins every operation): vn =
// the packed vertex normals (k_pack_vertex_normals), N the record's normal, Ng = N flipped against the ray.  Ng itself -- the same
// bits -- when the triangle has none, when the weighted sum cannot be normalised or when the result faces away from the ray.
PT_DEV f3 shading_normal(const float4* __restrict__ vn, const float4* __restrict__ tris, int ti, f3 D, f3 hp, f3 N, f3 Ng) {
    const float4 q1 = vn[(size_t)ti * 3], q2 = vn[(size_t)ti * 3 + 1], q3 = vn[(size_t)ti * 3 + 2];
    if (q1.w == 0.0f) return Ng;
    const float4 a = tris[ti * 3], b = tris[ti * 3 + 1], c = tris[ti * 3 + 2];
    const f3 r1 = mk(a.x, a.y, a.z), r2 = mk(a.w, b.x, b.y), r3 = mk(b.z, b.w, c.x);
    const float a1 = max0(dot3(cross3(r3 - r2, hp - r2), N));
    const float a2 = max0(dot3(cross3(r1 - r3, hp - r3), N));
    const float a3 = max0(dot3(cross3(r2 - r1, hp - r1), N));
    const f3 s = madd(mk(q3.x, q3.y, q3.z), a3, madd(mk(q2.x, q2.y, q2.z), a2, mk(q1.x, q1.y, q1.z) * a1));
    const float l2 = dot3(s, s);
    if (!(l2 > 0.0f && l2 < __builtin_inff())) return Ng;
    f3 Ns = s * (1.0f / __builtin_sqrtf(l2));
    if (dot3(Ns, Ng) < 0.0f) Ns = -Ns;
    if (!(dot3(-D, Ns) > 0.0f)) return Ng;
    return Ns;
}

// ---- albedo textures (option textures; include/pt_api.h pins every operation)
// a stored half widened by the hardware convert (v_cvt_f32_f16)
PT_DEV float half_to_float(unsigned bits) { return (float)__builtin_bit_cast(_Float16, (unsigned short)bits); }
// texel (x, y) of the texture that starts at `first`: one 8-byte load; 0 <= x < w, 0 <= y < h
PT_DEV f3 texel_rgb(const uint2* __restrict__ texels, unsigned first, int w, int x, int y) {
    const uint2 q = texels[first + (unsigned)y * (unsigned)w + (unsigned)x];
    return mk(half_to_float(q.x & 0xffffu), half_to_float(q.x >> 16), half_to_float(q.y & 0xffffu));
}
// (i mod n + n) mod n for the i a lookup can produce, -1 <= i <= n, without a division; any other i (a uv that overflowed) lands in range too
PT_DEV int tex_wrap(int i, int n) {
    if (i < 0) i += n;
    if (i >= n) i -= n;
    return i < 0 ? 0 : i > n - 1 ? n - 1 : i;
}
// texture T at (u, v): repeat wrap, row 0 at the top, nearest or bilinear
PT_DEV f3 texture_lookup(const TexView& tv, int T, float u, float v) {
    const TexDesc d = tv.desc[T];
    const float fu = u - __builtin_floorf(u), fv = v - __builtin_floorf(v);
    const float w = (float)d.w, h = (float)d.h;
    if (d.filter == 0) {
        const int x = (int)__builtin_floorf(fu * w), y = (int)__builtin_floorf((1.0f - fv) * h);
        return texel_rgb(tv.texels, d.first, d.w, x < d.w - 1 ? (x < 0 ? 0 : x) : d.w - 1, y < d.h - 1 ? (y < 0 ? 0 : y) : d.h - 1);
    }
    const float px = fmaf_(fu, w, -0.5f), py = fmaf_(1.0f - fv, h, -0.5f);
    const float x0 = __builtin_floorf(px), y0 = __builtin_floorf(py);
    const float tx = px - x0, ty = py - y0;
    const int xa = tex_wrap((int)x0, d.w), ya = tex_wrap((int)y0, d.h);
    const int xb = xa + 1 < d.w ? xa + 1 : 0, yb = ya + 1 < d.h ? ya + 1 : 0;
    const f3 c00 = texel_rgb(tv.texels, d.first, d.w, xa, ya), c10 = texel_rgb(tv.texels, d.first, d.w, xb, ya);
    const f3 c01 = texel_rgb(tv.texels, d.first, d.w, xa, yb), c11 = texel_rgb(tv.texels, d.first, d.w, xb, yb);
    const f3 top = mk(fmaf_(tx, c10.x - c00.x, c00.x), fmaf_(tx, c10.y - c00.y, c00.y), fmaf_(tx, c10.z - c00.z, c00.z));
    const f3 bot = mk(fmaf_(tx, c11.x - c01.x, c01.x), fmaf_(tx, c11.y - c01.y, c01.y), fmaf_(tx, c11.z - c01.z, c01.z));
    return mk(fmaf_(ty, bot.x - top.x, top.x), fmaf_(ty, bot.y - top.y, top.y), fmaf_(ty, bot.z - top.z, top.z));
}

// shading_normal() and the textured albedo of the same hit with ONE evaluation of the weights a1, a2, a3: returns Ns as
// shading_normal does (vn == nullptr: no triangle has vertex normals) and multiplies *kd by the texel when the material mati has
// type 0 and a texture bound and the triangle has uvs; every other case leaves *kd alone.  Only lanes at such a hit run the lookup.
PT_DEV f3 shading_normal_albedo(const float4* __restrict__ vn, const TexView& tv, const float4* __restrict__ tris, int ti, f3 D, f3 hp, f3 N, f3 Ng, int type,
                                int mati, f3* kd) {
    float4 q1 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vn) q1 = vn[(size_t)ti * 3];
    const bool sn = q1.w != 0.0f;
    int T = -1;
    if (type == 0) T = tv.mat_tex[mati];
    float4 ub = make_float4(0.f, 0.f, 0.f, 0.f);
    if (T >= 0) ub = tv.uv[(size_t)ti * 2 + 1];
    const bool tx = ub.z != 0.0f;
    if (!sn && !tx) return Ng;
    const float4 a = tris[ti * 3], b = tris[ti * 3 + 1], c = tris[ti * 3 + 2];
    const f3 r1 = mk(a.x, a.y, a.z), r2 = mk(a.w, b.x, b.y), r3 = mk(b.z, b.w, c.x);
    const float a1 = max0(dot3(cross3(r3 - r2, hp - r2), N));
    const float a2 = max0(dot3(cross3(r1 - r3, hp - r3), N));
    const float a3 = max0(dot3(cross3(r2 - r1, hp - r1), N));
    if (tx) {
        const float A = (a1 + a2) + a3;
        if (A > 0.0f && A < __builtin_inff()) {
            const float4 ua = tv.uv[(size_t)ti * 2];
            const float inv = 1.0f / A;
            const float u = fmaf_(ub.x, a3, fmaf_(ua.z, a2, ua.x * a1)) * inv;
            const float v = fmaf_(ub.y, a3, fmaf_(ua.w, a2, ua.y * a1)) * inv;
            *kd = *kd * texture_lookup(tv, T, u, v);
        }
    }
    if (!sn) return Ng;
    const float4 q2 = vn[(size_t)ti * 3 + 1], q3 = vn[(size_t)ti * 3 + 2];
    const f3 s = madd(mk(q3.x, q3.y, q3.z), a3, madd(mk(q2.x, q2.y, q2.z), a2, mk(q1.x, q1.y, q1.z) * a1));
    const float l2 = dot3(s, s);
    if (!(l2 > 0.0f && l2 < __builtin_inff())) return Ng;
    f3 Ns = s * (1.0f / __builtin_sqrtf(l2));
    if (dot3(Ns, Ng) < 0.0f) Ns = -Ns;
    if (!(dot3(-D, Ns) > 0.0f)) return Ng;
    return Ns;
}

// one iteration body of prog.cl:317-366 for a ray that hit packed triangle `ti` at `t`
// (SK: double-precision constants pinned to scalar registers, see KC)
// REC: what is constant per triangle comes from its shading record p.shaderec[ti] (ShadeRec, pt_internal.hpp) instead of being
// gathered and recomputed at every hit.  First round trip: normal, type, mati, kd -- without the record the type waits for
// meta[ti] and then the material.  Second, once the flip is known: a lobe hit reads the frame of its orientation, every other
// case the material fields it needs through mati; a diffuse hit on a material without a specular lobe never touches the material.
template <bool SK, bool REC = false, class ST, class HOOK = NoShadeHook>
PT_DEV void shade_hit(f3& rP, f3& rD, ST& st, int& seed, bool& inside, const RenderParams& p, const float4* tris, const TriMeta* meta, int ti, float t,
                      HOOK* hook = nullptr) {
    bool sc = false;                                                        // medium: the lane is at a scatter vertex, not at a hit
    if constexpr (HOOK::medium) {
        sc = hook->scatters();
        // (a miss may scatter: the loads below stay in bounds)
        if (sc || ti < 0) ti = 0;
    }
    f3 N, kd;
    int type;
    bool plain;                                                             // type 0: ks is +0 and the pow is skipped
    const pt_material* __restrict__ m;
    const float4* rec = nullptr;
    if constexpr (REC) {
        rec = p.shaderec + (size_t)ti * (sizeof(ShadeRec) / sizeof(float4));
        const float4 a = rec[0], b = rec[1];
        N = mk(a.x, a.y, a.z);
        type = __float_as_int(a.w);
        kd = mk(b.x, b.y, b.z);
        const unsigned mi = (unsigned)__float_as_int(b.w);
        plain = (mi & kShadeRecPlain) != 0;
        m = &p.mats[mi & ~kShadeRecPlain];
    } else {
        const float4 c = tris[ti * 3 + 2];
        N = mk(c.y, c.z, c.w);
        m = &p.mats[meta[ti].mati];
        type = m->type;
        if constexpr (HOOK::medium) if (sc) type = -1;
        kd = mk(0.0f, 0.0f, 0.0f);      // (read from the material where it is needed)
        plain = false;
    }
    const f3 hp = madd(rD, t, rP);
    if constexpr (!HOOK::textured)
        if (p.iterations == 1) st.setC((REC ? kd : ldf3(m->kd)) + ldf3(m->emission));        // prog.cl:323-325
    const bool flip = dot3(rD, N) > 0.0f;
    if (flip) N = -N;                                                       // prog.cl:326-328
    // smooth shading: from here on N is the shading normal Ns; the hook keeps the geometric one (hook->Ng) for the offsets and the
    // geometric-side rules
    // textures: the same call also leaves the vertex's albedo kd' in the hook (hook->albedo), which the preview colour, the factor_L
    // update below and the light sample read instead of the material's kd
    if constexpr (HOOK::medium) {
        if (!sc) {
            N = hook->shading_attributes_at(p, tris, ti, rD, hp, flip ? -N : N, N, type, m);
            if (p.iterations == 1) st.setC((type == 4 && hook->metal_live() ? ldf3(m->F0) : hook->albedo(m)) + ldf3(m->emission));
        }
    } else if constexpr (HOOK::textured) {
        static_assert(HOOK::smooth && !REC, "the textured instances are built on the smooth ones");
        N = hook->shading_attributes_at(p, tris, ti, rD, hp, flip ? -N : N, N, type, m);
        if (p.iterations == 1) st.setC((type == 4 && hook->metal_live() ? ldf3(m->F0) : hook->albedo(m)) + ldf3(m->emission));
    } else if constexpr (HOOK::smooth) N = hook->shading_normal_at(tris, ti, rD, hp, flip ? -N : N, N);
    // Every material that continues the path ends the same way: normalise the new direction, step off the surface
    // along +-N.  The two sampling branches below only produce the direction BEFORE normalisation and the side; the
    // tail is shared, so a wave that holds both kinds of hit runs one normalisation (IEEE sqrt + divide), not two.
    bool lobe = type == 0 || type == 3;
    const bool spec = type == 1 || type == 2;
    bool gl = false;                                                        // a rough-metal vertex (type 4 under option glossy)
    if constexpr (HOOK::glossy) {
        static_assert(HOOK::textured, "the glossy instances are built on the textured ones");
        gl = type == 4;
        if constexpr (HOOK::coated) gl = gl && hook->metal_live();
        lobe = lobe || gl;
    }
    bool ct = false;                                                        // a coated-diffuse vertex (type 5 under option coated)
    if constexpr (HOOK::coated) {
        static_assert(HOOK::glossy, "the coated instances are built on the glossy ones");
        ct = type == 5;
        if constexpr (HOOK::lens) ct = ct && hook->coat_live();             // (the lens instances serve option coated = 0 too)
        lobe = lobe || ct;
    }
    bool fr = false;                                                        // a rough-dielectric vertex (type 6 under option frosted)
    if constexpr (HOOK::frosted) {
        static_assert(HOOK::lens, "the frosted instances are built on the lens ones");
        fr = type == 6;
        if constexpr (HOOK::lights) fr = fr && hook->frost_live();          // (the lights instances serve option frosted = 0 too)
        lobe = lobe || fr;
    }
    f3 dnew = rD;
    float side = 0.001f;
    float inten = 0.0f;
    float wb = 1.0f;                                                        // the hook's weight of this hit's emission
    if (lobe || sc) {
        // diffuse (prog.cl:329-340) and emitter (prog.cl:358-366) both continue with a cosine-
        // sampled ray drawn from two LCG values; the emitter's cosine uses the OLD direction.
        inten = max0(dot3(-rD, N));
        if constexpr (HOOK::active) {
            if (type == 3) wb = hook->emitter_weight(ti, t, inten, rD);
            hook->light_sample(st, p, m, type, N, hp, rD, inside);          // before the LCG draws and this hit's emission
        }
        if (!sc) {
            const float rnd1 = lcg_rand(seed), rnd2 = lcg_rand(seed);
            if constexpr (HOOK::glossy) dnew = hook->template lobe_vertex<SK>(st, m, gl, ct, fr, N, rD, rnd1, rnd2, inside, &side);
            else if constexpr (REC) dnew = diffuse_direction_rec<SK>(N, rec + (flip ? 4 : 2), rnd1, rnd2);
            else dnew = diffuse_direction<SK>(N, rnd1, rnd2);
        }
    } else if (spec) {
        // smooth shading: the vertex as a function of the normal, which may have to run twice (TWIN: NeeHook::spec_vertex restates the
        // branch below; a change to one belongs in the other)
        if constexpr (HOOK::smooth) {
            hook->spec_vertex(rD, st, seed, inside, m, type, N, &dnew, &side);
        } else {
            // mirror (prog.cl:341-345) and dielectric (prog.cl:346-357, 228-245) share the Fresnel
            // term and the mirror direction; the dielectric may pick the refracted direction instead.
            const f3 oldD = rD;
            const f3 F0 = ldf3(m->F0);
            const f3 F = fresnel(F0, N, oldD);
            dnew = oldD - (N * dot3(N, oldD)) * 2.0f;
            if (type == 2) {
                float n = m->n;
                if (inside) n = 1.0f / n;
                const float rnd = lcg_rand(seed);
                const float cosa = dot3(-oldD, N);
                const float disc = 1.0f - (fmaf_(-cosa, cosa, 1.0f) / n) / n;
                const float prob = ((F.x + F.y) + F.z) / 3.0f;
                const bool refr = disc > 0.0f && rnd > prob;
                if (refr) {
                    const f3 dn = mk(oldD.x / n, oldD.y / n, oldD.z / n);
                    dnew = madd(N, cosa / n - sqrt_rn(disc), dn);
                    const float k = 1.0f / (1.0f - prob);
                    st.setR((st.R() * mk(1.0f - F.x, 1.0f - F.y, 1.0f - F.z)) * k);
                    inside = !inside;
                    side = -0.001f;
                } else {
                    const float k = 1.0f / prob;
                    st.setR((st.R() * F) * k);
                }
            } else {
                st.setS(st.S() * F);
            }
        }
    }
    if (lobe || spec) {
        // a lobe direction below the geometric surface ends the path (frosted: a refracted one, side < 0, that is not below it)
        if constexpr (HOOK::smooth) hook->leaves_surface(lobe, side < 0.0f, dnew);
        rD = normalize3(dnew);
        if constexpr (HOOK::smooth) rP = madd(hook->geo(N), side, hp);
        else rP = madd(N, side, hp);
    }
    if (type == 0) {
        const float idiff = max0(dot3(rD, N));
        if constexpr (HOOK::textured) st.setL(st.L() * (hook->albedo(m) * idiff));
        else st.setL(st.L() * ((REC ? kd : ldf3(m->kd)) * idiff));
        // m->_pad = 1: ks is exactly 0 and shininess is finite >= 0, so ks * pow(...) is +-0 whatever the
        // (finite) power is -- skip the halfway vector (two normalisations) and the double-precision pow
        // (set by pt_upload_materials)
        // (REC and `plain`: ks is +0 in every component, and ks * 1.0f is ks)
        if (REC && plain) {
            st.setB(st.B() * mk(0.0f, 0.0f, 0.0f));
        } else {
            float pw = 1.0f;
            if (!m->_pad) {
                const f3 view = normalize3(ldf3(p.cam.eye) - hp);
                const f3 halfway = normalize3(view + rD);
                const float ispec = max0(dot3(N, halfway));
                pw = spec_pow<SK>(ispec, m->shininess);
            }
            st.setB(st.B() * (ldf3(m->ks) * pw));
        }
    } else if (type == 3) {
        const f3 e = ((ldf3(m->emission) * (st.L() + st.B())) * st.S()) * st.R();
        if constexpr (HOOK::active) st.setC(madd(e * wb, inten, st.C()));
        else st.setC(madd(e, inten, st.C()));
    }
    // any other type: the ray is left unchanged and the loop hits the same surface again
    // (frosted: after a refracted direction the next emitter hit or sky miss has weight 1, as after a specular vertex)
    if constexpr (HOOK::active) hook->end_vertex(lobe && !(fr && side < 0.0f), gl || ct || fr, N, rD);
}

PT_DEV f3 running_mean(f3 acc, f3 color, int s) {   // prog.cl:379
    const float cs = (float)s, cs1 = (float)(s + 1);
    return mk(fmaf_(acc.x, cs, color.x) / cs1, fmaf_(acc.y, cs, color.y) / cs1, fmaf_(acc.z, cs, color.z) / cs1);
}

// option "moments" (pt_api.h): the running mean of prog.cl:379 over the squared luminance of the samples, kept in colors[].w
PT_DEV float luminance(f3 c) { return fmaf_(0.0722f, c.z, fmaf_(0.7152f, c.y, 0.2126f * c.x)); }
PT_DEV float running_moment(float m2, f3 color, int s) {
    const float l = luminance(color);
    return fmaf_(m2, (float)s, l * l) / (float)(s + 1);
}

// ---------------------------------------------------------------------------- LDS staging

// Nodes staged in LDS are re-laid out on the way in: the three box quads {L.lo, L.hi, R.lo, R.hi}
// become {L.lo, R.lo, L.hi, R.hi}, so that one 8-byte read at (quad + 0 | 8) returns the entry
// (or exit) planes of BOTH children for a ray whose direction sign on that axis is known
// (Trav::node_step, kVisitLds), and the child slots of the fourth quad are re-encoded to the 16-bit
// reference form.  The treelet of a large tree is staged verbatim (kVisitFlat reads both copies alike).
PT_DEV unsigned stage_ref(float slot) {
    const int r = __float_as_int(slot);
    return (unsigned)(r < 0 ? (0x8000 | ~r) : r) & 0xffffu;
}
template <int MODE>
PT_DEV void stage_nodes(const RenderParams& p, float4* lds_nodes) {
    if (MODE != kNodesLds) {                     // the treelet of a large tree: verbatim
        const int nn = p.treelet_nodes * 4;
        for (int i = threadIdx.x; i < nn; i += blockDim.x) lds_nodes[i] = p.nodes[i];
        return;
    }
    // whole tree: kLdsNodeBytes per node -- {L.lo, R.lo, L.hi, R.hi} per axis, then left | right << 16
    char* out = reinterpret_cast<char*>(lds_nodes);
    const int nn = p.n_nodes * 4;
    for (int i = threadIdx.x; i < nn; i += blockDim.x) {
        const float4 q = p.nodes[i];
        char* nb = out + (unsigned)(i >> 2) * (unsigned)kLdsNodeBytes;
        if ((i & 3) != 3) {
            float2* d = reinterpret_cast<float2*>(nb + (i & 3) * 16);
            d[0] = make_float2(q.x, q.z);
            d[1] = make_float2(q.y, q.w);
        } else {
            *reinterpret_cast<unsigned*>(nb + 48) = stage_ref(q.x) | (stage_ref(q.y) << 16);
        }
    }
}

// LDS layout of every traversal kernel: [per-lane stacks: stack_entries x BLOCK entries][staged nodes][flat packets]
template <int MODE, int BLOCK>
PT_DEV size_t traversal_stack_bytes_dev(const RenderParams& p) {
    return ((size_t)p.stack_entries * sizeof(typename StackOf<MODE>::type) * BLOCK + 15) & ~(size_t)15;
}
template <int MODE, int BLOCK>
PT_DEV size_t traversal_nodes_end_dev(const RenderParams& p) {
    return traversal_stack_bytes_dev<MODE, BLOCK>(p) + (MODE == kNodesLds ? (((size_t)p.n_nodes * kLdsNodeBytes + 15) & ~(size_t)15) : MODE == kNodesTreelet ? (size_t)p.treelet_nodes * 64 : 0);
}
template <int MODE, int BLOCK>
PT_DEV size_t traversal_lds_bytes_dev(const RenderParams& p) {      // == traversal_lds_bytes() on the host
    return traversal_nodes_end_dev<MODE, BLOCK>(p) + (size_t)p.n_flat * 100;    // packets + boxes + box-group masks of the big-triangle list
}
template <int MODE, int BLOCK>
PT_DEV void setup_traversal(const RenderParams& p, SceneView* sv, LaneStack<typename StackOf<MODE>::type>* stk) {
    typedef typename StackOf<MODE>::type StackT;
    stk->base = reinterpret_cast<StackT*>(pt_lds_raw) + threadIdx.x;          // [entry][lane]
    stk->stride = BLOCK;
    sv->nodes = p.nodes;
    sv->tris = p.tris;
    sv->meta = p.meta;
    sv->treelet = (unsigned)p.treelet_nodes;
    sv->n_flat = p.n_flat;
    sv->lds_nodes = nullptr;
    sv->lds_entries = p.stack_entries;
    sv->node_min_lanes = p.node_min_lanes;
    sv->leaf_min_lanes = p.leaf_min_lanes;
    sv->ovf = p.stack_ovf ? p.stack_ovf + (size_t)(blockIdx.y * gridDim.x + blockIdx.x) * BLOCK : nullptr;
    sv->ovf_stride = (unsigned)p.stack_ovf_lanes;
    float4* lds_flat = reinterpret_cast<float4*>(pt_lds_raw + traversal_nodes_end_dev<MODE, BLOCK>(p));
    // (the copy flat_pass tests: corner (c + rot) % 3 of the packet is its corner c, so that the halves of a paired wall start at
    // the same corner -- fpair_rot, plan_flat_pairs; N stays but for the sign of its zeros, fpair_canon)
    {
        const float* src = reinterpret_cast<const float*>(p.tris);
        float* dst = reinterpret_cast<float*>(lds_flat);
        for (int i = threadIdx.x; i < p.n_flat * 12; i += BLOCK) {
            const int t = i / 12, j = i - t * 12;
            const int rot = MODE == kNodesLds ? (int)(p.fpair_rot >> (2 * t)) & 3 : 0;      // (the other node modes test no pairs)
            const float v = src[t * 12 + (j < 9 ? (j + 3 * rot) % 9 : j)];
            dst[i] = (MODE == kNodesLds && j >= 9 && (p.fpair_canon >> t & 1u) != 0 && v == 0.0f) ? 0.0f : v;      // (-0 in N -> +0)
        }
    }
    sv->lds_flat = lds_flat;
    sv->fpair = p.fpair_mask;
    // padded boxes of the listed triangles (what padded_bounds() gives a triangle in a leaf: 1e-5 of the largest
    // coordinate + 1e-6), per axis {lo, hi, hi, lo} so that (entry, exit) is one 8-byte read at + 0 or + 8
    float* lds_fbox = reinterpret_cast<float*>(lds_flat + p.n_flat * 3);
    unsigned* lds_fmask = reinterpret_cast<unsigned*>(lds_fbox + p.n_flat * 12);
    for (int i = threadIdx.x; i < p.n_fbox; i += BLOCK) {
        const int t = p.fbox_rep[i];
        lds_fmask[i] = p.fbox_mask[i];
        const float4 a = p.tris[t * 3], b = p.tris[t * 3 + 1], c = p.tris[t * 3 + 2];
        const float lox = fminf(fminf(a.x, a.w), b.z), hix = fmaxf(fmaxf(a.x, a.w), b.z);
        const float loy = fminf(fminf(a.y, b.x), b.w), hiy = fmaxf(fmaxf(a.y, b.x), b.w);
        const float loz = fminf(fminf(a.z, b.y), c.x), hiz = fmaxf(fmaxf(a.z, b.y), c.x);
        const float mx = fmaxf(__builtin_fabsf(lox), __builtin_fabsf(hix)), my = fmaxf(__builtin_fabsf(loy), __builtin_fabsf(hiy));
        const float mz = fmaxf(__builtin_fabsf(loz), __builtin_fabsf(hiz));
        const float pad = fmaxf(fmaxf(mx, my), mz) * 1e-5f + 1e-6f;
        float4* rec = reinterpret_cast<float4*>(lds_fbox + i * 12);
        rec[0] = make_float4(lox - pad, hix + pad, hix + pad, lox - pad);
        rec[1] = make_float4(loy - pad, hiy + pad, hiy + pad, loy - pad);
        rec[2] = make_float4(loz - pad, hiz + pad, hiz + pad, loz - pad);
    }
    sv->lds_fbox = reinterpret_cast<const char*>(lds_fbox);
    sv->lds_fmask = lds_fmask;
    sv->n_fbox = p.n_fbox;
    if (MODE == kNodesLds || MODE == kNodesTreelet) {
        float4* lds_nodes = reinterpret_cast<float4*>(pt_lds_raw + traversal_stack_bytes_dev<MODE, BLOCK>(p));
        stage_nodes<MODE>(p, lds_nodes);
        sv->lds_nodes = lds_nodes;
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------- per-lane traversal kernels (host side)
// k_debug_closest_hit, k_aovs and k_nee: one lane per item, persistent blocks of the node mode's per-lane size, at most
// 2048 / BLOCK blocks per CU.  pick(LaneShape<MODE, BLOCK>{}) names the kernel instance; it is launched with (p, args...).
template <int MODE, int BLOCK>
struct LaneShape {
    static constexpr int mode = MODE, block = BLOCK;
};
// the workgroup size of the calling thread's last launch_lanes_t launch (host data; 0: none since the caller cleared it): how a caller
// reports the shape its launch took without a second copy of the switch statements that choose it (launch_nee)
inline thread_local int t_lanes_block = 0;
// `mark` is keyed on (PICK, MODE, BLOCK) -- PICK is the caller's own lambda -- so there is one per kernel instance
template <int MODE, int BLOCK, class PICK, class... A>
hipError_t launch_lanes_t(PICK pick, const RenderParams& p, int64_t n, int cu_count, hipStream_t stream, A... args) {
    const auto kern = pick(LaneShape<MODE, BLOCK>{});
    const size_t lds = traversal_lds_bytes(p, BLOCK);
    static LdsMark mark;
    const hipError_t e = ensure_dynamic_lds((const void*)kern, mark, lds);
    if (e != hipSuccess) return e;
    const long long need = (n + BLOCK - 1) / BLOCK;
    const int blocks = (int)std::min<long long>(need, (long long)cu_count * (2048 / BLOCK));
    if (p.stack_ovf && (long long)blocks * BLOCK > (long long)p.stack_ovf_lanes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(BLOCK), lds, stream, p, args...);
    t_lanes_block = BLOCK;
    return hipGetLastError();
}
template <class PICK, class... A>
hipError_t launch_lanes(PICK pick, const RenderParams& p, int64_t n, int cu_count, hipStream_t stream, A... args) {
    if (n == 0) return hipSuccess;
    switch (p.node_mode) {
    case kNodesLds: return launch_lanes_t<kNodesLds, 512>(pick, p, n, cu_count, stream, args...);
    case kNodesGlobal: return launch_lanes_t<kNodesGlobal, 256>(pick, p, n, cu_count, stream, args...);
    case kNodesWide: return launch_lanes_t<kNodesWide, 256>(pick, p, n, cu_count, stream, args...);
    case kNodesTreelet: return launch_lanes_t<kNodesTreelet, 1024>(pick, p, n, cu_count, stream, args...);
    }
    return hipErrorInvalidValue;
}

// statistics live in kStatRows rows of 8 counters; a block adds to the row picked by its index, so
// no single address sees more than a few dozen atomics per launch (one address saturates at
// ~88 atomics/us on MI355X, which cost a 32k-wave launch ~0.4 ms when every wave hit one word)
PT_DEV void stat_add(const RenderParams& p, int slot, unsigned long long v) {
    atomicAdd(&p.stats[(size_t)((blockIdx.x + blockIdx.y * 37u) % kStatRows) * kStatCols + slot], v);
}

PT_DEV unsigned long long wave_sum(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

}  // namespace ptamd
