// pt_denoise.hip -- guide buffers (pt_render_aovs) and the edge-avoiding a-trous filter over them (pt_denoise).
//   k_aovs      one lane per local pixel, persistent blocks: n x n fixed sub-pixel camera rays through the render kernels'
//               traversal (pt_device.hpp), a short deterministic specular chain, then albedo / normal / depth (include/pt_api.h)
//               k_aovs<.., AovShade>: the same pass with the shading normal and the textured albedo of the NEE path (pt_render_aovs_ex)
//               k_aovs<.., AovLights>, k_aovs<.., AovShade, AovLights>: either pass seeing the sphere lights and the suns (option aov_lights)
//   k_atrous    one launch per iteration, 32x8 blocks, 5x5 taps at step 2^i; demodulation fused into the first launch and
//               remodulation into the last
// The specular step below restates what shade_hit does for types 1 and 2 without the random draw.
#include "pt_device.hpp"

namespace ptamd {

// ---------------------------------------------------------------------------- AOV pass
// The shaded form (pt_render_aovs_ex with PT_AOV_SHADED) takes one more argument, an AovShade: every chain hit then runs
// shading_normal_albedo() as k_nee does, the specular step is evaluated with Ns and falls back to Ng on the wrong geometric side, offsets
// use Ng, and the terminal hit gives Ns and the textured albedo (pinned in include/pt_api.h).  The loads that adds happen once per chain
// hit, outside the traversal.  Without the argument the kernel compiles to what it was before the shaded form existed.
struct AovShade {
    const float4* vn;              // packed vertex normals; nullptr: option smooth_normals is off
    TexView tv;                    // tv.uv == nullptr: option textures is off
    int glossy;                    // option glossy: a terminal type-4 hit is a metal (albedo tint x F0)
    int coated;                    // option coated: a terminal type-5 hit is a plastic (albedo tint x kd')
    int frosted;                   // option frosted: a terminal type-6 hit is a rough dielectric (albedo tint x 1)
};
// The lit forms (option aov_lights with an area set that has a non-black light) take an AovLights last: after every closest_hit of a chain the
// nearest sphere light in front of the triangle ends the chain, and a miss takes the suns whose disc holds the direction (pinned in
// include/pt_api.h).  The view is a kernel argument by value, so the loops over the records have a wave-uniform trip count and wave-uniform
// addresses, as in k_nee; they run once per chain hit, outside the traversal.  Every statement of the lit forms sits under if constexpr (LIT).
struct AovLights {
    AreaLightsView v;
};
template <class... SH>
PT_DEV const AovShade& only(const AovShade& s, const SH&...) { return s; }
PT_DEV const AreaLightsView& lights_of(const AovLights& l) { return l.v; }
PT_DEV const AreaLightsView& lights_of(const AovShade&, const AovLights& l) { return l.v; }
template <class T, class... SH>
constexpr bool aov_has = (std::is_same<T, SH>::value || ...);

// the lit guides' test after the closest_hit (ti, t) of the ray (P, D), with the chain's tint: 1 the chain ends on a sphere light at *ts, 2 it
// ends on a miss (under the suns whose disc holds D, if any), 0 it goes on with triangle ti
PT_DEV int aov_light_end(const AreaLightsView& v, f3 P, f3 D, int ti, float t, f3 tint, f3* alb, f3* nrm, float* mat, float* ts) {
    const int j = area_sphere_hit(v, P, D, ti >= 0 ? t : __builtin_inff(), -1, ts);
    if (j >= 0) {
        const float4 q0 = v.rec[3 * j], q1 = v.rec[3 * j + 1];
        *alb = tint * mk(q1.x, q1.y, q1.z);
        *nrm = normalize3(madd(D, *ts, P) - mk(q0.x, q0.y, q0.z));
        *mat = (float)(-2 - j);
        return 1;
    }
    if (ti >= 0) return 0;
    const unsigned long long mask = area_sun_mask(v, D);
    if (mask) {
        f3 L = mk(0.f, 0.f, 0.f);
        int first = -1;
        for (int k = v.n_sphere; k < v.n; ++k) {
            if (!((mask >> (k - v.n_sphere)) & 1ull)) continue;
            const float4 q1 = v.rec[3 * k + 1];
            L = L + mk(q1.x, q1.y, q1.z);
            if (first < 0) first = k;
        }
        *alb = tint * L;
        *mat = (float)(-2 - first);
    }
    return 2;
}

template <int MODE, int BLOCK, class... SH>
__global__ void __launch_bounds__(BLOCK) k_aovs(RenderParams p, int sub, int spec_depth, long long npix, float4* albedo_rgbm, float4* normal_depth,
                                                SH... shade) {
    constexpr bool SHADED = aov_has<AovShade, SH...>, LIT = aov_has<AovLights, SH...>;
    LaneStack<typename StackOf<MODE>::type> stk;
    SceneView sv;
    setup_traversal<MODE, BLOCK>(p, &sv, &stk);
    WorkCount wc;
    const float fn = (float)sub;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < npix; i += (long long)gridDim.x * BLOCK) {
        const int lrow = (int)(i / p.width), x = (int)(i % p.width);
        const int grow = global_row(p, lrow);
        const int gid = grow * p.width + x;
        f3 sa = mk(0.f, 0.f, 0.f), sn = sa;
        float st = 0.0f;
        int hits = 0;
        float mat0 = -1.0f;
        for (int j = 0; j < sub; ++j) {
            for (int k = 0; k < sub; ++k) {
                f3 P, D;
                camera_get_ray(gid, p.cam, ((float)k + 0.5f) / fn, ((float)j + 0.5f) / fn, &P, &D);
                float t;
                int ti = closest_hit<MODE, false>(sv, P, D, stk, &t, &wc);
                f3 alb = mk(0.f, 0.f, 0.f), nrm = alb;
                float mat = -1.0f;
                bool chain = ti >= 0;
                if constexpr (LIT) {
                    float ts;
                    const int e = aov_light_end(lights_of(shade...), P, D, ti, t, mk(1.f, 1.f, 1.f), &alb, &nrm, &mat, &ts);
                    if (e == 1) {           // a sphere light ends the primary ray: a hit, also where no triangle was
                        st += ts;
                        ++hits;
                    }
                    chain = e == 0;
                }
                if (chain) {
                    st += t;
                    ++hits;
                    f3 tint = mk(1.f, 1.f, 1.f);
                    bool inside = false;
                    for (int d = 0;; ++d) {
                        const float4 c = p.tris[ti * 3 + 2];
                        f3 N = mk(c.y, c.z, c.w);
                        const int mi = p.meta[ti].mati;
                        const pt_material* __restrict__ m = &p.mats[mi];
                        const int type = m->type;
                        if constexpr (SHADED) {
                            const f3 Ng = dot3(D, N) > 0.0f ? -N : N;
                            const f3 hp = madd(D, t, P);
                            f3 kd = mk(0.f, 0.f, 0.f);
                            const AovShade& sh = only(shade...);
                            const bool plastic = type == 5 && sh.coated;
                            if (type == 0 || type == 3 || plastic) kd = ldf3(m->kd);
                            const f3 Ns = shading_normal_albedo(sh.vn, sh.tv, p.tris, ti, D, hp, N, Ng, sh.tv.uv ? (plastic ? 0 : type) : -1, mi, &kd);
                            if ((type == 1 || type == 2) && d < spec_depth) {
                                float n = 1.0f;
                                if (type == 2) {
                                    n = m->n;
                                    if (inside) n = 1.0f / n;
                                }
                                f3 dnew;
                                bool refr;
                                auto eval = [&](f3 Nx) {
                                    dnew = D - (Nx * dot3(Nx, D)) * 2.0f;
                                    refr = false;
                                    if (type == 2) {
                                        const float cosa = dot3(-D, Nx);
                                        const float disc = 1.0f - (fmaf_(-cosa, cosa, 1.0f) / n) / n;
                                        if (disc > 0.0f) {
                                            const f3 dn = mk(D.x / n, D.y / n, D.z / n);
                                            dnew = madd(Nx, cosa / n - __builtin_sqrtf(disc), dn);
                                            refr = true;
                                        }
                                    }
                                };
                                eval(Ns);
                                const float g = dot3(dnew, Ng);
                                if (refr ? g >= 0.0f : g <= 0.0f) eval(Ng);      // the wrong geometric side: once more with Ng, and that stands
                                if (type == 1) tint = tint * ldf3(m->F0);
                                if (refr) inside = !inside;
                                D = normalize3(dnew);
                                P = madd(Ng, refr ? -0.001f : 0.001f, hp);
                                ti = closest_hit<MODE, false>(sv, P, D, stk, &t, &wc);
                                if constexpr (LIT) {
                                    float ts;
                                    if (aov_light_end(lights_of(shade...), P, D, ti, t, tint, &alb, &nrm, &mat, &ts)) break;
                                } else if (ti < 0) break;   // escaped: albedo 0, normal 0
                                continue;
                            }
                            const f3 a = type == 1 || (type == 4 && sh.glossy) ? ldf3(m->F0) : type == 2 || (type == 6 && sh.frosted) ? mk(1.f, 1.f, 1.f) : plastic ? kd : kd + ldf3(m->emission);
                            alb = tint * a;
                            nrm = Ns;
                            mat = (float)mi;
                            break;
                        }
                        if (dot3(D, N) > 0.0f) N = -N;
                        if ((type == 1 || type == 2) && d < spec_depth) {
                            const f3 hp = madd(D, t, P);
                            f3 dnew = D - (N * dot3(N, D)) * 2.0f;
                            float side = 0.001f;
                            if (type == 1) {
                                tint = tint * ldf3(m->F0);
                            } else {
                                float n = m->n;
                                if (inside) n = 1.0f / n;
                                const float cosa = dot3(-D, N);
                                const float disc = 1.0f - (fmaf_(-cosa, cosa, 1.0f) / n) / n;
                                if (disc > 0.0f) {
                                    const f3 dn = mk(D.x / n, D.y / n, D.z / n);
                                    dnew = madd(N, cosa / n - __builtin_sqrtf(disc), dn);
                                    inside = !inside;
                                    side = -0.001f;
                                }
                            }
                            D = normalize3(dnew);
                            P = madd(N, side, hp);
                            ti = closest_hit<MODE, false>(sv, P, D, stk, &t, &wc);
                            if constexpr (LIT) {
                                float ts;
                                if (aov_light_end(lights_of(shade...), P, D, ti, t, tint, &alb, &nrm, &mat, &ts)) break;
                            } else if (ti < 0) break;       // escaped: albedo 0, normal 0
                            continue;
                        }
                        const f3 a = type == 1 ? ldf3(m->F0) : type == 2 ? mk(1.f, 1.f, 1.f) : ldf3(m->kd) + ldf3(m->emission);
                        alb = tint * a;
                        nrm = N;
                        mat = (float)mi;
                        break;
                    }
                }
                if (j == 0 && k == 0) mat0 = mat;
                sa = sa + alb;
                sn = sn + nrm;
            }
        }
        const float n2 = (float)(sub * sub);
        albedo_rgbm[i] = make_float4(sa.x / n2, sa.y / n2, sa.z / n2, mat0);
        f3 nout = mk(0.f, 0.f, 0.f);
        if (sn.x != 0.0f || sn.y != 0.0f || sn.z != 0.0f) {
            const float s = 1.0f / __builtin_sqrtf((sn.x * sn.x + sn.y * sn.y) + sn.z * sn.z);
            nout = sn * s;
        }
        normal_depth[i] = make_float4(nout.x, nout.y, nout.z, hits ? st / (float)hits : -1.0f);
    }
}

// lights == nullptr: the unlit instances, which are what they were before the lit ones existed
hipError_t launch_aovs_shaded(const RenderParams& p, int32_t subpixels, int32_t specular_depth, int64_t npix, float4* albedo_rgbm, float4* normal_depth,
                              const float4* vn, const TexView& tv, int glossy, int coated, int frosted, const AreaLightsView* lights, int cu_count,
                              hipStream_t stream) {
    const AovShade sh{vn, tv, glossy, coated, frosted};
    if (lights)
        return launch_lanes([](auto s) { return k_aovs<s.mode, s.block, AovShade, AovLights>; }, p, npix, cu_count, stream, subpixels, specular_depth,
                            (long long)npix, albedo_rgbm, normal_depth, sh, AovLights{*lights});
    return launch_lanes([](auto s) { return k_aovs<s.mode, s.block, AovShade>; }, p, npix, cu_count, stream, subpixels, specular_depth,
                        (long long)npix, albedo_rgbm, normal_depth, sh);
}

hipError_t launch_aovs(const RenderParams& p, int32_t subpixels, int32_t specular_depth, int64_t npix, float4* albedo_rgbm, float4* normal_depth,
                       const AreaLightsView* lights, int cu_count, hipStream_t stream) {
    if (lights)
        return launch_lanes([](auto s) { return k_aovs<s.mode, s.block, AovLights>; }, p, npix, cu_count, stream, subpixels, specular_depth,
                            (long long)npix, albedo_rgbm, normal_depth, AovLights{*lights});
    return launch_lanes([](auto s) { return k_aovs<s.mode, s.block>; }, p, npix, cu_count, stream, subpixels, specular_depth, (long long)npix,
                        albedo_rgbm, normal_depth);
}

// ---------------------------------------------------------------------------- a-trous iteration
PT_DEV f3 demod(float4 c, float4 a) {
    return mk(c.x / fmaxf(a.x, 1e-3f), c.y / fmaxf(a.y, 1e-3f), c.z / fmaxf(a.z, 1e-3f));
}

// FIRST: `in` is the context's colors, demodulated tap by tap when DEMOD; LAST: the result is remodulated when DEMOD
template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(256) k_atrous(const float4* __restrict__ in, float4* __restrict__ out, const float4* __restrict__ albedo,
                                                const float4* __restrict__ nd, int W, int H, AtrousStep s) {
    const int x = blockIdx.x * 32 + (threadIdx.x & 31);
    const int y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= W || y >= H) return;
    const float kern[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const size_t ip = (size_t)y * W + x;
    const float4 gp = nd[ip];
    const bool miss_p = gp.w < 0.0f, zero_np = gp.x == 0.0f && gp.y == 0.0f && gp.z == 0.0f;
    const float4 cp4 = in[ip];
    const f3 cp = (FIRST && s.demodulate) ? demod(cp4, albedo[ip]) : mk(cp4.x, cp4.y, cp4.z);
    f3 acc = mk(0.f, 0.f, 0.f);
    float wsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * s.step;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * s.step;
            if (qx < 0 || qx >= W) continue;
            const size_t iq = (size_t)qy * W + qx;
            const float4 gq = nd[iq];
            const bool miss_q = gq.w < 0.0f;
            if (miss_p != miss_q) continue;                     // w_z = 0 across a hit / miss boundary
            const float4 cq4 = in[iq];
            const f3 cq = (FIRST && s.demodulate) ? demod(cq4, albedo[iq]) : mk(cq4.x, cq4.y, cq4.z);
            float w = kern[dx + 2] * kern[dy + 2];
            if (dx == 0 && dy == 0) {                           // the centre tap: 9/64, every term 1
                wsum += w;
                continue;
            }
            if (s.color_on) {
                const f3 dc = cp - cq;
                const float d2 = (dc.x * dc.x + dc.y * dc.y) + dc.z * dc.z;
                if (d2 != 0.0f) w *= expf(-(d2 * s.color_scale) / s.sigma_color2);
            }
            if (s.normal_on && !zero_np && !(gq.x == 0.0f && gq.y == 0.0f && gq.z == 0.0f)) {
                const float dn = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
                w *= powf(fmaxf(dn, 0.0f), s.sigma_normal);
            }
            if (s.depth_on && !miss_p) {
                const float dz = fabsf(gp.w - gq.w);
                if (dz != 0.0f) w *= expf(-dz / (((s.sigma_depth * (float)s.step) * (float)max(abs(dx), abs(dy))) * gp.w));
            }
            acc = madd(cq - cp, w, acc);
            wsum += w;
        }
    }
    // x(p) + sum w (x(q) - x(p)) / sum w: the same weighted mean, and a flat neighbourhood comes out with the centre's bits
    f3 r = mk(cp.x + acc.x / wsum, cp.y + acc.y / wsum, cp.z + acc.z / wsum);
    if (LAST && s.demodulate) {
        const float4 a = albedo[ip];
        r = mk(r.x * fmaxf(a.x, 1e-3f), r.y * fmaxf(a.y, 1e-3f), r.z * fmaxf(a.z, 1e-3f));
    }
    out[ip] = make_float4(r.x, r.y, r.z, 1.0f);
}

// ---------------------------------------------------------------------------- variance of the mean luminance (pt_read_variance)
// n = tile_spp[tile of the pixel] (adaptive frames) or n_all; v = max(m2 - mu^2, 0) / (n - 1), +inf below two samples (pinned in pt_api.h)
__global__ void __launch_bounds__(256) k_variance(const float4* __restrict__ colors, const int32_t* __restrict__ tile_spp, int32_t n_all, int W,
                                                  long long npix, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    int n = n_all;
    if (tile_spp) {
        const int y = (int)(i / W), x = (int)(i - (long long)y * W);
        n = tile_spp[(y >> 3) * ((W + 7) >> 3) + (x >> 3)];
    }
    const float4 c = colors[i];
    const float mu = luminance(mk(c.x, c.y, c.z));
    out[i] = n < 2 ? __builtin_inff() : fmaxf(fmaf_(-mu, mu, c.w), 0.0f) / (float)(n - 1);
}

hipError_t launch_variance(const float4* colors, const int32_t* tile_spp, int32_t n_all, int32_t W, int64_t npix, float* out, hipStream_t stream) {
    if (npix <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_variance, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, colors, tile_spp, n_all, W, (long long)npix, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------- variance-guided a-trous iteration (pt_denoise_variance)
// x(p) and v(p) of an iteration's input: FIRST reads the context's colors and the variance read-out, demodulated when s.demodulate
// (x / max(a, 1e-3) per channel, v / max(l(a), 1e-3)^2); later iterations read the previous one's {x, v} float4
template <bool FIRST>
PT_DEV void load_xv(const float4* __restrict__ in, const float* __restrict__ var, const float4* __restrict__ albedo, size_t i, int demodulate,
                    f3* x, float* v) {
    const float4 c = in[i];
    if (FIRST) {
        float vv = var[i];
        if (demodulate) {
            const float4 a = albedo[i];
            *x = demod(c, a);
            const float la = fmaxf(luminance(mk(a.x, a.y, a.z)), 1e-3f);
            vv = vv / (la * la);
        } else {
            *x = mk(c.x, c.y, c.z);
        }
        *v = vv;
    } else {
        *x = mk(c.x, c.y, c.z);
        *v = c.w;
    }
}

template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(256) k_atrous_var(const float4* __restrict__ in, const float* __restrict__ var, float4* __restrict__ out,
                                                    const float4* __restrict__ albedo, const float4* __restrict__ nd, int W, int H, AtrousVarStep s) {
    const int x = blockIdx.x * 32 + (threadIdx.x & 31);
    const int y = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (x >= W || y >= H) return;
    const float kern[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const float gk[3] = {0.25f, 0.5f, 0.25f};
    const size_t ip = (size_t)y * W + x;
    const float4 gp = nd[ip];
    const bool miss_p = gp.w < 0.0f, zero_np = gp.x == 0.0f && gp.y == 0.0f && gp.z == 0.0f;
    f3 cp;
    float vp;
    load_xv<FIRST>(in, var, albedo, ip, s.demodulate, &cp, &vp);
    const float lp = luminance(cp);
    // g(p): the 3x3 blur of v, one pixel apart, normalised over the taps inside the frame
    float lum_scale = 0.0f;          // sigma_luminance sqrt(g(p)) + 1e-6; 0: the luminance term is off (weight 1)
    if (s.lum_on) {
        float gs = 0.0f, gw = 0.0f;
        for (int dy = -1; dy <= 1; ++dy) {
            const int qy = y + dy;
            if (qy < 0 || qy >= H) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = x + dx;
                if (qx < 0 || qx >= W) continue;
                f3 xq;
                float vq;
                load_xv<FIRST>(in, var, albedo, (size_t)qy * W + qx, s.demodulate, &xq, &vq);
                const float k = gk[dx + 1] * gk[dy + 1];
                gs = fmaf_(k, vq, gs);
                gw += k;
            }
        }
        const float g = gs / gw;
        if (g < __builtin_inff()) lum_scale = s.sigma_luminance * sqrtf(g) + 1e-6f;
    }
    f3 acc = mk(0.f, 0.f, 0.f);
    float wsum = 0.0f, vacc = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * s.step;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * s.step;
            if (qx < 0 || qx >= W) continue;
            const size_t iq = (size_t)qy * W + qx;
            const float4 gq = nd[iq];
            const bool miss_q = gq.w < 0.0f;
            if (miss_p != miss_q) continue;                     // w_z = 0 across a hit / miss boundary
            f3 cq;
            float vq;
            load_xv<FIRST>(in, var, albedo, iq, s.demodulate, &cq, &vq);
            float w = kern[dx + 2] * kern[dy + 2];
            if (!(dx == 0 && dy == 0)) {                        // the centre tap: 9/64, every term 1
                if (lum_scale > 0.0f) {
                    const float dl = fabsf(lp - luminance(cq));
                    if (dl != 0.0f) w *= expf(-dl / lum_scale);
                }
                if (s.normal_on && !zero_np && !(gq.x == 0.0f && gq.y == 0.0f && gq.z == 0.0f)) {
                    const float dn = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
                    w *= powf(fmaxf(dn, 0.0f), s.sigma_normal);
                }
                if (s.depth_on && !miss_p) {
                    const float dz = fabsf(gp.w - gq.w);
                    if (dz != 0.0f) w *= expf(-dz / (((s.sigma_depth * (float)s.step) * (float)max(abs(dx), abs(dy))) * gp.w));
                }
                if (w == 0.0f) continue;                        // a tap of weight 0 adds nothing (not even 0 x inf to the variance)
            }
            acc = madd(cq, w, acc);
            vacc = fmaf_(w * w, vq, vacc);
            wsum += w;
        }
    }
    f3 r = mk(acc.x / wsum, acc.y / wsum, acc.z / wsum);
    float rv = vacc / (wsum * wsum);
    if (LAST && s.demodulate) {
        const float4 a = albedo[ip];
        r = mk(r.x * fmaxf(a.x, 1e-3f), r.y * fmaxf(a.y, 1e-3f), r.z * fmaxf(a.z, 1e-3f));
        const float la = fmaxf(luminance(mk(a.x, a.y, a.z)), 1e-3f);
        rv = rv * (la * la);
    }
    out[ip] = make_float4(r.x, r.y, r.z, rv);
}

hipError_t launch_atrous_var(const float4* in, const float* var, float4* out, const float4* albedo, const float4* nd, int32_t W, int32_t H,
                             const AtrousVarStep& s, bool first, bool last, hipStream_t stream) {
    const dim3 grid((W + 31) / 32, (H + 7) / 8), block(256);
    if (first && last) hipLaunchKernelGGL((k_atrous_var<true, true>), grid, block, 0, stream, in, var, out, albedo, nd, W, H, s);
    else if (first) hipLaunchKernelGGL((k_atrous_var<true, false>), grid, block, 0, stream, in, var, out, albedo, nd, W, H, s);
    else if (last) hipLaunchKernelGGL((k_atrous_var<false, true>), grid, block, 0, stream, in, var, out, albedo, nd, W, H, s);
    else hipLaunchKernelGGL((k_atrous_var<false, false>), grid, block, 0, stream, in, var, out, albedo, nd, W, H, s);
    return hipGetLastError();
}

hipError_t launch_atrous(const float4* in, float4* out, const float4* albedo, const float4* nd, int32_t W, int32_t H, const AtrousStep& s,
                         bool first, bool last, hipStream_t stream) {
    const dim3 grid((W + 31) / 32, (H + 7) / 8), block(256);
    if (first && last) hipLaunchKernelGGL((k_atrous<true, true>), grid, block, 0, stream, in, out, albedo, nd, W, H, s);
    else if (first) hipLaunchKernelGGL((k_atrous<true, false>), grid, block, 0, stream, in, out, albedo, nd, W, H, s);
    else if (last) hipLaunchKernelGGL((k_atrous<false, true>), grid, block, 0, stream, in, out, albedo, nd, W, H, s);
    else hipLaunchKernelGGL((k_atrous<false, false>), grid, block, 0, stream, in, out, albedo, nd, W, H, s);
    return hipGetLastError();
}

}  // namespace ptamd
