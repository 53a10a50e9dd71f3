// pt_nee.hip -- next-event estimation with multiple importance sampling (pt_render_nee; the estimator is pinned in include/pt_api.h).
//   k_nee   one lane per local pixel, persistent blocks (like k_aovs): every sample of the pixel back to back, path state in
//           registers.  The segment body restates shade_hit's arithmetic -- shade_hit itself is not touched (every k_render
//           instance inlines it) -- and adds the MIS weight of an emitter hit after a lobe vertex and, at a lobe vertex, a light
//           sample: one shadow ray whose search is cut just past the sampled point.  The light sample's three numbers come from a
//           counter-based hash of (LCG state at the start of the sample, segment, dimension), never from the LCG, so the BSDF
//           path draws exactly what pt_render draws and rnds / rays come out the same in every strategy.
#include "pt_device.hpp"

#include <algorithm>

namespace ptamd {

PT_DEV unsigned lowbias32(unsigned x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
PT_DEV unsigned nee_rand(unsigned state, int segment, int dim) {        // == pt_nee_rand (pt_host.cpp)
    return lowbias32(lowbias32(state) + 0x9e3779b9u * (unsigned)(3 * segment + dim + 1));
}
PT_DEV float nee_unit(unsigned h) { return (float)(h >> 8) * 5.9604644775390625e-08f; }   // [0, 1), 24 bits

constexpr float kInvPi = 0.318309886183790672f;

// closest hit of (o, w) among the triangles nearer than `limit` (-1: none): the traversal starts with best_t = limit, so the
// big-triangle list and every node box behind the light sample are pruned from the first test
template <int MODE>
PT_DEV int shadow_hit(const SceneView& sv, f3 o, f3 w, float limit, const LaneStack<typename StackOf<MODE>::type> stk, WorkCount* wc) {
    Trav<MODE> tr;
    tr.begin(o, w, stk);
    tr.best_t = limit;
    tr.template flat_pass<false>(sv, wc);
    while (!tr.done()) tr.template round<false>(sv, wc);
    return tr.best;
}

template <int MODE, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_nee(RenderParams p, NeeTable lt, long long npix) {
    LaneStack<typename StackOf<MODE>::type> stk;
    SceneView sv;
    setup_traversal<MODE, BLOCK>(p, &sv, &stk);
    WorkCount wc;
    const bool nee = lt.n > 0 && lt.strategy != 0;
    const bool mis = lt.strategy == 2;
    const int camX = (int)p.cam.XM;
    const f3 eye = ldf3(p.cam.eye);
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < npix; i += (long long)gridDim.x * BLOCK) {
        const int lrow = (int)(i / p.width), x = (int)(i % p.width);
        const int grow = ((lrow / p.rows_per_block) * p.world + p.rank) * p.rows_per_block + lrow % p.rows_per_block;
        const int gid = grow * p.width + x;
        const float pix_x = (float)(gid % camX), pix_y = (float)(gid / camX);      // prog.cl:84-85
        int seed = p.rnds[i];
        f3 acc = mk(0.f, 0.f, 0.f);
        if (p.first_sample != 0) {                 // prog.cl:312-314: sample 0 starts from black
            const float4 c = p.colors[i];
            acc = mk(c.x, c.y, c.z);
        }
        f3 rP = mk(0.f, 0.f, 0.f), rD = mk(0.f, 0.f, 1.f);
        for (int s = p.first_sample; s < p.first_sample + p.nsamples; ++s) {
            const unsigned key = (unsigned)seed;    // the light samples' key: the LCG state at the start of the sample
            PathRegs st;
            st.reset();
            bool inside = false;
            {
                const float rnd1 = lcg_rand(seed), rnd2 = lcg_rand(seed);
                camera_get_ray_xy(pix_x, pix_y, p.cam, rnd1, rnd2, &rP, &rD);
            }
            bool after_lobe = false;               // the previous vertex was a lobe vertex (its flipped normal: Nprev)
            f3 Nprev = mk(0.f, 0.f, 0.f);
            for (int k = 0; k < p.iterations; ++k) {
                float t;
                const int ti = closest_hit<MODE, false>(sv, rP, rD, stk, &t, &wc);
                if (ti < 0) break;                 // black environment, prog.cl:367-376
                // ---- shade_hit (pt_device.hpp), restated with the two weights
                const float4 c = p.tris[ti * 3 + 2];
                f3 N = mk(c.y, c.z, c.w);
                const f3 hp = madd(rD, t, rP);
                const pt_material* __restrict__ m = &p.mats[p.meta[ti].mati];
                const int type = m->type;
                if (p.iterations == 1) st.setC(ldf3(m->kd) + ldf3(m->emission));   // prog.cl:323-325
                if (dot3(rD, N) > 0.0f) N = -N;
                const bool lobe = type == 0 || type == 3, spec = type == 1 || type == 2;
                f3 dnew = rD;
                float side = 0.001f;
                float inten = 0.0f;
                float wb = 1.0f;                   // weight of this hit's emission
                if (lobe) {
                    inten = max0(dot3(-rD, N));
                    if (type == 3 && nee && after_lobe) {
                        const float pa = lt.pdf_area[ti];
                        if (pa > 0.0f && inten > 0.0f) {
                            if (!mis) {
                                wb = 0.0f;
                            } else {
                                const float pb = max0(dot3(Nprev, rD)) * kInvPi;
                                const float pl = pa * (t * t) / inten;
                                const float rr = pl / pb;          // pb = 0: rr = inf, weight 0
                                wb = 1.0f / fmaf_(rr, rr, 1.0f);
                            }
                        }
                    }
                    if (nee && k + 1 < p.iterations) {
                        // ---- light sample: a point y on a light, the bracket an emitter hit at y on segment k + 1 would add
                        const float u0 = nee_unit(nee_rand(key, k, 0)), u1 = nee_unit(nee_rand(key, k, 1)), u2 = nee_unit(nee_rand(key, k, 2));
                        int lo = 0, hi = lt.n - 1;        // first light with cdf > u0
                        while (lo < hi) {
                            const int mid = (lo + hi) >> 1;
                            if (lt.cdf[mid] > u0) hi = mid;
                            else lo = mid + 1;
                        }
                        const int li = lt.tri[lo];
                        const float4 a = p.tris[li * 3], b = p.tris[li * 3 + 1], cc = p.tris[li * 3 + 2];
                        const f3 v1 = mk(a.x, a.y, a.z), v2 = mk(a.w, b.x, b.y), v3 = mk(b.z, b.w, cc.x), Ny = mk(cc.y, cc.z, cc.w);
                        const float su = __builtin_sqrtf(u1);
                        const f3 y = madd(v3 - v1, su * (1.0f - u2), madd(v2 - v1, u2 * su, v1));
                        const f3 o = madd(N, 0.001f, hp);
                        const f3 d = y - o;
                        const float r2 = dot3(d, d);
                        const float r = __builtin_sqrtf(r2);
                        const f3 w = mk(d.x / r, d.y / r, d.z / r);
                        const float cosx = dot3(N, w), cosy = __builtin_fabsf(dot3(w, Ny));
                        const float pl = lt.pdf_area[li] * r2 / cosy;
                        if (cosx > 0.0f && cosy > 0.0f && pl > 0.0f && pl < __builtin_inff()) {
                            if (shadow_hit<MODE>(sv, o, w, r * 1.0001f, stk, &wc) == li) {
                                const float pb = cosx * kInvPi;
                                const float q = pb / pl;
                                const float wl = mis ? q / fmaf_(q, q, 1.0f) : q;
                                f3 fl = st.L(), fb = st.B();
                                if (type == 0) {           // the factors x's own update with w would give (below)
                                    fl = fl * (ldf3(m->kd) * cosx);
                                    float pw = 1.0f;
                                    if (!m->_pad) {
                                        const f3 view = normalize3(eye - hp);
                                        const f3 halfway = normalize3(view + w);
                                        pw = spec_pow<false>(max0(dot3(N, halfway)), m->shininess);
                                    }
                                    fb = fb * (ldf3(m->ks) * pw);
                                }
                                const f3 e = ((ldf3(p.mats[p.meta[li].mati].emission) * (fl + fb)) * st.S()) * st.R();
                                if (wl < __builtin_inff()) st.setC(madd(e, cosy * wl, st.C()));
                            }
                        }
                    }
                    const float rnd1 = lcg_rand(seed), rnd2 = lcg_rand(seed);
                    dnew = diffuse_direction<false>(N, rnd1, rnd2);
                } else if (spec) {
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
                            dnew = madd(N, cosa / n - __builtin_sqrtf(disc), dn);
                            const float kk = 1.0f / (1.0f - prob);
                            st.setR((st.R() * mk(1.0f - F.x, 1.0f - F.y, 1.0f - F.z)) * kk);
                            inside = !inside;
                            side = -0.001f;
                        } else {
                            const float kk = 1.0f / prob;
                            st.setR((st.R() * F) * kk);
                        }
                    } else {
                        st.setS(st.S() * F);
                    }
                }
                if (lobe || spec) {
                    rD = normalize3(dnew);
                    rP = madd(N, side, hp);
                }
                if (type == 0) {
                    const float idiff = max0(dot3(rD, N));
                    st.setL(st.L() * (ldf3(m->kd) * idiff));
                    float pw = 1.0f;
                    if (!m->_pad) {
                        const f3 view = normalize3(eye - hp);
                        const f3 halfway = normalize3(view + rD);
                        const float ispec = max0(dot3(N, halfway));
                        pw = spec_pow<false>(ispec, m->shininess);
                    }
                    st.setB(st.B() * (ldf3(m->ks) * pw));
                } else if (type == 3) {
                    const f3 e = ((ldf3(m->emission) * (st.L() + st.B())) * st.S()) * st.R();
                    st.setC(madd(e * wb, inten, st.C()));        // (wb = 1: e's own bits)
                }
                after_lobe = lobe;
                Nprev = N;
            }
            acc = running_mean(acc, st.C(), s);
        }
        p.colors[i] = make_float4(acc.x, acc.y, acc.z, 0.0f);
        p.rnds[i] = seed;
        float4* rr = reinterpret_cast<float4*>(&p.rays[i]);        // the last segment's ray, as trace_ray leaves it
        rr[0] = make_float4(rP.x, rP.y, rP.z, 0.0f);
        rr[1] = make_float4(rD.x, rD.y, rD.z, 0.0f);
    }
}

template <int MODE, int BLOCK>
static hipError_t launch_nee_t(const RenderParams& p, const NeeTable& lt, int64_t npix, int cu_count, hipStream_t stream) {
    const size_t lds = traversal_lds_bytes(p, BLOCK);
    auto kern = k_nee<MODE, BLOCK>;
    static LdsMark mark;
    const hipError_t e = ensure_dynamic_lds((const void*)kern, mark, lds);
    if (e != hipSuccess) return e;
    const long long need = (npix + BLOCK - 1) / BLOCK;
    const int blocks = (int)std::min<long long>(need, (long long)cu_count * (2048 / BLOCK));
    if (p.stack_ovf && (long long)blocks * BLOCK > (long long)p.stack_ovf_lanes) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(BLOCK), lds, stream, p, lt, (long long)npix);
    return hipGetLastError();
}

hipError_t launch_nee(const RenderParams& p, const NeeTable& lt, int64_t npix, int cu_count, hipStream_t stream) {
    if (npix == 0) return hipSuccess;
    switch (p.node_mode) {
    case kNodesLds: return launch_nee_t<kNodesLds, 512>(p, lt, npix, cu_count, stream);
    case kNodesGlobal: return launch_nee_t<kNodesGlobal, 256>(p, lt, npix, cu_count, stream);
    case kNodesWide: return launch_nee_t<kNodesWide, 256>(p, lt, npix, cu_count, stream);
    case kNodesTreelet: return launch_nee_t<kNodesTreelet, 1024>(p, lt, npix, cu_count, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace ptamd
