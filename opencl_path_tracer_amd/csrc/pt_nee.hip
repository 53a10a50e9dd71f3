// pt_nee.hip -- next-event estimation with multiple importance sampling (pt_render_nee; the estimator is pinned in include/pt_api.h).
// One body, nee_frame<FAMILY, MODE, BLOCK, ENV, TILED>: one lane per local pixel, persistent blocks (like k_aovs), every sample of the pixel back
// to back, path state in registers.  Each segment is shade_hit (pt_device.hpp) with a light hook, NeeHook<FAMILY, MODE, ENV>: the MIS weight of
// an emitter hit after a lobe vertex and, at a lobe vertex, a light sample: one shadow ray whose search is cut just past the sampled point.
// The light sample's three numbers come from a counter-based hash (nee_rand, pt_internal.hpp) of (LCG state at the start of the sample,
// segment, dimension), never from the LCG, so the BSDF path draws exactly what pt_render draws and rnds / rays come out the same in every
// strategy.  FAMILY is a NeeFamily (pt_internal.hpp): each family is the one before it with one more feature compiled in, so a family names
// the features it has -- NeeHook derives them (smooth = FAMILY >= kNeeSmooth, ...).  What a feature adds sits under `if constexpr (feature)`
// here and under HOOK::feature in shade_hit, and what it carries in a *Slot that is empty without it, so an instance compiles to the code it
// was before the features it lacks existed.  The two forms' flags, then the features in the families' order:
//   ENV     an environment map (pt_set_environment): a miss adds the sky, and a lobe vertex samples either the sky or a triangle light,
//           chosen by one more hash value
//   TILED   the work is a list of 8x8 frame tiles (the rounds of pt_render_adaptive_ex): item j is pixel j & 63 of tile
//           frame_tile(p, j >> 6), so a wave is a tile as in k_render.  Three declarations sit outside the flag because both branches use
//           them afterwards (the loop counter j with the pixel i = j, lrow / x, and the pixel counter `rendered`, dead when untiled)
//   smooth  smooth shading from vertex normals (option smooth_normals)
//   textured  albedo textures (option textures, section 5.10)
//   glossy  material type 4 is the rough metal (option glossy, section 5.12)
//   coated  material type 5 is the coated diffuse (option coated, section 5.13); whether type 4 is live is a run-time field from here on
//           (kNeeFlagGlossy)
//   lens    each sample starts on the thin-lens ray (pt_set_lens, section 5.14); whether type 5 is live is a run-time field from here on
//           (kNeeFlagCoated)
//   frosted  material type 6 is the rough dielectric (option frosted, section 5.15); whether a lens is set is a run-time field (kNeeFlagLens)
//   lights  analytic point, spot and directional lights (pt_set_lights, section 5.16): a lobe vertex samples the set, the sky or a triangle
//           light; whether type 6 is live is a run-time field from here on (kNeeFlagFrosted)
//   medium  a homogeneous participating medium (pt_set_medium, section 5.17): a segment may end at a scatter vertex before its hit, and every
//           light sample outside a dielectric carries the transmittance of its shadow ray; whether a pickable light set is held is a
//           run-time field (kNeeFlagLights)
//   grid    the medium's extinction is sigma_t times a voxel density (pt_set_medium_density, section 5.20): the free flight and the transmittance
//           walk the grid (grid_walk, pt_device.hpp); everything else is medium's
//   interior  a type-2 or type-6 material may hold an interior (pt_set_material_interior, section 5.21): a segment inside such a dielectric takes
//           Beer-Lambert absorption and may end at a scatter vertex of the interior; whether a medium is held and whether its grid is live are
//           run-time fields (kNeeFlagMedium, kNeeFlagGrid)
//   ltree   the triangle-light branch of a light sample picks its triangle by walking the light hierarchy (option light_tree, section 5.22), and
//           an emitter hit's weight walks it towards the hit triangle from the previous lobe vertex, whose origin and cull normal the hook
//           keeps; whether an interior binding is live is a run-time field (kNeeFlagInterior)
//   area    sphere lights and suns with an angular size (pt_set_area_lights, section 5.24): a lobe vertex samples the area set, or whatever it
//           sampled before; a segment ends on the nearest sphere light in front of its hit, and a miss adds the suns whose disc holds it;
//           every shadow ray is also blocked by the spheres; whether the light hierarchy is walked is a run-time field (kNeeFlagLightTree)
// The kernels are k_nee<FAMILY, MODE, BLOCK, ENV, TILED> for the thirteen families the host can ask for.  In a family whose option is off the data
// is null (vn, tv.uv) or the flag clear.
#include "pt_device.hpp"
#include <type_traits>

namespace ptamd {

PT_DEV float nee_unit(unsigned h) { return (float)(h >> 8) * 5.9604644775390625e-08f; }   // [0, 1), 24 bits

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

// the environment a hook carries: nothing without one
template <bool ENV>
struct EnvSlot {};
template <>
struct EnvSlot<true> {
    EnvView v;
};

// what a hook carries for smooth shading (option smooth_normals): nothing without it
template <bool SMOOTH>
struct SmoothSlot {};
template <>
struct SmoothSlot<true> {
    const float4* vn = nullptr;    // packed vertex normals (k_pack_vertex_normals, pt_smooth.hip)
    int ti = 0;                    // the current vertex's packed triangle and whether its normal was flipped against the ray: the geometric
    bool flip = false;             // normal Ng is read back from the packet where it is needed, not carried across the light sample's traversal
    bool dead = false;             // a lobe vertex sampled a direction below the geometric surface: the path ends
};

// what a hook carries for albedo textures (option textures): nothing without it
template <bool TEX>
struct TexSlot {};
template <>
struct TexSlot<true> {
    TexView v;                     // packed uvs, texels, descriptors, bindings (texture_prepare, pt_host.cpp)
    f3 kd = mk(0.f, 0.f, 0.f);     // the current vertex's albedo kd' (its material's kd where nothing is bound)
};

// what a hook carries for the rough metal (option glossy): nothing without it
template <bool GLOSSY>
struct GlossySlot {};
template <>
struct GlossySlot<true> {
    float pb = 0.0f;               // p_b of the direction the previous lobe vertex sampled (these instances keep it instead of Nprev)
};

// what a hook carries for the coated diffuse (option coated): nothing without it
template <bool COAT>
struct CoatSlot {};
template <>
struct CoatSlot<true> {
    bool metal = false;            // option glossy: type 4 is the rough metal in this launch (else inert, as in the instances without it)
};

// what a frame carries for the thin lens (pt_set_lens): nothing without it
template <bool LENS>
struct LensSlot {};
template <>
struct LensSlot<true> {
    LensView v;                    // aperture, focus distance and the launch's f, Rh, Uh (lens_view, pt_internal.hpp)
    bool coat = true;              // option coated: type 5 is the coated diffuse in this launch (else inert, as in the instances without it)
};

// what a frame carries for the rough dielectric (option frosted): nothing without it
template <bool FROST>
struct FrostSlot {};
template <>
struct FrostSlot<true> {
    bool lens = true;              // a lens with aperture > 0 is set in this launch (else the pinhole ray, as in the instances without one)
};

// what a hook carries for the analytic lights (pt_set_lights): nothing without them
template <bool LIGHTS>
struct LightsSlot {};
template <>
struct LightsSlot<true> {
    LightsView v;                  // records, cdf, count and the launch's P_ana
    bool frost = true;             // option frosted with a type-6 material uploaded: type 6 is live in this launch (else inert, as in the instances without it)
};

// what a hook carries for the medium (pt_set_medium): nothing without it
template <bool MEDIUM>
struct MediumSlot {};
template <>
struct MediumSlot<true> {
    MediumView v;                  // sigma_t, albedo, g and the box: wave-uniform
    bool sc = false;               // the current segment ended at a scatter vertex (shade_hit then only takes the light sample)
    float T = 1.0f;                // the transmittance of the current light sample's shadow ray (light_sample_env to light_add)
};

// what a hook carries for the medium's density grid (pt_set_medium_density): nothing without it
template <bool GRID>
struct GridSlot {};
template <>
struct GridSlot<true> {
    GridView v;                    // the densities, the dimensions and the cell sizes: wave-uniform
};

// what a hook carries for the interiors of dielectrics (pt_set_material_interior): nothing without them
template <bool INTERIOR>
struct InteriorSlot {};
template <>
struct InteriorSlot<true> {
    InteriorView v;                // the table: two float4 per material on the device
    bool medium = true;            // a medium with sigma_t > 0 is held in this launch (else no free flight outside and T = 1, as in the instances without one)
    bool grid = true;              // ... and its density grid is live (else the homogeneous medium's flight and transmittance)
};

// what a hook carries for the light hierarchy (option light_tree): nothing without it
template <bool LTREE>
struct LightTreeSlot {};
template <>
struct LightTreeSlot<true> {
    LightTreeView v;               // nodes, tree-order lights, their inv_area, the packed triangles' tree-order indices
    f3 o = mk(0.f, 0.f, 0.f);      // the previous lobe vertex's shadow-ray origin and cull normal (zero at a scatter vertex of the medium): what
    f3 G = mk(0.f, 0.f, 0.f);      // the weight walk of an emitter hit on the next segment starts from
    bool interior = true;          // an interior binding is live in this launch (else no table is read, as in the instances without one)
};

// what a hook carries for the area lights (pt_set_area_lights): nothing without them
template <bool AREA>
struct AreaLightsSlot {};
template <>
struct AreaLightsSlot<true> {
    AreaLightsView v;              // records, cdf, counts and the launch's P_area: wave-uniform
    bool tree = true;              // option light_tree with a non-empty table: the hierarchy is walked (else the table's cdf, as in the instances without it)
};

// shade_hit's light hook: what k_nee adds to a segment
// and what a family compiles in: every feature up to its own (the names are what shade_hit asks a hook for, and what the comments here call them)
template <int FAMILY, int MODE, bool ENV>
struct NeeHook {
    static_assert(FAMILY >= kNeePlain && FAMILY <= kNeeAreaLights, "FAMILY is a NeeFamily");
    static constexpr bool active = true;
    static constexpr bool smooth = FAMILY >= kNeeSmooth, textured = FAMILY >= kNeeTex, glossy = FAMILY >= kNeeGlossy, coated = FAMILY >= kNeeCoated;
    static constexpr bool lens = FAMILY >= kNeeLens, frosted = FAMILY >= kNeeFrosted, lights = FAMILY >= kNeeLights, medium = FAMILY >= kNeeMedium;
    static constexpr bool grid = FAMILY >= kNeeGrid, interior = FAMILY >= kNeeInterior, ltree = FAMILY >= kNeeLightTree;
    static constexpr bool area = FAMILY >= kNeeAreaLights;
    NeeTable lt;
    const SceneView& sv;
    LaneStack<typename StackOf<MODE>::type> stk;
    WorkCount* wc;
    f3 eye;
    bool nee, mis;
    unsigned key = 0;              // the light samples' key: the LCG state at the start of the sample
    int k = 0;                     // the segment
    bool after_lobe = false;       // the previous vertex was a lobe vertex (its flipped normal: Nprev)
    f3 Nprev = mk(0.f, 0.f, 0.f);
    EnvSlot<ENV> env;
    SmoothSlot<smooth> sm;
    TexSlot<textured> tx;
    GlossySlot<glossy> gs;
    CoatSlot<coated> ct;
    LensSlot<lens> ln;
    FrostSlot<frosted> frs;
    LightsSlot<lights> lg;
    MediumSlot<medium> md;
    GridSlot<grid> gr;
    InteriorSlot<interior> in;
    LightTreeSlot<ltree> lts;
    AreaLightsSlot<area> ar;

    // area: the light hierarchy is walked (a run-time answer in the area-light instances only: the light-tree ones run only when it is)
    PT_DEV bool tree_live() const {
        if constexpr (area) return ar.tree;
        else return ltree;
    }
    // area: the nearest sphere light along (o, d) in front of t (its record index, t cut to its distance), or -1
    PT_DEV int sphere_hit(f3 o, f3 d, float* t) const {
        float ts;
        const int j = area_sphere_hit(ar.v, o, d, *t, -1, &ts);
        if (j >= 0) *t = ts;
        return j;
    }
    // area: a path that ends on segment kk on a light of radiance L whose sample density from the segment's origin is pl: L itself on segment 0
    // (the lamp seen by the camera, as the sky is), else the bracket of `miss` with the weight W_b
    PT_DEV void area_emit(PathRegs& st, f3 L, float pl, int kk) const {
        if (kk == 0) {
            st.setC(st.C() + L);
            return;
        }
        float wb = 1.0f;
        if (nee && after_lobe && pl > 0.0f) {
            if (mis) {
                const float rr = pl / gs.pb;       // pb = 0: rr = inf, weight 0
                wb = 1.0f / fmaf_(rr, rr, 1.0f);
            } else {
                wb = 0.0f;
            }
        }
        st.setC(madd(((L * (st.L() + st.B())) * st.S()) * st.R(), wb, st.C()));
    }
    // area: the segment (o, d) ends on sphere j
    PT_DEV void sphere_end(PathRegs& st, int j, f3 o, f3 d, int kk) const {
        const float4 q0 = ar.v.rec[3 * j], q1 = ar.v.rec[3 * j + 1];
        f3 c;
        float d2, R2;
        const float q = area_sphere_q(q0, o, &c, &d2, &R2);
        area_emit(st, mk(q1.x, q1.y, q1.z), (ar.v.p_area * q1.w) * (1.0f / (6.28318530717958647692f * q)), kk);
    }
    // area: the segment along d misses everything: every sun whose disc holds d adds its radiance, each with its own weight
    PT_DEV void sun_miss(PathRegs& st, f3 d, int kk) const {
        for (int j = ar.v.n_sphere; j < ar.v.n; ++j) {
            const float4 q0 = ar.v.rec[3 * j];
            if (!(dot3(d, mk(q0.x, q0.y, q0.z)) >= q0.w)) continue;
            const float4 q1 = ar.v.rec[3 * j + 1], q2 = ar.v.rec[3 * j + 2];
            area_emit(st, mk(q1.x, q1.y, q1.z), (ar.v.p_area * q1.w) * (1.0f / (6.28318530717958647692f * q2.x)), kk);
        }
    }
    // area: the light that u0 draws from the set's cdf, sampled from o with (u1, u2): false if rejected; else *w, *limit the search's cut (none
    // for a sun), *e its radiance, *pl = P_area P_light p_omega and *j its record (-1 for a sun: no sphere is skipped by the shadow test)
    PT_DEV bool area_direction(float u0, float u1, float u2, f3 o, f3* w, float* limit, f3* e, float* pl, int* j) const {
        const AreaLightsView& av = ar.v;
        int lo = 0, hi = av.n - 1;        // first light with cdf > u0
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (av.cdf[mid] > u0) hi = mid;
            else lo = mid + 1;
        }
        const float4 q0 = av.rec[lo * 3], q1 = av.rec[lo * 3 + 1];
        float pw;
        if (lo < av.n_sphere) {
            if (!area_sphere_sample(q0, o, u1, u2, w, &pw, limit)) return false;
            *j = lo;
        } else {
            const float q = av.rec[lo * 3 + 2].x;
            *w = area_cone(mk(q0.x, q0.y, q0.z), q, u1, u2);
            pw = 1.0f / (6.28318530717958647692f * q);
            *limit = __builtin_inff();
            *j = -1;
        }
        *e = mk(q1.x, q1.y, q1.z);
        *pl = (av.p_area * q1.w) * pw;
        return true;
    }

    // ltree: an interior binding is live (a run-time answer in the light-tree instances only: the interior ones run only when one is)
    PT_DEV bool interior_live() const {
        if constexpr (ltree) return lts.interior;
        else return interior;
    }
    // medium: the lane enters shade_hit at a scatter vertex
    PT_DEV bool scatters() const {
        if constexpr (medium) return md.sc;
        else return false;
    }
    // medium: the free flight of segment k along (rP, rD), whose closest hit is at t (+inf: a miss): the distance of the scatter vertex, or -1
    // when the segment reaches its end.  A segment with nothing inside the box draws no number (d >= 0 is never below L = 0)
    // grid: the same through the voxels: tau = -log1pf(-u) of the same number against the optical depth the walk accumulates
    PT_DEV float free_flight(f3 rP, f3 rD, float t) const {
        if constexpr (interior) {          // (the grid is a run-time answer here)
            if (in.grid) {
                const float tau = -log1pf(-nee_unit(nee_rand(key ^ 0x5bd1e995u, k, 0)));
                const GridWalk w = grid_walk<true>(md.v, gr.v, rP, rD, t, tau);
                return w.voxel >= 0 ? max0(w.s) : -1.0f;
            }
        } else if constexpr (grid) {
            const float tau = -log1pf(-nee_unit(nee_rand(key ^ 0x5bd1e995u, k, 0)));      // (a hash, not a draw: unused where the clip is empty)
            const GridWalk w = grid_walk<true>(md.v, gr.v, rP, rD, t, tau);
            return w.voxel >= 0 ? max0(w.s) : -1.0f;       // (s < 0 would take an accumulated depth a rounding past tau in a voxel at the origin)
        }
        float a;
        const float b = medium_clip(md.v, rP, rD, t, &a);
        const float L = max0(b - a);
        if (!(L > 0.0f)) return -1.0f;
        const float d = medium_flight(md.v.sigma_t, nee_unit(nee_rand(key ^ 0x5bd1e995u, k, 0)));
        return d < L ? a + d : -1.0f;
    }
    // medium: the scatter vertex's own factor; false: the albedo left nothing and the path ends
    PT_DEV bool scatter_albedo(PathRegs& st) const {
        const f3 fs = st.S() * mk(md.v.albedo[0], md.v.albedo[1], md.v.albedo[2]);
        st.setS(fs);
        return fs.x != 0.0f || fs.y != 0.0f || fs.z != 0.0f;
    }
    // medium: the scatter vertex at distance s ends: the next segment starts there, along a direction of the phase function; a lobe vertex
    // for what follows, with its p_b kept where the rough vertices keep theirs
    PT_DEV void scatter_direction(f3& rP, f3& rD, float s) {
        if constexpr (medium) {
            const float u1 = nee_unit(nee_rand(key ^ 0x5bd1e995u, k, 1)), u2 = nee_unit(nee_rand(key ^ 0x5bd1e995u, k, 2));
            rP = madd(rD, s, rP);
            rD = normalize3(medium_direction(md.v.g, rD, u1, u2, &gs.pb));
            after_lobe = true;
        }
    }
    // interior: a medium with sigma_t > 0 is held (a run-time answer in the interior instances only: the medium ones run only when one is)
    PT_DEV bool medium_live() const {
        if constexpr (interior) return in.medium;
        else return medium;
    }
    // interior: the free flight of segment k inside a dielectric whose hit is at t, through the interior q0 = {sigma_a.rgb, sigma_s}: the
    // distance of the scatter vertex, or -1 when the segment reaches its hit.  The exterior medium never draws while inside, so dimension 0
    // of its stream at this segment is free
    PT_DEV float interior_flight(const float4 q0, float t) const {
        if (!(q0.w > 0.0f)) return -1.0f;          // (no hash without scattering)
        return ptamd::interior_flight(q0.w, nee_unit(nee_rand(key ^ 0x5bd1e995u, k, 0)), t);
    }
    // interior: Beer-Lambert over the length l of the segment inside; false: the factor left nothing and the path ends
    PT_DEV bool interior_absorb(PathRegs& st, const float4 q0, float l) const {
        const f3 fs = st.S() * ptamd::interior_absorb(mk(q0.x, q0.y, q0.z), l);
        st.setS(fs);
        return fs.x != 0.0f || fs.y != 0.0f || fs.z != 0.0f;
    }
    // interior: scatter_direction with the vertex's own g and the after-lobe answer: a scatter vertex of an interior is no lobe vertex for what
    // follows (an emitter hit or a sky miss on the next segment has weight 1, as after a refraction)
    PT_DEV void scatter_direction(f3& rP, f3& rD, float s, float g, bool lobe) {
        if constexpr (medium) {
            const float u1 = nee_unit(nee_rand(key ^ 0x5bd1e995u, k, 1)), u2 = nee_unit(nee_rand(key ^ 0x5bd1e995u, k, 2));
            float pb;
            rP = madd(rD, s, rP);
            rD = normalize3(medium_direction(g, rD, u1, u2, &pb));
            if (lobe) gs.pb = pb;
            after_lobe = lobe;
        }
    }
    // lights: type 6 is live (option frosted; a run-time answer in the lights instances only: the frosted ones run only when it is)
    PT_DEV bool frost_live() const {
        if constexpr (lights) return lg.frost;
        else return frosted;
    }
    // lens: type 5 is live (option coated; a run-time answer in the lens instances only: the coated ones run only when it is)
    PT_DEV bool coat_live() const {
        if constexpr (lens) return ln.coat;
        else return coated;
    }
    // coated: type 4 is live (option glossy)
    PT_DEV bool metal_live() const {
        if constexpr (coated) return ct.metal;
        else return glossy;
    }
    // frosted: the reflection lobe's p_b of the unit direction w at the type-6 vertex with normal N reached along rD (ins: inside the
    // medium), and the factor_R its own update with w would give -- through frosted_pdf_weight, as the sampled direction's
    PT_DEV float frosted_light(const pt_material* __restrict__ m, f3 N, f3 rD, f3 w, bool ins, f3 fR, f3* fr) const {
        f3 Z, X;
        tangent_frame(N, &Z, &X);
        const float n = m->n;
        f3 g;
        const float pb = frosted_pdf_weight_of(m->shininess, ldf3(m->F0), ins ? 1.0f / n : n, to_local(-rD, X, Z, N), to_local(w, X, Z, N), &g);
        *fr = fR * g;
        return pb;
    }
    // coated: the mixture's p_b of the unit direction w at the type-5 vertex with normal N reached along rD, and the factor_S its own update
    // with w would give -- through coated_pdf_weight, as the sampled direction's (lobe_direction_rough)
    PT_DEV float coated_light(const pt_material* __restrict__ m, f3 N, f3 rD, f3 w, f3 fS, f3* fs) const {
        f3 Z, X;
        tangent_frame(N, &Z, &X);
        f3 g;
        const float pb = coated_pdf_weight_of(m->n, ldf3(m->F0), albedo(m), to_local(-rD, X, Z, N), to_local(w, X, Z, N), &g);
        *fs = fS * g;
        return pb;
    }
    // glossy: p_b of the unit direction w at the type-4 vertex with normal N reached along rD, and the factor_S its own update with w
    // would give -- through glossy_pdf, as the sampled direction's (lobe_direction_rough)
    PT_DEV float glossy_light(const pt_material* __restrict__ m, f3 N, f3 rD, f3 w, f3 fS, f3* fs) const {
        f3 Z, X;
        tangent_frame(N, &Z, &X);
        const float alpha = m->n;
        const f3 o = to_local(-rD, X, Z, N), wl = to_local(w, X, Z, N);
        f3 h;
        const float pb = glossy_pdf_of(alpha, o, wl, &h);
        *fs = fS * glossy_weight(alpha, ldf3(m->F0), o, h, wl);
        return pb;
    }
    // glossy: the sampled direction (before normalisation) of a lobe vertex of any kind (lobe_direction_rough).  A rough vertex also
    // multiplies a factor by g(w), keeps its p_b and may end the path: the metal (gl) factor_S, unless w.z > 0; coated: the coated vertex (ct_)
    // factor_S, unless w.z > 0 and p_b > 0; frosted: the frosted one (fr_) factor_R -- a reflection unless w.z > 0, while a refraction toggles
    // `inside`, leaves along -Ng (*side) and ends the path unless w.z < 0.  The lobe of a coated or frosted vertex is chosen by a hash value
    // keyed like the environment's selection, dimension 1 (a vertex has one type)
    template <bool SK, class ST>
    PT_DEV f3 lobe_vertex(ST& st, const pt_material* __restrict__ m, bool gl, bool ct_, bool fr_, f3 N, f3 rD, float rnd1, float rnd2, bool& inside,
                          float* side) {
        float alpha = 1.0f, u_sel = 0.0f, eta = 1.0f;
        f3 F0 = mk(0.f, 0.f, 0.f), kd = F0;
        if constexpr (frosted) {
            if (gl || ct_) alpha = m->n;   // (the device copy of a type-4 or type-5 material carries its roughness there: pt_upload_materials)
            if (fr_) {
                alpha = m->shininess;      // (that of a type-6 material here; its n is the index of refraction)
                eta = m->n;
                if (inside) eta = 1.0f / eta;
            }
            if (gl || ct_ || fr_) F0 = ldf3(m->F0);
            if (ct_) kd = albedo(m);
            if (ct_ || fr_) u_sel = nee_unit(nee_rand(~key, k, 1));
        } else {                           // (the same without fr_, in the order the instances without frosted were compiled from)
            if (gl || ct_) {
                alpha = m->n;
                F0 = ldf3(m->F0);
            }
            if (ct_) {
                kd = albedo(m);
                u_sel = nee_unit(nee_rand(~key, k, 1));
            }
        }
        GlossyOut go;
        CoatedOut co;
        FrostedOut fo;
        const f3 d = lobe_direction_rough<SK, coated>(N, rD, gl, ct_, fr_, alpha, F0, kd, eta, u_sel, rnd1, rnd2, &go, &co, &fo);
        if (gl) {
            st.setS(st.S() * (go.F * go.g1w));
            gs.pb = go.pb;
            if (!(go.wz > 0.0f)) sm.dead = true;
        }
        if constexpr (coated)
            if (ct_) {
                st.setS(st.S() * co.g);
                gs.pb = co.pb;
                if (!(co.wz > 0.0f && co.pb > 0.0f)) sm.dead = true;
            }
        if constexpr (frosted)
            if (fr_) {
                st.setR(st.R() * fo.g);
                gs.pb = fo.pb;
                if (!fo.refl) {
                    inside = !inside;
                    *side = -0.001f;
                }
                if (!(fo.refl ? fo.wz > 0.0f : fo.wz < 0.0f)) sm.dead = true;
            }
        return d;
    }
    // the albedo of the current type-0 vertex: the material's kd, or under textured what shading_attributes_at left
    PT_DEV f3 albedo(const pt_material* __restrict__ m) const {
        if constexpr (textured) return tx.kd;
        else return ldf3(m->kd);
    }
    // textured: shading_normal_at and the vertex's albedo from one evaluation of the weights (sm.vn == nullptr: smooth_normals is off).  kd is
    // read where something uses it: a type-0 vertex and the preview of iterations == 1
    PT_DEV f3 shading_attributes_at(const RenderParams& p, const float4* __restrict__ tris, int ti, f3 rD, f3 hp, f3 N, f3 Ng, int type,
                                    const pt_material* __restrict__ m) {
        sm.ti = ti;
        sm.flip = dot3(rD, N) > 0.0f;      // shade_hit's flip
        f3 kd = mk(0.f, 0.f, 0.f);
        if (type == 0 || p.iterations == 1) kd = ldf3(m->kd);
        int ttype = type;              // glossy: the instances also run with option textures off (a view with uv = null): no lookup then
        if constexpr (lens) {          // lens: as coated below where type 5 is live in the launch (option coated)
            const bool live = type == 5 && ln.coat;
            if (live) kd = ldf3(m->kd);
            ttype = live ? 0 : type;
        } else {
            if constexpr (coated) if (type == 5) kd = ldf3(m->kd);
            if constexpr (coated) ttype = type == 5 ? 0 : type;      // coated: the lookup runs for type 0 or 5
        }
        if constexpr (glossy) ttype = tx.v.uv ? ttype : -1;
        const f3 Ns = shading_normal_albedo(sm.vn, tx.v, tris, ti, rD, hp, N, Ng, ttype, (int)(m - p.mats), &kd);
        tx.kd = kd;
        return Ns;
    }
    // the normal the offsets use: N itself, or under smooth shading (where N is the shading normal) the geometric one
    PT_DEV f3 geo(f3 N) const {
        if constexpr (smooth) {
            const float4 c = sv.tris[sm.ti * 3 + 2];
            const f3 Ng = mk(c.y, c.z, c.w);
            return sm.flip ? -Ng : Ng;
        } else {
            return N;
        }
    }
    // smooth: the shading normal of the hit (N the record's normal, Ng flipped against the ray); keeps Ng for the rest of the vertex
    PT_DEV f3 shading_normal_at(const float4* __restrict__ tris, int ti, f3 rD, f3 hp, f3 N, f3 Ng) {
        sm.ti = ti;
        sm.flip = dot3(rD, N) > 0.0f;      // shade_hit's flip
        return shading_normal(sm.vn, tris, ti, rD, hp, N, Ng);
    }
    // smooth: a lobe vertex whose sampled direction (before normalisation) is not above the geometric surface ends the path; frosted: a refracted
    // one (through) that is not below it
    PT_DEV void leaves_surface(bool lobe, bool through, f3 dnew) {
        if (!lobe) return;
        const float g = dot3(dnew, geo(dnew));
        if (frosted && through ? g >= 0.0f : g <= 0.0f) sm.dead = true;
    }
    // smooth: the mirror / dielectric vertex of shade_hit evaluated with Ns; if the direction it picks is on the wrong geometric side
    // (a reflection not above, a refraction not below the surface), once more with Ng and the same LCG value, and that stands
    // (TWIN of the specular branch of shade_hit: the same expressions in the same order)
    template <class ST>
    PT_DEV void spec_vertex(f3 oldD, ST& st, int& seed, bool& inside, const pt_material* __restrict__ m, int type, f3 Ns, f3* dnew, float* side) {
        const f3 F0 = ldf3(m->F0);
        float n = 1.0f, rnd = 0.0f;
        if (type == 2) {
            n = m->n;
            if (inside) n = 1.0f / n;
            rnd = lcg_rand(seed);
        }
        const f3 Ng = geo(Ns);
        f3 F, d;
        float prob = 0.0f;
        bool refr = false;
        auto eval = [&](f3 N) {
            F = fresnel(F0, N, oldD);
            d = oldD - (N * dot3(N, oldD)) * 2.0f;
            refr = false;
            if (type == 2) {
                const float cosa = dot3(-oldD, N);
                const float disc = 1.0f - (fmaf_(-cosa, cosa, 1.0f) / n) / n;
                prob = ((F.x + F.y) + F.z) / 3.0f;
                refr = disc > 0.0f && rnd > prob;
                if (refr) {
                    const f3 dn = mk(oldD.x / n, oldD.y / n, oldD.z / n);
                    d = madd(N, cosa / n - sqrt_rn(disc), dn);
                }
            }
        };
        eval(Ns);
        const float g = dot3(d, Ng);
        if (refr ? g >= 0.0f : g <= 0.0f) eval(Ng);
        *dnew = d;
        if (type == 2) {
            if (refr) {
                const float k = 1.0f / (1.0f - prob);
                st.setR((st.R() * mk(1.0f - F.x, 1.0f - F.y, 1.0f - F.z)) * k);
                inside = !inside;
                *side = -0.001f;
            } else {
                const float k = 1.0f / prob;
                st.setR((st.R() * F) * k);
            }
        } else {
            st.setS(st.S() * F);
        }
    }

    // the weight of an emitter hit's emission (at distance t, cosine inten, along rD)
    PT_DEV float emitter_weight(int ti, float t, float inten, f3 rD) const {
        if (!nee || !after_lobe) return 1.0f;
        float pa;
        if constexpr (ltree) {             // the weight walk from the previous lobe vertex: the P the pick there had for this triangle
            pa = 0.0f;
            if (tree_live()) {
                const int s = lts.v.slot[ti];
                if (s >= 0 && inten > 0.0f) {
                    float P;
                    if (lt_walk<false>(lts.v, lts.o.x, lts.o.y, lts.o.z, lts.G.x, lts.G.y, lts.G.z, 0.0f, s, &P) >= 0) pa = P * lts.v.inv_area[s];
                }
            } else if constexpr (area) pa = lt.pdf_area[ti];
        } else pa = lt.pdf_area[ti];
        if constexpr (ENV) pa *= 1.0f - env.v.p_env;                 // the light table is chosen with probability 1 - P_env
        if constexpr (lights) pa *= 1.0f - lg.v.p_ana;               // ... and the sky or the table with probability 1 - P_ana
        if constexpr (area) pa *= 1.0f - ar.v.p_area;                // ... and any of them with probability 1 - P_area
        if (!(pa > 0.0f && inten > 0.0f)) return 1.0f;
        if (!mis) return 0.0f;
        float pb;
        if constexpr (glossy) pb = gs.pb;
        else pb = max0(dot3(Nprev, rD)) * kOneOverPi;
        const float pl = pa * (t * t) / inten;
        const float rr = pl / pb;          // pb = 0: rr = inf, weight 0
        return 1.0f / fmaf_(rr, rr, 1.0f);
    }

    // the light table's triangle that u0 draws (returned), *y the point on it that (u1, u2) draw and *Ny its normal
    PT_DEV int light_point(const RenderParams& p, float u0, float u1, float u2, f3* y, f3* Ny) const {
        int lo = 0, hi = lt.n - 1;        // first light with cdf > u0
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (lt.cdf[mid] > u0) hi = mid;
            else lo = mid + 1;
        }
        const int li = lt.tri[lo];
        const float4 a = p.tris[li * 3], b = p.tris[li * 3 + 1], cc = p.tris[li * 3 + 2];
        const f3 v1 = mk(a.x, a.y, a.z), v2 = mk(a.w, b.x, b.y), v3 = mk(b.z, b.w, cc.x);
        *Ny = mk(cc.y, cc.z, cc.w);
        const float su = __builtin_sqrtf(u1);
        *y = madd(v3 - v1, su * (1.0f - u2), madd(v2 - v1, u2 * su, v1));
        return li;
    }
    // ltree: the same with the triangle that the walk of the light hierarchy from o (cull normal lts.G) draws with u0; *pa = P x inv_area
    PT_DEV int tree_light_point(const RenderParams& p, f3 o, float u0, float u1, float u2, f3* y, f3* Ny, float* pa) const {
        float P;
        const int s = lt_walk<true>(lts.v, o.x, o.y, o.z, lts.G.x, lts.G.y, lts.G.z, u0, -1, &P);
        if (s < 0) return -1;
        *pa = P * lts.v.inv_area[s];
        const int li = lts.v.tri[s];
        const float4 a = p.tris[li * 3], b = p.tris[li * 3 + 1], cc = p.tris[li * 3 + 2];
        const f3 v1 = mk(a.x, a.y, a.z), v2 = mk(a.w, b.x, b.y), v3 = mk(b.z, b.w, cc.x);
        *Ny = mk(cc.y, cc.z, cc.w);
        const float su = __builtin_sqrtf(u1);
        *y = madd(v3 - v1, su * (1.0f - u2), madd(v2 - v1, u2 * su, v1));
        return li;
    }
    // that point seen from o: the unit direction to it (returned), *r2 and *r the squared distance and the distance, *cosy the emitter's cosine
    PT_DEV static f3 light_direction(f3 o, f3 y, f3 Ny, float* r2, float* r, float* cosy) {
        const f3 d = y - o;
        *r2 = dot3(d, d);
        *r = __builtin_sqrtf(*r2);
        const f3 w = mk(d.x / *r, d.y / *r, d.z / *r);
        *cosy = __builtin_fabsf(dot3(w, Ny));
        return w;
    }
    // what an unoccluded light sample adds: the bracket an emitter hit (or, ENV, a miss) along w on segment k + 1 would add, for the lobe
    // vertex hp (normal N, cosx = N.w, reached along rD; ins: inside a dielectric).  pl: the sample's p_l; g: the emitter's cosine (1 for the
    // sky); e: its radiance with ENV (the sky's texel or the triangle's emission, which light_sample_env has before the traversal).  Without ENV
    // e is not read: the emission of triangle li is loaded here, after the traversal, where those instances always read it.  lights: e comes
    // with the sample as with ENV; delta: an analytic light's sample, which no other strategy can find: its weight is p_b / p_l under MIS too
    // medium: type -1 is a scatter vertex of the medium (p_b the phase function's, N and cosx not read); the sample carries md.T
    PT_DEV void light_add(PathRegs& st, const RenderParams& p, const pt_material* __restrict__ m, int type, f3 N, f3 hp, f3 rD, bool ins, f3 w, float cosx,
                          float pl, float g, int li, f3 e, bool delta = false) const {
        float pb = cosx * kOneOverPi;
        if constexpr (medium) if (type < 0) pb = medium_hg(md.v.g, dot3(rD, w));
        f3 fs = st.S();
        if constexpr (glossy)
            if (type == 4) {
                pb = glossy_light(m, N, rD, w, fs, &fs);
                if (!(pb > 0.0f)) return;      // no density (or a half vector that cannot be normalised): the sample adds nothing
            }
        if constexpr (coated)
            if (type == 5) {
                pb = coated_light(m, N, rD, w, fs, &fs);
                if (!(pb > 0.0f)) return;
            }
        f3 fr = st.R();
        if constexpr (frosted)
            if (type == 6 && frost_live()) {
                pb = frosted_light(m, N, rD, w, ins, fr, &fr);
                if (!(pb > 0.0f)) return;
            }
        const float q = pb / pl;
        float wl = mis ? q / fmaf_(q, q, 1.0f) : q;
        if constexpr (lights) if (delta) wl = q;
        f3 fl = st.L(), fb = st.B();
        if (type == 0) {           // the factors the vertex's own update with w would give (shade_hit)
            fl = fl * (albedo(m) * cosx);
            float pw = 1.0f;
            if (!m->_pad) {
                const f3 view = normalize3(eye - hp);
                const f3 halfway = normalize3(view + w);
                pw = spec_pow<false>(max0(dot3(N, halfway)), m->shininess);
            }
            fb = fb * (ldf3(m->ks) * pw);
        }
        if constexpr (!ENV && !lights) e = ldf3(p.mats[p.meta[li].mati].emission);
        e = ((e * (fl + fb)) * fs) * fr;
        if constexpr (medium) e = e * md.T;
        if (wl < __builtin_inff()) st.setC(madd(e, g * wl, st.C()));
    }

    // a point y on a light, the bracket an emitter hit at y on segment k + 1 would add, for the lobe vertex hp (normal N)
    // (rD: the direction the vertex was reached along, read for a rough vertex; ins: the path is inside a dielectric, read for a type-6 one)
    PT_DEV void light_sample(PathRegs& st, const RenderParams& p, const pt_material* __restrict__ m, int type, f3 N, f3 hp, f3 rD, bool ins) {
        if (!nee || k + 1 >= p.iterations) return;
        if constexpr (ENV || lights) {
            light_sample_env(st, p, m, type, N, hp, rD, ins);
            return;
        }
        const float u0 = nee_unit(nee_rand(key, k, 0)), u1 = nee_unit(nee_rand(key, k, 1)), u2 = nee_unit(nee_rand(key, k, 2));
        f3 y, Ny;
        float r2, r, cosy;
        const int li = light_point(p, u0, u1, u2, &y, &Ny);
        const f3 o = madd(geo(N), 0.001f, hp);
        const f3 w = light_direction(o, y, Ny, &r2, &r, &cosy);
        const float cosx = dot3(N, w);
        const float pl = lt.pdf_area[li] * r2 / cosy;
        if (!(cosx > 0.0f && cosy > 0.0f && pl > 0.0f && pl < __builtin_inff())) return;
        if constexpr (smooth) if (!(dot3(geo(N), w) > 0.0f)) return;          // the sample must be above the geometric surface too
        if (shadow_hit<MODE>(sv, o, w, r * 1.0001f, stk, wc) != li) return;
        light_add(st, p, m, type, N, hp, rD, ins, w, cosx, pl, cosy, li, mk(0.f, 0.f, 0.f));
    }

    // lights: the analytic light that u0 draws from the set's cdf, seen from o: false if it adds nothing (a point light at o, or o outside its
    // cone); else *w the unit direction to it, *limit the search's cut (its distance r; none for a directional light), *e its intensity x
    // cone / d (d = r^2, or 1 for a directional light) and *pl = P_ana P_light.  One record load: the light picked
    PT_DEV bool analytic_direction(float u0, f3 o, f3* w, float* limit, f3* e, float* pl) const {
        const LightsView& lv = lg.v;
        int lo = 0, hi = lv.n - 1;        // first light with cdf > u0
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (lv.cdf[mid] > u0) hi = mid;
            else lo = mid + 1;
        }
        const float4 q0 = lv.rec[lo * 4], q1 = lv.rec[lo * 4 + 1], q2 = lv.rec[lo * 4 + 2], q3 = lv.rec[lo * 4 + 3];
        const f3 axis = mk(q1.x, q1.y, q1.z);
        float d = 1.0f;
        *limit = __builtin_inff();
        if (__float_as_int(q0.w) == PT_LIGHT_DIRECTIONAL) {
            *w = -axis;
        } else {
            const f3 dv = mk(q0.x, q0.y, q0.z) - o;
            d = dot3(dv, dv);
            if (!(d > 0.0f && d < __builtin_inff())) return false;
            const float r = __builtin_sqrtf(d);
            *w = mk(dv.x / r, dv.y / r, dv.z / r);
            *limit = r;
        }
        const float c = dot3(-*w, axis);
        float cone = 1.0f;                // full inside cos_inner (q1.w), nothing outside cos_outer (q2.w), smoothstep between
        if (!(c >= q1.w)) {
            if (c <= q2.w) return false;
            const float s = (c - q2.w) / (q1.w - q2.w);
            cone = (s * s) * (3.0f - 2.0f * s);
        }
        *e = mk(q2.x, q2.y, q2.z) * (cone / d);
        *pl = lv.p_ana * q3.x;
        return true;
    }
    // the sample is the sky's (u_sel, keyed with ~key, against P_env); never without ENV
    PT_DEV bool picks_sky() const {
        if constexpr (ENV) return nee_unit(nee_rand(~key, k, 0)) < env.v.p_env;
        else return false;
    }

    // ENV: the sky with probability P_env (u_sel, keyed with ~key), else a light of the table with its pdf times 1 - P_env.  Both
    // branches only produce the shadow ray and what it would add; the traversal and the weighting are shared, so a wave that holds
    // both kinds of sample runs one traversal
    // lights: before either, the analytic set with probability P_ana (keyed with ~key, dimension 2): a third branch of the same kind, and
    // the other two's p_l take the factor 1 - P_ana.  Without ENV there is no sky branch
    PT_DEV void light_sample_env(PathRegs& st, const RenderParams& p, const pt_material* __restrict__ m, int type, f3 N, f3 hp, f3 rD, bool ins) {
        const float u1 = nee_unit(nee_rand(key, k, 1)), u2 = nee_unit(nee_rand(key, k, 2));
        const bool mvx = medium && type < 0;       // medium: a scatter vertex of the medium: the origin is hp itself, and no cosine is tested
        f3 o = hp;
        if (!mvx) o = madd(geo(N), 0.001f, hp);
        if constexpr (ltree) {             // (kept for the emitter hit of the next segment, whichever branch this sample takes)
            lts.o = o;
            lts.G = mvx ? mk(0.f, 0.f, 0.f) : geo(N);
        }
        f3 w, e;
        float limit, pl, g;            // the search's cut, p_l, the emitter's cosine (1 for the sky and for an analytic light)
        int want;                      // what the shadow ray must return
        bool delta = false;            // lights: the sample is an analytic light's
        bool apick = false;            // area: the sample is an area light's, of sphere aj (-1: a sun)
        int aj = -1;
        if constexpr (area) apick = nee_unit(nee_rand(key ^ kAreaKey, k, 0)) < ar.v.p_area;
        if constexpr (lights) delta = !apick && nee_unit(nee_rand(~key, k, 2)) < lg.v.p_ana;
        if (area && apick) {
            if constexpr (area) {
                if (!area_direction(nee_unit(nee_rand(key, k, 0)), u1, u2, o, &w, &limit, &e, &pl, &aj)) return;
                g = 1.0f;
                want = -1;
            }
        } else if (lights && delta) {
            if constexpr (lights) {
                if (!analytic_direction(nee_unit(nee_rand(key, k, 0)), o, &w, &limit, &e, &pl)) return;
                if constexpr (area) pl *= 1.0f - ar.v.p_area;
                g = 1.0f;
                want = -1;
            }
        } else if (picks_sky()) {
            if constexpr (ENV) {
                const EnvView& ev = env.v;
                int lo = 0, hi = ev.h - 1;        // first row with cdf > u1, then first column of that row with cdf > u2
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (ev.row_cdf[mid] > u1) hi = mid;
                    else lo = mid + 1;
                }
                const int row = lo;
                const float rb = row ? ev.row_cdf[row - 1] : 0.0f;
                const float t1 = (u1 - rb) / (ev.row_cdf[row] - rb);
                const float* __restrict__ cc = ev.col_cdf + (size_t)row * ev.w;
                lo = 0;
                hi = ev.w - 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (cc[mid] > u2) hi = mid;
                    else lo = mid + 1;
                }
                const int col = lo;
                const float cb = col ? cc[col - 1] : 0.0f;
                const float t2 = (u2 - cb) / (cc[col] - cb);
                const float4 tx = ev.texels[(size_t)row * ev.w + col];
                const float c0 = cosf(3.14159265358979323846f * (float)row / (float)ev.h), c1 = cosf(3.14159265358979323846f * (float)(row + 1) / (float)ev.h);
                const float ct = c0 - t1 * (c0 - c1);
                const float sn = __builtin_sqrtf(max0(fmaf_(-ct, ct, 1.0f)));
                const float phi = fmaf_(6.28318530717958647692f, ((float)col + t2) / (float)ev.w, ev.yaw);
                w = mk(sn * cosf(phi), ct, sn * sinf(phi));
                e = mk(tx.x, tx.y, tx.z) * ev.scale;
                pl = ev.p_env * tx.w;
                if constexpr (lights) pl *= 1.0f - lg.v.p_ana;
                if constexpr (area) pl *= 1.0f - ar.v.p_area;
                g = 1.0f;
                limit = __builtin_inff();
                want = -1;
            }
        } else {
            if (lt.n <= 0) return;            // (P_env or P_ana is 1 then: not reached)
            f3 y, Ny;
            float r2, r, pa;
            if (ltree && tree_live()) {
                if constexpr (ltree) {
                    want = tree_light_point(p, o, nee_unit(nee_rand(key, k, 0)), u1, u2, &y, &Ny, &pa);
                    if (want < 0) return;     // (a tree that does not cover its table: not reached)
                }
            } else {
                want = light_point(p, nee_unit(nee_rand(key, k, 0)), u1, u2, &y, &Ny);
                pa = lt.pdf_area[want];
            }
            w = light_direction(o, y, Ny, &r2, &r, &g);
            if constexpr (ENV) pl = (pa * (1.0f - env.v.p_env)) * r2 / g;     // g = 0: inf or NaN, rejected below
            else pl = pa * r2 / g;
            if constexpr (lights) pl *= 1.0f - lg.v.p_ana;
            if constexpr (area) pl *= 1.0f - ar.v.p_area;
            e = ldf3(p.mats[p.meta[want].mati].emission);
            limit = r * 1.0001f;
        }
        const float cosx = dot3(N, w);
        if (!((mvx || cosx > 0.0f) && pl > 0.0f && pl < __builtin_inff())) return;
        if constexpr (smooth) if (!(mvx || dot3(geo(N), w) > 0.0f)) return;   // as in light_sample
        if constexpr (interior) {      // (the medium and its grid are run-time answers here)
            md.T = 1.0f;
            if (!ins && in.medium) {
                if (in.grid) {
                    const float depth = grid_walk<false>(md.v, gr.v, o, w, limit, __builtin_inff()).acc;
                    if (depth != 0.0f) md.T = expf(-depth);
                } else md.T = medium_transmittance(md.v, o, w, limit);
            }
        } else if constexpr (grid) {   // (for a vertex outside a dielectric)
            md.T = 1.0f;
            if (!ins) {
                const float depth = grid_walk<false>(md.v, gr.v, o, w, limit, __builtin_inff()).acc;
                if (depth != 0.0f) md.T = expf(-depth);
            }
        } else if constexpr (medium) md.T = ins ? 1.0f : medium_transmittance(md.v, o, w, limit);
        if constexpr (area) {          // one traversal, then the spheres: the nearest thing along w must be what was sampled
            const int got = shadow_hit<MODE>(sv, o, w, limit, stk, wc);
            float tb;
            if (area_sphere_hit(ar.v, o, w, limit, aj, &tb) >= 0) return;
            if (got != want) return;
        } else if (shadow_hit<MODE>(sv, o, w, limit, stk, wc) != want) return;
        if constexpr (lights) light_add(st, p, m, type, N, hp, rD, ins, w, cosx, pl, g, want, e, delta);
        else light_add(st, p, m, type, N, hp, rD, ins, w, cosx, pl, g, want, e);
    }

    // ENV: a miss on segment kk along rD (the path ends there)
    PT_DEV void miss(PathRegs& st, f3 rD, int kk) const {
        const EnvView& ev = env.v;
        int row, col;
        env_texel(ev.w, ev.h, ev.yaw, rD.x, rD.y, rD.z, &row, &col);
        const float4 tx = ev.texels[(size_t)row * ev.w + col];
        const f3 e = mk(tx.x, tx.y, tx.z) * ev.scale;
        if (kk == 0) {             // prog.cl:369: the sky itself
            st.setC(st.C() + e);
            return;
        }
        float wb = 1.0f;
        float pl = ev.p_env * tx.w;
        if constexpr (lights) pl *= 1.0f - lg.v.p_ana;
        if constexpr (area) pl *= 1.0f - ar.v.p_area;
        if (nee && after_lobe && pl > 0.0f) {
            if (mis) {
                float pb;
                if constexpr (glossy) pb = gs.pb;
                else pb = max0(dot3(Nprev, rD)) * kOneOverPi;
                const float rr = pl / pb;      // pb = 0: rr = inf, weight 0
                wb = 1.0f / fmaf_(rr, rr, 1.0f);
            } else {
                wb = 0.0f;
            }
        }
        st.setC(madd(((e * (st.L() + st.B())) * st.S()) * st.R(), wb, st.C()));      // prog.cl:371-373
    }

    // the vertex ends (rD: the new direction; rough: the lobe vertex kept its own p_b).  glossy: a cosine lobe's p_b of rD is what emitter_weight
    // / miss would compute from Nprev, which the other instances keep
    PT_DEV void end_vertex(bool lobe, bool rough, f3 N, f3 rD) {
        after_lobe = lobe;
        if constexpr (glossy) {
            if (lobe && !rough) gs.pb = max0(dot3(N, rD)) * kOneOverPi;
        } else {
            Nprev = N;
        }
    }
};

// One frame of the FAMILY's instance
template <int FAMILY, int MODE, int BLOCK, bool ENV, bool TILED>
PT_DEV void nee_frame(const RenderParams& p, const NeeTable& lt, const EnvSlot<ENV>& env, long long npix, const float4* vn, const TexView* tv, int flags,
                      const LensView* lens, const LightsView* lights, const MediumView* medium, const GridView* grid, const InteriorView* interior,
                      const LightTreeView* ltree, const AreaLightsView* area) {
    using Hook = NeeHook<FAMILY, MODE, ENV>;
    LaneStack<typename StackOf<MODE>::type> stk;
    SceneView sv;
    setup_traversal<MODE, BLOCK>(p, &sv, &stk);
    WorkCount wc;
    Hook hook{lt, sv, stk, &wc, ldf3(p.cam.eye), lt.n > 0 && lt.strategy != 0, lt.strategy == 2};
    if constexpr (Hook::smooth) hook.sm.vn = vn;
    if constexpr (Hook::textured) hook.tx.v = *tv;
    if constexpr (Hook::coated) hook.ct.metal = (flags & kNeeFlagGlossy) != 0;
    if constexpr (Hook::lens) {
        hook.ln.coat = (flags & kNeeFlagCoated) != 0;
        hook.ln.v = *lens;
    }
    if constexpr (Hook::frosted) hook.frs.lens = (flags & kNeeFlagLens) != 0;
    if constexpr (ENV) {
        hook.env = env;
        hook.nee = lt.strategy != 0;       // the sky is a light (the host launches this instance only for a map with a distribution)
    }
    if constexpr (Hook::lights) {
        hook.lg.v = *lights;
        hook.lg.frost = (flags & kNeeFlagFrosted) != 0;
        // the set is a light (the host launches the lights instances only for a set with a pickable light; the medium ones say whether one is held)
        if (!Hook::medium || (flags & kNeeFlagLights) != 0) hook.nee = lt.strategy != 0;
    }
    if constexpr (Hook::medium) hook.md.v = *medium;
    if constexpr (Hook::grid) hook.gr.v = *grid;
    if constexpr (Hook::interior) {
        hook.in.v = *interior;
        hook.in.medium = (flags & kNeeFlagMedium) != 0;
        hook.in.grid = (flags & kNeeFlagGrid) != 0;
    }
    if constexpr (Hook::ltree) {
        hook.lts.v = *ltree;
        hook.lts.interior = (flags & kNeeFlagInterior) != 0;
    }
    if constexpr (Hook::area) {
        hook.ar.v = *area;
        hook.ar.tree = (flags & kNeeFlagLightTree) != 0;
        if (area->p_area > 0.0f) hook.nee = lt.strategy != 0;      // the set is a light
    }
    const int camX = (int)p.cam.XM;
    unsigned rendered = 0;                     // TILED: pixels this lane rendered (statistic "samples", as k_render counts them)
    if constexpr (TILED) npix = (long long)p.n_tiles * 64;      // work items: 64 per listed tile
    for (long long j = (long long)blockIdx.x * BLOCK + threadIdx.x; j < npix; j += (long long)gridDim.x * BLOCK) {
        long long i = j;                       // the local pixel
        int lrow, x;
        if constexpr (TILED) {                 // BLOCK is whole waves and so is the stride: a wave is one tile, j >> 6 wave-uniform
            const int tile = frame_tile(p, (int)(j >> 6));
            const int tiles_x = (p.width + 7) >> 3;
            const int ty = tile / tiles_x, lane = (int)(j & 63);
            x = (tile - ty * tiles_x) * 8 + (lane & 7);
            lrow = ty * 8 + (lane >> 3);
            if (x >= p.width || lrow >= p.local_rows) continue;       // (a ragged tile's lanes outside the frame)
            i = (long long)lrow * p.width + x;
            ++rendered;
        } else {
            lrow = (int)(i / p.width);
            x = (int)(i % p.width);
        }
        const int gid = global_row(p, lrow) * p.width + x;
        const float pix_x = (float)(gid % camX), pix_y = (float)(gid / camX);      // prog.cl:84-85
        int seed = p.rnds[i];
        f3 acc = mk(0.f, 0.f, 0.f);
        float m2 = 0.0f;                           // option "moments": the running second moment (colors[].w)
        if (p.first_sample != 0) {                 // prog.cl:312-314: sample 0 starts from black
            const float4 c = p.colors[i];
            acc = mk(c.x, c.y, c.z);
            if (p.moments) m2 = c.w;
        }
        f3 rP = mk(0.f, 0.f, 0.f), rD = mk(0.f, 0.f, 1.f);
        for (int s = p.first_sample; s < p.first_sample + p.nsamples; ++s) {
            hook.key = (unsigned)seed;
            hook.after_lobe = false;
            if constexpr (Hook::smooth) hook.sm.dead = false;
            PathRegs st;
            st.reset();
            bool inside = false;
            {
                const float rnd1 = lcg_rand(seed), rnd2 = lcg_rand(seed);
                if constexpr (Hook::frosted) {
                    if (hook.frs.lens) lens_get_ray_xy(pix_x, pix_y, p.cam, hook.ln.v, rnd1, rnd2, hook.key, &rP, &rD);
                    else camera_get_ray_xy(pix_x, pix_y, p.cam, rnd1, rnd2, &rP, &rD);
                } else if constexpr (Hook::lens) lens_get_ray_xy(pix_x, pix_y, p.cam, hook.ln.v, rnd1, rnd2, hook.key, &rP, &rD);
                else camera_get_ray_xy(pix_x, pix_y, p.cam, rnd1, rnd2, &rP, &rD);
            }
            for (int k = 0; k < p.iterations; ++k) {
                float t;
                const int ti = closest_hit<MODE, false>(sv, rP, rD, stk, &t, &wc);
                if constexpr (Hook::interior) {
                    // medium's body below with the interior in the `else` of `if (!inside)`: the segment runs inside the dielectric whose
                    // boundary it hits at ti, the surface the path will leave through, and the interior is the one bound to that material.
                    // Only lanes that are inside look the table up.  Its scatter vertex takes no light sample (a shadow ray from inside ends
                    // on the object's own boundary), so the lane skips shade_hit
                    // area: a sphere light nearer than the hit ends the segment in its place (sj: which), before either free flight looks at
                    // the segment's length; a segment that reaches it ends the path there
                    hook.k = k;
                    int sj = -1;
                    if constexpr (Hook::area) {
                        if (ti < 0) t = __builtin_inff();
                        sj = hook.sphere_hit(rP, rD, &t);
                    }
                    float ts = -1.0f;              // the distance of this segment's scatter vertex; < 0: it reaches its hit or misses
                    float ig = 0.0f;               // the g of the interior it scatters in
                    bool isc = false, dead = false;
                    if (!inside) {
                        if (hook.medium_live()) ts = hook.free_flight(rP, rD, ti < 0 && sj < 0 ? __builtin_inff() : t);
                    } else if (ti >= 0 && hook.interior_live()) {
                        const float4* __restrict__ rec = hook.in.v.rec + 2 * (size_t)p.meta[ti].mati;
                        const float4 q1 = rec[1];
                        if (q1.y != 0.0f) {
                            const float4 q0 = rec[0];
                            ts = hook.interior_flight(q0, t);
                            isc = ts >= 0.0f;
                            dead = !hook.interior_absorb(st, q0, isc ? ts : t);
                            ig = q1.x;
                        }
                    }
                    if (dead) break;
                    const bool sc = ts >= 0.0f && !isc;
                    hook.md.sc = sc;
                    if (ti < 0 && sj < 0 && !sc) {
                        if constexpr (Hook::area) hook.sun_miss(st, rD, k);
                        if constexpr (ENV) hook.miss(st, rD, k);
                        break;
                    }
                    if constexpr (Hook::area)
                        if (sj >= 0 && !sc && !isc) {
                            hook.sphere_end(st, sj, rP, rD, k);
                            break;
                        }
                    if (sc && !hook.scatter_albedo(st)) break;
                    if (!isc) shade_hit<false>(rP, rD, st, seed, inside, p, p.tris, p.meta, ti, sc ? ts : t, &hook);
                    if (sc) hook.scatter_direction(rP, rD, ts);
                    if (isc) hook.scatter_direction(rP, rD, ts, ig, false);
                } else if constexpr (Hook::medium) {
                    // the free flight of the segment; then the scatter vertex: its factor here, its light sample in shade_hit's one call of
                    // light_sample (the lane does nothing else there), its new direction after it
                    hook.k = k;
                    float ts = -1.0f;              // the distance of this segment's scatter vertex; < 0: it reaches its hit or misses
                    if (!inside) ts = hook.free_flight(rP, rD, ti < 0 ? __builtin_inff() : t);
                    const bool sc = ts >= 0.0f;
                    hook.md.sc = sc;
                    if (ti < 0 && !sc) {
                        if constexpr (ENV) hook.miss(st, rD, k);
                        break;
                    }
                    if (sc && !hook.scatter_albedo(st)) break;
                    shade_hit<false>(rP, rD, st, seed, inside, p, p.tris, p.meta, ti, sc ? ts : t, &hook);
                    if (sc) hook.scatter_direction(rP, rD, ts);
                } else {
                    if (ti < 0) {                  // prog.cl:367-376: black without an environment
                        if constexpr (ENV) hook.miss(st, rD, k);
                        break;
                    }
                    hook.k = k;
                    shade_hit<false>(rP, rD, st, seed, inside, p, p.tris, p.meta, ti, t, &hook);
                }
                if constexpr (Hook::smooth) if (hook.sm.dead) break;
            }
            acc = running_mean(acc, st.C(), s);
            if (p.moments) m2 = running_moment(m2, st.C(), s);
        }
        p.colors[i] = make_float4(acc.x, acc.y, acc.z, m2);
        p.rnds[i] = seed;
        float4* rr = reinterpret_cast<float4*>(&p.rays[i]);        // the last segment's ray, as trace_ray leaves it
        rr[0] = make_float4(rP.x, rP.y, rP.z, 0.0f);
        rr[1] = make_float4(rD.x, rD.y, rD.z, 0.0f);
    }
    if constexpr (TILED) {
        if (p.stats) {
            const unsigned long long n = wave_sum((unsigned long long)rendered) * (unsigned long long)p.nsamples;
            if ((threadIdx.x & 63) == 0 && n) stat_add(p, 1, n);
        }
    }
}

// An argument that an instance has only where ON: elsewhere the parameter is an empty NeeNone, which nothing reads
struct NeeNone {};
template <bool ON, class T>
using NeeArg = std::conditional_t<ON, T, NeeNone>;
// The kernel: k_nee<FAMILY, MODE, BLOCK, ENV, TILED>, twelve families times four forms (ENV, TILED) times the node modes' shapes.  Each view is an
// argument of its own from the family that compiles its feature in, the flags (NeeFlag) from the first family in which one is a run-time answer
template <int FAMILY, int MODE, int BLOCK, bool ENV, bool TILED, class F = NeeHook<FAMILY, MODE, ENV>>
__global__ void __launch_bounds__(BLOCK)
    k_nee(RenderParams p, NeeTable lt, NeeArg<ENV, EnvView> env, NeeArg<F::smooth, const float4*> vn, NeeArg<F::textured, TexView> tv, NeeArg<F::coated, int> flags,
          NeeArg<F::lens, LensView> lv, NeeArg<F::lights, LightsView> lg, NeeArg<F::medium, MediumView> mv, NeeArg<F::grid, GridView> gv,
          NeeArg<F::interior, InteriorView> iv, NeeArg<F::ltree, LightTreeView> tr, NeeArg<F::area, AreaLightsView> av,
          NeeArg<!TILED, long long> npix) {
    EnvSlot<ENV> slot;
    long long n = 0;
    const float4* vnp = nullptr;
    const TexView* tvp = nullptr;
    int fl = 0;
    const LensView* lvp = nullptr;
    const LightsView* lgp = nullptr;
    const MediumView* mvp = nullptr;
    const GridView* gvp = nullptr;
    const InteriorView* ivp = nullptr;
    const LightTreeView* trp = nullptr;
    const AreaLightsView* avp = nullptr;
    if constexpr (ENV) slot.v = env;
    if constexpr (!TILED) n = npix;
    if constexpr (F::smooth) vnp = vn;
    if constexpr (F::textured) tvp = &tv;
    if constexpr (F::coated) fl = flags;
    if constexpr (F::lens) lvp = &lv;
    if constexpr (F::lights) lgp = &lg;
    if constexpr (F::medium) mvp = &mv;
    if constexpr (F::grid) gvp = &gv;
    if constexpr (F::interior) ivp = &iv;
    if constexpr (F::ltree) trp = &tr;
    if constexpr (F::area) avp = &av;
    nee_frame<FAMILY, MODE, BLOCK, ENV, TILED>(p, lt, slot, n, vnp, tvp, fl, lvp, lgp, mvp, gvp, ivp, trp, avp);
}

// launch_lanes with 512-thread workgroups for a treelet: in the mode's 1,024-thread shape the 128-VGPR cap of sixteen waves per workgroup makes
// the instances with the most live state spill (first the smooth family's ENV TILED one: 134 VGPRs, no scratch at 512; the stacks and the
// staged treelet are sized for the workgroup at launch, as for every shape)
template <class PICK, class... A>
static hipError_t launch_lanes_wide(PICK pick, const RenderParams& p, int64_t n, int cu_count, hipStream_t stream, A... args) {
    if (n == 0) return hipSuccess;
    switch (p.node_mode) {
    case kNodesLds: return launch_lanes_t<kNodesLds, 512>(pick, p, n, cu_count, stream, args...);
    case kNodesGlobal: return launch_lanes_t<kNodesGlobal, 256>(pick, p, n, cu_count, stream, args...);
    case kNodesWide: return launch_lanes_t<kNodesWide, 256>(pick, p, n, cu_count, stream, args...);
    case kNodesTreelet: return launch_lanes_t<kNodesTreelet, 512>(pick, p, n, cu_count, stream, args...);
    }
    return hipErrorInvalidValue;
}

// which forms of a family take launch_lanes_wide: bit f is form f = ENV + 2 TILED.  The smooth family's ENV TILED instance; the textured
// family's ENV one too (3 VGPRs more than the smooth one's, which sits at the 128-VGPR cap); every instance from the glossy family on
enum : int { kWidePlain = 1, kWideEnv = 2, kWideTiles = 4, kWideEnvTiles = 8, kWideAll = 15 };
constexpr int kNeeWide[kNeeAreaLights + 1] = {0,        kWideEnvTiles, kWideEnv | kWideEnvTiles, kWideAll, kWideAll, kWideAll, kWideAll,
                                              kWideAll, kWideAll,      kWideAll,                 kWideAll, kWideAll, kWideAll};

// launch_lanes_t keys its static LdsMark on the type of `pick`, so every kernel arrives through a type of its own
template <int FAMILY, bool ENV, bool TILED>
struct NeePick {
    template <class S>
    auto operator()(S s) const { return k_nee<FAMILY, s.mode, s.block, ENV, TILED>; }
};
// the launch's value for an argument the instance has, NeeNone for one it has not
template <bool ON, class T>
static NeeArg<ON, T> nee_arg(const T& v) {
    if constexpr (ON) return v;
    else return NeeNone{};
}
template <int FAMILY, bool ENV, bool TILED>
static hipError_t launch_nee_form(const RenderParams& p, const NeeTable& lt, const NeeLaunch& nl, int64_t n, int cu_count, hipStream_t stream) {
    using F = NeeHook<FAMILY, 0, ENV>;
    const NeePick<FAMILY, ENV, TILED> pick;
    const auto launch = [&](auto... a) {
        if constexpr ((kNeeWide[FAMILY] >> (ENV + 2 * TILED) & 1) != 0) return launch_lanes_wide(pick, p, n, cu_count, stream, lt, a...);
        else return launch_lanes(pick, p, n, cu_count, stream, lt, a...);
    };
    return launch(nee_arg<ENV>(nl.env ? *nl.env : EnvView{}), nee_arg<F::smooth>(nl.vn), nee_arg<F::textured>(nl.tv), nee_arg<F::coated>(nl.flags),
                  nee_arg<F::lens>(nl.lens), nee_arg<F::lights>(nl.lights), nee_arg<F::medium>(nl.medium), nee_arg<F::grid>(nl.grid),
                  nee_arg<F::interior>(nl.interior), nee_arg<F::ltree>(nl.ltree), nee_arg<F::area>(nl.area), nee_arg<!TILED>((long long)n));
}
// the four kernels of one family: n is the pixels of the frame or, tiled, 64 work items per listed tile
template <int FAMILY>
static hipError_t launch_nee_family(const RenderParams& p, const NeeTable& lt, const NeeLaunch& nl, int64_t npix, int cu_count, hipStream_t stream) {
    const int64_t n = nl.tiled ? (int64_t)p.n_tiles * 64 : npix;
    if (nl.tiled) return nl.env ? launch_nee_form<FAMILY, true, true>(p, lt, nl, n, cu_count, stream) : launch_nee_form<FAMILY, false, true>(p, lt, nl, n, cu_count, stream);
    return nl.env ? launch_nee_form<FAMILY, true, false>(p, lt, nl, n, cu_count, stream) : launch_nee_form<FAMILY, false, false>(p, lt, nl, n, cu_count, stream);
}

// The families from kNeeMedium on are each compiled in a translation unit of their own: pt_nee_medium.hip, pt_nee_grid.hip, pt_nee_interior.hip
// pt_nee_lighttree.hip and pt_nee_arealights.hip include this file with PT_NEE_TU set to their family (PT_NEE_FAMILY_*, pt_internal.hpp) and get launch_nee_tu<PT_NEE_TU> only.  Compiled next to the
// other families, the medium instances cost 48 of them two instructions in their uv fetch (the compiler no longer derives for a helper they
// share that its triangle index is never negative; profiles/medium/README.md); each later family likewise, so that the ones before it compile
// as they did before it existed
template <int FAMILY>
hipError_t launch_nee_tu(const RenderParams& p, const NeeTable& lt, const NeeLaunch& nl, int64_t npix, int cu_count, hipStream_t stream);
#if defined(PT_NEE_TU)
template <int FAMILY>
hipError_t launch_nee_tu(const RenderParams& p, const NeeTable& lt, const NeeLaunch& nl, int64_t npix, int cu_count, hipStream_t stream) {
    return launch_nee_family<FAMILY>(p, lt, nl, npix, cu_count, stream);
}
template hipError_t launch_nee_tu<PT_NEE_TU>(const RenderParams&, const NeeTable&, const NeeLaunch&, int64_t, int, hipStream_t);
#else
hipError_t launch_nee(const RenderParams& p, const NeeTable& lt, const NeeLaunch& nl, int64_t npix, int cu_count, hipStream_t stream) {
    t_lanes_block = 0;
    hipError_t e = hipErrorInvalidValue;
    switch (nl.family) {
    case kNeePlain: e = launch_nee_family<kNeePlain>(p, lt, nl, npix, cu_count, stream); break;
    case kNeeSmooth: e = launch_nee_family<kNeeSmooth>(p, lt, nl, npix, cu_count, stream); break;
    case kNeeTex: e = launch_nee_family<kNeeTex>(p, lt, nl, npix, cu_count, stream); break;
    case kNeeGlossy: e = launch_nee_family<kNeeGlossy>(p, lt, nl, npix, cu_count, stream); break;
    case kNeeCoated: e = launch_nee_family<kNeeCoated>(p, lt, nl, npix, cu_count, stream); break;
    case kNeeLens: e = launch_nee_family<kNeeLens>(p, lt, nl, npix, cu_count, stream); break;
    case kNeeFrosted: e = launch_nee_family<kNeeFrosted>(p, lt, nl, npix, cu_count, stream); break;
    case kNeeLights: e = launch_nee_family<kNeeLights>(p, lt, nl, npix, cu_count, stream); break;
    case kNeeMedium: e = launch_nee_tu<kNeeMedium>(p, lt, nl, npix, cu_count, stream); break;
    case kNeeGrid: e = launch_nee_tu<kNeeGrid>(p, lt, nl, npix, cu_count, stream); break;
    case kNeeInterior: e = launch_nee_tu<kNeeInterior>(p, lt, nl, npix, cu_count, stream); break;
    case kNeeLightTree: e = launch_nee_tu<kNeeLightTree>(p, lt, nl, npix, cu_count, stream); break;
    case kNeeAreaLights: e = launch_nee_tu<kNeeAreaLights>(p, lt, nl, npix, cu_count, stream); break;
    }
    if (nl.block) *nl.block = t_lanes_block;      // (what launch_lanes_t launched with, in this translation unit or in the family's own)
    return e;
}
#endif

#if defined(PT_NEE_TU) && PT_NEE_TU == PT_NEE_FAMILY_LIGHTTREE      // (pt_debug_light_tree_eval's kernel sits with the instances that make the same walks)
// in: 7 floats per item {o, G, u0} and the tree-order light whose probability the weight walk returns (-1: none); out: 4 words per item {the
// tree-order light the pick draws, bits(its P), bits(the weight walk's P of the target), 0}: the two walks as the instances above call them
__global__ void __launch_bounds__(256) k_debug_light_tree(LightTreeView v, const float* __restrict__ in, const int32_t* __restrict__ target, long long n,
                                                          int32_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* q = in + i * 7;
    float P, Pw;
    const int s = lt_walk<true>(v, q[0], q[1], q[2], q[3], q[4], q[5], q[6], -1, &P);
    lt_walk<false>(v, q[0], q[1], q[2], q[3], q[4], q[5], 0.0f, target[i], &Pw);
    int32_t* o = out + i * 4;
    o[0] = s;
    o[1] = __float_as_int(P);
    o[2] = __float_as_int(Pw);
    o[3] = 0;
}
hipError_t launch_debug_light_tree(const LightTreeView& v, const float* in, const int32_t* target, int64_t n, int32_t* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_debug_light_tree, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, v, in, target, (long long)n, out);
    return hipGetLastError();
}
#endif

#if defined(PT_NEE_TU) && PT_NEE_TU == PT_NEE_FAMILY_AREALIGHTS     // (pt_debug_area_light_eval's kernel sits with the instances that call the same functions)
// sample items: in 6 floats {o, bits(record), u1, u2}, out 6 words {w, p_omega, t_s (+inf for a sun), accept}; hit items: in 7 floats {o, d, t_max},
// out 4 words {nearest sphere or -1, bits(t), the suns' mask low, high}.  Every record index is tested against the count before its loads
__global__ void __launch_bounds__(256) k_debug_area_light(AreaLightsView v, const float* __restrict__ s_in, long long n_s, int32_t* __restrict__ s_out,
                                                          const float* __restrict__ h_in, long long n_h, int32_t* __restrict__ h_out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_s) {
        const float* q = s_in + i * 6;
        const int j = __float_as_int(q[3]);
        f3 w = mk(0.f, 0.f, 0.f);
        float pw = 0.0f, ts = __builtin_inff();
        bool ok = false;
        if ((unsigned)j < (unsigned)v.n) {
            const float4 q0 = v.rec[3 * j];
            if (j < v.n_sphere) {
                ok = area_sphere_sample(q0, mk(q[0], q[1], q[2]), q[4], q[5], &w, &pw, &ts);
            } else {
                const float qq = v.rec[3 * j + 2].x;
                w = area_cone(mk(q0.x, q0.y, q0.z), qq, q[4], q[5]);
                pw = 1.0f / (6.28318530717958647692f * qq);
                ok = true;
            }
        }
        int32_t* o = s_out + i * 6;
        o[0] = __float_as_int(w.x);
        o[1] = __float_as_int(w.y);
        o[2] = __float_as_int(w.z);
        o[3] = __float_as_int(pw);
        o[4] = __float_as_int(ts);
        o[5] = ok ? 1 : 0;
    }
    if (i < n_h) {
        const float* q = h_in + i * 7;
        float t;
        const f3 d = mk(q[3], q[4], q[5]);
        const int j = area_sphere_hit(v, mk(q[0], q[1], q[2]), d, q[6], -1, &t);
        const unsigned long long m = area_sun_mask(v, d);
        int32_t* o = h_out + i * 4;
        o[0] = j;
        o[1] = __float_as_int(t);
        o[2] = (int32_t)(unsigned)(m & 0xffffffffull);
        o[3] = (int32_t)(unsigned)(m >> 32);
    }
}
hipError_t launch_debug_area_light(const AreaLightsView& v, const float* s_in, int64_t n_s, int32_t* s_out, const float* h_in, int64_t n_h, int32_t* h_out,
                                   hipStream_t stream) {
    const int64_t n = n_s > n_h ? n_s : n_h;
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_debug_area_light, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, v, s_in, (long long)n_s, s_out, h_in, (long long)n_h, h_out);
    return hipGetLastError();
}
#endif

}  // namespace ptamd
