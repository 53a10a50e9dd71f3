// pt_lighttree.cpp -- the light hierarchy of pt_render_nee (option light_tree; include/pt_api.h pins the tree, the walk and the probabilities;
// DESIGN.md section 5.22): the host builder over the light table, the device copies, pt_debug_light_tree and pt_debug_light_tree_eval.  The walk
// itself is lt_walk (pt_internal.hpp), one __host__ __device__ body that this file runs on the host and pt_nee.hip (k_nee*_lighttree and
// k_debug_light_tree, compiled in pt_nee_lighttree.hip) on the device.
#include "pt_context.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace ptamd {

namespace {
struct TreeBuilder {
    const std::vector<float>& vtx;          // 9 floats per light, table order
    const std::vector<double>& cen;         // 3 per light: the centroid
    const std::vector<double>& phi;         // per light
    std::vector<int32_t> idx;               // the lights, permuted into tree order as the build goes
    std::vector<float> nodes;               // 8 per node
    int32_t depth = 0;

    static int ceil_log2(int64_t m) {
        int k = 0;
        while (((int64_t)1 << k) < m) ++k;
        return k;
    }
    // the subtree of idx[b, e) at depth d: its node index; *lo, *hi the box of its lights' vertices, *sum its phi in double
    int32_t build(int32_t b, int32_t e, int d, float* lo, float* hi, double* sum) {
        const int32_t node = (int32_t)(nodes.size() / 8);
        nodes.resize(nodes.size() + 8, 0.0f);
        const int32_t n = e - b;
        int32_t right = 0;
        if (n == 1) {
            const float* v = vtx.data() + 9 * (size_t)idx[(size_t)b];
            for (int a = 0; a < 3; ++a) {
                lo[a] = std::min(v[a], std::min(v[3 + a], v[6 + a]));
                hi[a] = std::max(v[a], std::max(v[3 + a], v[6 + a]));
            }
            *sum = phi[(size_t)idx[(size_t)b]];
            depth = std::max(depth, d);
        } else {
            double clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int32_t i = b; i < e; ++i)
                for (int a = 0; a < 3; ++a) {
                    const double c = cen[3 * (size_t)idx[(size_t)i] + a];
                    clo[a] = std::min(clo[a], c);
                    chi[a] = std::max(chi[a], c);
                }
            int axis = 0;
            for (int a = 1; a < 3; ++a)
                if (chi[a] - clo[a] >= chi[axis] - clo[axis]) axis = a;      // (a tie goes to the later axis)
            auto key = [&](int32_t l) { return cen[3 * (size_t)l + axis]; };
            int32_t m = b;
            if (d + 1 + ceil_log2(n - 1) <= kLightTreeMaxDepth) {
                const double mid = 0.5 * (clo[axis] + chi[axis]);
                m = (int32_t)(std::stable_partition(idx.begin() + b, idx.begin() + e, [&](int32_t l) { return key(l) < mid; }) - idx.begin());
            }
            if (m == b || m == e) {            // equal counts
                std::stable_sort(idx.begin() + b, idx.begin() + e, [&](int32_t x, int32_t y) { return key(x) < key(y); });
                m = b + (n + 1) / 2;
            }
            float llo[3], lhi[3], rlo[3], rhi[3];
            double ls, rs;
            build(b, m, d + 1, llo, lhi, &ls);
            right = build(m, e, d + 1, rlo, rhi, &rs);
            for (int a = 0; a < 3; ++a) {
                lo[a] = std::min(llo[a], rlo[a]);
                hi[a] = std::max(lhi[a], rhi[a]);
            }
            *sum = ls + rs;
        }
        float* q = nodes.data() + 8 * (size_t)node;
        double r2 = 0.0;
        for (int a = 0; a < 3; ++a) {
            q[a] = (float)(0.5 * ((double)lo[a] + (double)hi[a]));
            const double h = std::max((double)hi[a] - (double)q[a], (double)q[a] - (double)lo[a]);
            r2 += h * h;
        }
        const double r = std::sqrt(r2);
        float rf = (float)r;
        if ((double)rf < r) rf = std::nextafterf(rf, INFINITY);
        q[3] = std::nextafterf(rf, INFINITY);
        q[4] = (float)*sum;
        std::memcpy(q + 5, &b, 4);
        std::memcpy(q + 6, &n, 4);
        std::memcpy(q + 7, &right, 4);
        return node;
    }
};
}  // namespace

int light_tree_ready(pt_context* ctx) {
    int rc = light_table_ready(ctx);
    if (rc != PT_OK) return rc;
    if (ctx->lt_valid) return PT_OK;
    const size_t nl = ctx->nee_tri.size();
    std::vector<float> vtx(nl * 9);
    std::vector<double> cen(nl * 3);
    for (size_t j = 0; j < nl; ++j) {
        const pt_triangle& t = ctx->tris[(size_t)ctx->orig[(size_t)ctx->nee_tri[j]]];
        for (int a = 0; a < 3; ++a) {
            vtx[9 * j + a] = t.r1.s[a];
            vtx[9 * j + 3 + a] = t.r2.s[a];
            vtx[9 * j + 6 + a] = t.r3.s[a];
            cen[3 * j + a] = (((double)t.r1.s[a] + (double)t.r2.s[a]) + (double)t.r3.s[a]) / 3.0;
        }
    }
    TreeBuilder tb{vtx, cen, ctx->nee_phi};
    tb.idx.resize(nl);
    for (size_t j = 0; j < nl; ++j) tb.idx[j] = (int32_t)j;
    if (nl) {
        tb.nodes.reserve(16 * nl);
        float lo[3], hi[3];
        double sum;
        tb.build(0, (int32_t)nl, 0, lo, hi, &sum);
    }
    ctx->lt_nodes.swap(tb.nodes);
    ctx->lt_depth = tb.depth;
    ctx->lt_tri.resize(nl);
    ctx->lt_inv_area.resize(nl);
    ctx->lt_slot.assign(std::max<size_t>(ctx->orig.size(), 1), -1);
    for (size_t s = 0; s < nl; ++s) {
        const size_t j = (size_t)tb.idx[s];
        ctx->lt_tri[s] = ctx->nee_tri[j];
        ctx->lt_inv_area[s] = (float)(1.0 / ctx->nee_area[j]);
        ctx->lt_slot[(size_t)ctx->nee_tri[j]] = (int32_t)s;
    }
    ctx->lt_valid = true;
    ctx->lt_uploaded = false;
    return PT_OK;
}

LightTreeView light_tree_host(const pt_context* ctx) {
    return LightTreeView{reinterpret_cast<const float4*>(ctx->lt_nodes.data()), ctx->lt_tri.data(), ctx->lt_inv_area.data(), ctx->lt_slot.data(),
                         (int32_t)(ctx->lt_nodes.size() / 8), (int32_t)ctx->lt_tri.size()};
}

int light_tree_prepare(pt_context* ctx, LightTreeView* v) {
    int rc = light_tree_ready(ctx);
    if (rc != PT_OK) return rc;
    PT_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->lt_uploaded) {
        PT_HIP(ctx, hipStreamSynchronize(ctx->stream));      // a frame in flight may still read the previous tree
        if ((rc = upload_vec(ctx, &ctx->d_lt_nodes, ctx->lt_nodes.data(), sizeof(float) * ctx->lt_nodes.size())) != PT_OK) return rc;
        if ((rc = upload_vec(ctx, &ctx->d_lt_tri, ctx->lt_tri.data(), sizeof(int32_t) * ctx->lt_tri.size())) != PT_OK) return rc;
        if ((rc = upload_vec(ctx, &ctx->d_lt_inv_area, ctx->lt_inv_area.data(), sizeof(float) * ctx->lt_inv_area.size())) != PT_OK) return rc;
        if ((rc = upload_vec(ctx, &ctx->d_lt_slot, ctx->lt_slot.data(), sizeof(int32_t) * ctx->lt_slot.size())) != PT_OK) return rc;
        ctx->lt_uploaded = true;
    }
    *v = LightTreeView{ctx->d_lt_nodes, ctx->d_lt_tri, ctx->d_lt_inv_area, ctx->d_lt_slot, (int32_t)(ctx->lt_nodes.size() / 8), (int32_t)ctx->lt_tri.size()};
    return PT_OK;
}

}  // namespace ptamd

using namespace ptamd;

extern "C" {

int pt_debug_light_tree(pt_context* ctx, float* nodes, int64_t node_cap, int64_t* n_nodes, int32_t* orig_tri, int64_t light_cap, int64_t* n_lights) {
    if (!ctx) return PT_EINVAL;
    if (!n_nodes || !n_lights || node_cap < 0 || light_cap < 0) return fail(ctx, PT_EINVAL, "pt_debug_light_tree: n_nodes or n_lights is NULL, or a cap < 0");
    const int rc = light_tree_ready(ctx);
    if (rc != PT_OK) return rc;
    *n_nodes = (int64_t)(ctx->lt_nodes.size() / 8);
    *n_lights = (int64_t)ctx->lt_tri.size();
    if (nodes) std::memcpy(nodes, ctx->lt_nodes.data(), sizeof(float) * 8 * (size_t)std::min(node_cap, *n_nodes));
    if (orig_tri)
        for (size_t s = 0; s < (size_t)std::min(light_cap, *n_lights); ++s) orig_tri[s] = ctx->orig[(size_t)ctx->lt_tri[s]];
    return PT_OK;
}

int pt_debug_light_tree_eval(pt_context* ctx, const float* points, const float* normals, const float* u0, const int32_t* tris, int64_t n,
                             pt_light_tree_eval* out, int32_t on_device) {
    if (!ctx) return PT_EINVAL;
    if (n < 0 || (n > 0 && (!points || !normals || !u0 || !tris || !out)))
        return fail(ctx, PT_EINVAL, "pt_debug_light_tree_eval: n < 0, or an array is NULL");
    if (on_device) PT_NEED_DEVICE(ctx);
    int rc = light_tree_ready(ctx);
    if (rc != PT_OK) return rc;
    for (int64_t i = 0; i < n; ++i)
        if (!(u0[i] >= 0.0f && u0[i] < 1.0f)) return fail(ctx, PT_EINVAL, "pt_debug_light_tree_eval: every u0 must lie in [0, 1)");
    if (n == 0) return PT_OK;
    std::vector<int32_t> packed(ctx->tris.size(), -1), target((size_t)n, -1);
    for (size_t k = 0; k < ctx->orig.size(); ++k) packed[(size_t)ctx->orig[k]] = (int32_t)k;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t k = tris[i] >= 0 && (size_t)tris[i] < packed.size() ? packed[(size_t)tris[i]] : -1;
        target[(size_t)i] = k >= 0 ? ctx->lt_slot[(size_t)k] : -1;
    }
    std::vector<int32_t> raw((size_t)n * 4);       // {picked slot, bits(P), bits(P of the target), 0} per item
    if (on_device) {
        LightTreeView v;
        if ((rc = light_tree_prepare(ctx, &v)) != PT_OK) return rc;
        std::vector<float> in((size_t)n * 7);
        for (int64_t i = 0; i < n; ++i) {
            std::memcpy(in.data() + 7 * i, points + 3 * i, 12);
            std::memcpy(in.data() + 7 * i + 3, normals + 3 * i, 12);
            in[(size_t)(7 * i + 6)] = u0[i];
        }
        DeviceBuf d_in, d_target, d_out;
        PT_HIP(ctx, d_in.alloc(sizeof(float) * in.size()));
        PT_HIP(ctx, d_target.alloc(sizeof(int32_t) * target.size()));
        PT_HIP(ctx, d_out.alloc(sizeof(int32_t) * raw.size()));
        PT_HIP(ctx, hipMemcpy(d_in.p, in.data(), sizeof(float) * in.size(), hipMemcpyHostToDevice));
        PT_HIP(ctx, hipMemcpy(d_target.p, target.data(), sizeof(int32_t) * target.size(), hipMemcpyHostToDevice));
        PT_HIP(ctx, launch_debug_light_tree(v, (const float*)d_in.p, (const int32_t*)d_target.p, n, (int32_t*)d_out.p, ctx->stream));
        PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        PT_HIP(ctx, hipMemcpy(raw.data(), d_out.p, sizeof(int32_t) * raw.size(), hipMemcpyDeviceToHost));
    } else {
        const LightTreeView v = light_tree_host(ctx);
        for (int64_t i = 0; i < n; ++i) {
            const float *o = points + 3 * i, *g = normals + 3 * i;
            float P, Pw;
            raw[(size_t)(4 * i)] = lt_walk<true>(v, o[0], o[1], o[2], g[0], g[1], g[2], u0[i], -1, &P);
            lt_walk<false>(v, o[0], o[1], o[2], g[0], g[1], g[2], 0.0f, target[(size_t)i], &Pw);
            std::memcpy(&raw[(size_t)(4 * i + 1)], &P, 4);
            std::memcpy(&raw[(size_t)(4 * i + 2)], &Pw, 4);
        }
    }
    for (int64_t i = 0; i < n; ++i) {
        const int32_t s = raw[(size_t)(4 * i)];
        out[i].slot = s;
        out[i].tri = s >= 0 && (size_t)s < ctx->lt_tri.size() ? ctx->orig[(size_t)ctx->lt_tri[(size_t)s]] : -1;
        std::memcpy(&out[i].p, &raw[(size_t)(4 * i + 1)], 4);
        std::memcpy(&out[i].p_weight, &raw[(size_t)(4 * i + 2)], 4);
    }
    return PT_OK;
}

}  // extern "C"
