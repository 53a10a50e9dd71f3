"""Float64 model of the light hierarchy of Scene.render_nee (option light_tree; include/pt_api.h pins the tree, the walk and the
probabilities): the walk over the nodes Scene.debug_light_tree() returns, and tests/nee_ref.py's estimator with it (TreeModel: the
setting `tree` of tests/path_ref.py's PathModel puts the pick and the weight walk in place of the table's cdf and P_sel).  Also
the invariants a tree must satisfy, as the host test states them."""
import numpy as np

import nee_ref as R

NEAR = 1e-5


class Tree:
    """nodes, orig_tri: Scene.debug_light_tree().  Slots are tree-order light indices; orig_tri[slot] is the add-order triangle."""

    def __init__(self, nodes, orig_tri):
        self.c = np.asarray(nodes["c"], dtype=np.float64).reshape(-1, 3)
        self.r = np.asarray(nodes["r"], dtype=np.float64)
        self.phi = np.asarray(nodes["phi"], dtype=np.float64)
        self.first = np.asarray(nodes["first"], dtype=np.int64)
        self.count = np.asarray(nodes["count"], dtype=np.int64)
        self.right = np.asarray(nodes["right"], dtype=np.int64)
        self.tri = np.asarray(orig_tri, dtype=np.int64)
        self.slot_of = {int(t): s for s, t in enumerate(self.tri)}

    def importance(self, i, o, G):
        d = self.c[i] - o
        if float(G @ d) < -self.r[i]:
            return 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.float64(self.phi[i]) / max(float(d @ d), self.r[i] * self.r[i]))

    def p_left(self, node, o, G):
        L, Rr = node + 1, int(self.right[node])
        iL, iR = self.importance(L, o, G), self.importance(Rr, o, G)
        s = iL + iR
        if not (s > 0.0 and np.isfinite(s)):
            iL, iR = float(self.phi[L]), float(self.phi[Rr])
            s = iL + iR
        p = iL / s if s > 0 else float("nan")
        return p if 0.0 <= p <= 1.0 else 0.5

    def pick(self, o, G, u0):
        """(slot, P, near): the leaf u0 draws, its probability, and whether u0 came within a relative NEAR of a branch boundary on the
        way (the boundaries are kept in u0's own units: the interval [lo, lo + w) of u0 values that reach the node)"""
        o, G = np.asarray(o, dtype=np.float64), np.asarray(G, dtype=np.float64)
        if len(self.count) == 0:
            return -1, 0.0, False
        node, P, lo, w, near = 0, 1.0, 0.0, 1.0, False
        while self.count[node] > 1:
            pL = self.p_left(node, o, G)
            b = lo + pL * w
            near |= abs(u0 - b) <= NEAR * max(u0, b)
            if u0 < b:
                P, w, node = P * pL, pL * w, node + 1
            else:
                P, lo, w, node = P * (1.0 - pL), b, (1.0 - pL) * w, int(self.right[node])
        return int(self.first[node]), P, bool(near)

    def weight(self, o, G, slot):
        """the probability of the leaf `slot` from (o, G); 0 for slot < 0"""
        if slot is None or slot < 0 or len(self.count) == 0:
            return 0.0
        o, G = np.asarray(o, dtype=np.float64), np.asarray(G, dtype=np.float64)
        node, P = 0, 1.0
        while self.count[node] > 1:
            pL = self.p_left(node, o, G)
            L = node + 1
            if slot < self.first[L] + self.count[L]:
                P, node = P * pL, L
            else:
                P, node = P * (1.0 - pL), int(self.right[node])
        assert self.first[node] == slot
        return P

    def probabilities(self, o, G):
        """P of every slot from (o, G), float64"""
        return np.array([self.weight(o, G, s) for s in range(len(self.tri))])

    def depth(self):
        best, stack = 0, [(0, 0)] if len(self.count) else []
        while stack:
            node, d = stack.pop()
            if self.count[node] <= 1:
                best = max(best, d)
            else:
                stack += [(node + 1, d + 1), (int(self.right[node]), d + 1)]
        return best


def check_invariants(nodes, orig_tri, verts, phi_of):
    """The invariants of a tree over the lights `orig_tri` (tree order): verts (ntris, 3, 3) float32 the scene's triangles in add
    order, phi_of {add-order triangle: its weight in float64}.  Returns the depth."""
    t = Tree(nodes, orig_tri)
    n = len(t.tri)
    if n == 0:
        assert len(t.count) == 0
        return 0
    assert len(t.count) == 2 * n - 1
    assert sorted(t.tri.tolist()) == sorted(phi_of.keys())            # every light once
    v = np.asarray(verts, dtype=np.float64)
    seen = np.zeros(n, dtype=int)

    def visit(node, first, count, d):
        """(box lo, box hi, phi in double, depth) of the subtree; checks range, sphere and phi"""
        assert t.first[node] == first and t.count[node] == count, node
        if count == 1:
            seen[first] += 1
            tv = v[t.tri[first]]
            lo, hi, ph, dd = tv.min(axis=0), tv.max(axis=0), float(phi_of[int(t.tri[first])]), d
        else:
            L, Rr = node + 1, int(t.right[node])
            cl = int(t.count[L])
            assert 1 <= cl < count and t.first[L] == first and t.first[Rr] == first + cl and t.count[Rr] == count - cl     # a partition
            llo, lhi, lp, ld = visit(L, first, cl, d + 1)
            rlo, rhi, rp, rd = visit(Rr, first + cl, count - cl, d + 1)
            lo, hi, ph, dd = np.minimum(llo, rlo), np.maximum(lhi, rhi), lp + rp, max(ld, rd)
        corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
        assert (np.linalg.norm(corners - t.c[node], axis=1) <= t.r[node]).all(), node      # the sphere contains the box (of both children too)
        assert np.float32(ph) == np.float32(t.phi[node]), node                             # the rounded double sum
        return lo, hi, ph, dd

    depth = visit(0, 0, n, 0)[3]
    assert (seen == 1).all()
    assert depth <= 64
    return depth


class TreeModel(R.Model):
    """nee_ref.Model with the light hierarchy: `tree` a Tree over the same lights; the pick in place of the cdf search and P inv_area
    in place of P_sel / area, from the origin and the cull normal of the lobe vertex."""

    def __init__(self, *args, tree=None, **kw):
        super().__init__(*args, **kw)
        self.tree = tree
        assert sorted(tree.tri.tolist()) == sorted(int(x) for x in self.lights)


def variance_ratio_prediction(tree, table_phi, points, normals, verts, emission_sum):
    """A rough CPU prediction of what the tree buys: for each (point, normal) the second moment of the unoccluded one-sample direct-light
    estimate E_sum G / p over the lights, under the table's probabilities (phi shares) and under the tree's; returns mean(second
    moment with the table) / mean(with the tree).  Geometry term from the triangle centroids; lights below the horizon contribute 0."""
    v = np.asarray(verts, dtype=np.float64)
    share = np.asarray(table_phi, dtype=np.float64)
    share = share / share.sum()
    m_tab, m_tree = [], []
    for o, N in zip(np.asarray(points, dtype=np.float64), np.asarray(normals, dtype=np.float64)):
        pt = tree.probabilities(o, N)
        f = np.zeros(len(tree.tri))
        for s, tr in enumerate(tree.tri):
            tv = v[tr]
            cen = tv.mean(axis=0)
            nrm = np.cross(tv[1] - tv[0], tv[2] - tv[0])
            area = 0.5 * np.linalg.norm(nrm)
            nrm = nrm / (2.0 * area)
            d = cen - o
            r2 = float(d @ d)
            w = d / np.sqrt(r2)
            f[s] = emission_sum[int(tr)] * max(0.0, float(N @ w)) * abs(float(nrm @ w)) * area / r2
        with np.errstate(divide="ignore", invalid="ignore"):
            m_tab.append(np.where(f > 0, f * f / share, 0.0).sum())
            m_tree.append(np.where((f > 0) & (pt > 0), f * f / pt, 0.0).sum())
    return float(np.mean(m_tab) / np.mean(m_tree))
