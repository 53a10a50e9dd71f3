"""Float64 replay of the lit guide buffers (option aov_lights; include/pt_api.h pins them): the guides of pt_render_aovs /
PT_AOV_SHADED that see the sphere lights and the suns of the area set.

The chain is tests/aov_shaded_ref.trace_chain itself, by import: LitModel stands in front of the chain's model and answers its
`intersect` by the rule of the lit guides -- after every closest hit the nearest sphere light in front of the triangle
(arealights_ref.sphere_hit) ends the chain, and a miss takes the suns whose disc holds the direction (arealights_ref.sun_mask).  A chain
that ends on a light is handed to trace_chain as a hit on one more triangle, of a material of its own whose kd is the light's radiance
(so the chain's tint multiplies it) and whose normal is the sphere's; replay() then writes what the rule pins for it (material
-2 - j; for a sun normal 0, and no depth on the primary ray).  With smooth = textured = False the chain is pt_render_aovs's.

Every decision of the rule reports its relative margin, the distance from its other outcome: `outside` (|d^2 - R^2| / R^2: the
origin against the sphere's surface), `disc` (the discriminant's sign), `t_tri` (t_s against the triangle's distance), `nearest`
(the two nearest candidate spheres) and `sun` (|dot(D, axis) - cos a| / (1 - cos a))."""
import numpy as np

import aov_shaded_ref as A
import arealights_ref as AR

DECISIONS = ("outside", "disc", "t_tri", "nearest", "sun")


class _Mats:
    """the model's material records, and one more: the light a chain ended on"""

    def __init__(self, mats):
        self.mats, self.light = mats, None

    def __len__(self):
        return len(self.mats) + 1

    def __getitem__(self, i):
        return self.light if i == len(self.mats) else self.mats[i]


class LitModel:
    """the chain's model (a texture_ref.TextureModel) with the area set of Scene.debug_area_lights() in front of its intersect"""

    def __init__(self, model, area):
        self.model = model
        rec = np.asarray(area["records"], dtype=np.float64)
        ns = int(area["n_sphere"])
        self.spheres = [(rec[j, :3], rec[j, 3]) for j in range(ns)]
        self.suns = [(rec[j, :3], rec[j, 3]) for j in range(ns, len(rec))]
        self.L = rec[:, 4:7]
        nt = len(model.mat_of)
        self.slot = nt                                           # the triangle a light stands in for
        self.mats = _Mats(model.mats)
        self.mat_of = np.append(np.asarray(model.mat_of, dtype=np.int64), len(model.mats))
        self.n = np.vstack([model.n, np.zeros((1, 3))])
        self.v = np.concatenate([model.v, np.zeros((1, 3, 3))])
        self.vn = np.concatenate([model.vn, np.zeros((1, 3, 3))])
        self.has = np.append(model.has, False)
        self.begin()

    def __getattr__(self, name):                                 # camera_ray, _spec, albedo_at, ...: the model's own
        return getattr(self.model, name)

    def begin(self):
        """a new chain: no light met, every margin open"""
        self.calls, self.end = 0, None                           # end = (kind, record, met by the primary ray)
        self.margin = {k: np.inf for k in DECISIONS}

    def _note(self, key, value):
        self.margin[key] = min(self.margin[key], float(value))

    def _light(self, kind, j, normal, radiance):
        self.end = (kind, j, self.calls == 1)
        self.n[self.slot] = normal
        self.mats.light = {"type": 3, "kd": np.asarray(radiance, dtype=np.float64), "emission": np.zeros(3), "F0": np.zeros(3), "n": 1.0}

    def intersect(self, P, D, limit=np.inf):
        self.calls += 1
        ti, t, tie = self.model.intersect(P, D, limit)
        t_tri = t if ti >= 0 else np.inf
        j, ts, marg = AR.sphere_hit(self.spheres, P, D, t_tri, np.float64)
        cand = []                                                # the spheres the ray meets from outside, in front of its origin
        for k, (m, sp) in enumerate(zip(marg, self.spheres)):
            self._note("outside", m[0])
            hit, tk, _ = AR.sphere_hit([sp], P, D, np.inf, np.float64)
            c = np.asarray(sp[0]) - P
            if float(c @ c) > sp[1] * sp[1] and float(c @ D) > 0:
                self._note("disc", m[1])
            if hit == 0:
                cand.append(float(tk))
        cand.sort()
        if cand and np.isfinite(t_tri):
            self._note("t_tri", min(abs(c - t_tri) / max(c, t_tri) for c in cand))
        if len(cand) > 1:
            self._note("nearest", (cand[1] - cand[0]) / cand[1])
        if j >= 0:
            Cj = self.spheres[j][0]
            nrm = P + D * ts - Cj
            self._light("sphere", j, nrm / np.linalg.norm(nrm), self.L[j])
            return self.slot, float(ts), tie
        if ti >= 0:
            return ti, t, tie
        mask, smarg = AR.sun_mask(self.suns, D, np.float64)
        for m, (_, ca) in zip(smarg, self.suns):
            self._note("sun", m / (1.0 - ca))
        if mask:
            on = [s for s in range(len(self.suns)) if mask >> s & 1]
            total = np.zeros(3)
            for s in on:                                         # ascending record order
                total = total + self.L[len(self.spheres) + s]
            self._light("sun", len(self.spheres) + on[0], -D, total)
            return self.slot, 1.0, tie                           # (the distance is not read: replay() drops it)
        return -1, t, tie


def trace_chain(lit, gid, rnd1, rnd2, specular_depth, smooth=True, textured=True):
    """aov_shaded_ref.trace_chain through a LitModel, with what the rule pins for a chain that ends on a light; adds `margin`, the
    chain's smallest relative margin per decision, and `light`, the record it ended on or -1"""
    lit.begin()
    c = A.trace_chain(lit, gid, rnd1, rnd2, specular_depth, smooth, textured)
    c["margin"], c["light"] = dict(lit.margin), -1
    if lit.end is not None:
        kind, j, primary = lit.end
        c["light"], c["mat"] = j, -2 - j
        if kind == "sun":
            c["normal"] = np.zeros(3)
            if primary:
                c["t"] = None                                    # a sun's disc is a miss
    return c


def replay(lit, pixel_ids, offsets, specular_depth, smooth=True, textured=True):
    """The lit guides of those global pixel ids in float64, summed and normalised as aov_shaded_ref.replay does: albedo_rgbm (n, 4),
    normal_depth (n, 4), near (n,), margin {decision: (n,)}, light (n,): the record the first sub-pixel's chain ended on, or -1, and
    ends (n,): how many of the pixel's chains ended on a light."""
    n = len(pixel_ids)
    alb, nd = np.zeros((n, 4)), np.zeros((n, 4))
    near = np.zeros(n, bool)
    margin = {k: np.full(n, np.inf) for k in DECISIONS}
    light = np.full(n, -1, dtype=np.int64)
    ends = np.zeros(n, dtype=np.int64)
    for p, gid in enumerate(pixel_ids):
        sa, sn, st, hits, mat0 = np.zeros(3), np.zeros(3), 0.0, 0, -1
        for k, (r1, r2) in enumerate(offsets):
            c = trace_chain(lit, int(gid), r1, r2, specular_depth, smooth, textured)
            near[p] |= c["near"]
            ends[p] += c["light"] >= 0
            for key in DECISIONS:
                margin[key][p] = min(margin[key][p], c["margin"][key])
            if c["t"] is not None:
                st += c["t"]
                hits += 1
            if k == 0:
                mat0, light[p] = c["mat"], c["light"]
            sa += c["albedo"]
            sn += c["normal"]
        alb[p, :3] = sa / len(offsets)
        alb[p, 3] = mat0
        l = np.linalg.norm(sn)
        if l > 0:
            nd[p, :3] = sn / l
        nd[p, 3] = st / hits if hits else -1.0
    return alb, nd, near, margin, light, ends


def closest_margin(margin):
    """the smallest relative margin of any decision, per pixel"""
    return np.min(np.stack([margin[k] for k in DECISIONS]), axis=0)
