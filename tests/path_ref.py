"""Float64 numpy model of Scene.render_nee (include/pt_api.h pins the estimator): PathModel, the one path loop of tests/.  The same LCG
stream and hashes as the device, brute-force intersection, every feature of the NEE path as a setting: an environment, vertex normals,
albedo textures, the rough metal, the coated diffuse and the rough dielectric (material types 4, 5, 6), a thin lens, analytic lights,
sphere lights and suns, a medium with or without a density grid, interiors bound to glass, and a light tree in place of the light table.
A setting left at its default changes no bit of a sample.  The class names of the *_ref.py modules (nee_ref.Model ... interior_ref.
InteriorFrostedModel) are constructors that translate their arguments into these settings and fix the events they report; the pure
float64 functions a vertex is made of stay in those modules, where tests/test_*_host.py test them directly.  The model shares no code with
the library and calls nothing in it for arithmetic."""
import numpy as np

ALL_EVENTS = (
    "spec_fallback", "lobe_end", "ng_reject",
    "glossy_vertex", "glossy_end_wz", "glossy_end_ng", "glossy_light", "glossy_emitter_wb", "glossy_sky",
    "coated_coat", "coated_base", "coated_end_wz", "coated_end_ng", "coated_light", "coated_emitter_wb", "coated_sky",
    "frosted_reflect", "frosted_refract", "frosted_tir", "frosted_inside", "frosted_end_wz", "frosted_end_ng", "frosted_light", "frosted_emitter_wb",
    "frosted_sky", "frosted_through_emitter", "frosted_through_sky",
    "delta", "delta_glossy", "delta_ng_reject",
    "scatter", "scatter_light", "scatter_delta", "scatter_emitter_wb", "scatter_sky",
    "grid_scatter_thin", "grid_scatter_dense", "grid_empty_crossed", "grid_light_partial",
    "sphere_end", "sphere_end_rough", "sphere_end_scatter", "sun_miss", "area_sample", "area_glossy", "area_ng_reject", "sphere_blocks",
    "interior_scatter", "interior_absorbed", "interior_exit", "interior_then_light")

AREA_KEY = 0x9e3779b9
HIT_MARGIN = 1e-4               # a sphere decision nearer than this (relative) to its other outcome is a near-tie
SUN_RIM_MARGIN = 1e-4           # ... and a direction nearer than this share of 1 - cos a to a sun's rim
ROUGH = {4: "glossy", 5: "coated", 6: "frosted"}


def _bind():
    """The modules of the pure functions, bound on first use: each of them defines its class names on PathModel, so none can be imported
    while this module loads."""
    global A, K, E, F, G, GR, IR, LN, L, M, R, S, TX
    import arealights_ref as A
    import coated_ref as K
    import env_ref as E
    import frosted_ref as F
    import glossy_ref as G
    import grid_ref as GR
    import interior_ref as IR
    import lens_ref as LN
    import lights_ref as L
    import medium_ref as M
    import nee_ref as R
    import smooth_ref as S
    import texture_ref as TX


class PathModel:
    """verts (n,3,3), normals (n,3) (the Triangle records' N), mats (MATERIAL records), mat_of (n,), cam (CAMERA record); table =
    Scene.debug_light_table().  Settings, each off by default:
      env = dict(rgb=, tables=Scene.debug_environment(), scale=, yaw_degrees=); vnormals (n,3,3) as recorded, zero where a triangle has none;
      uvs, textures = [(texels, filter)], mat_tex = {material: texture}; glossy / coated / frosted: shade type 4 / 5 / 6 (else inert);
      lights = Scene.debug_lights(); area = Scene.debug_area_lights(); medium = Scene.medium(), density = Scene.medium_density();
      interiors = {material: Scene.material_interior()}; tree = lighttree_ref.Tree; set_lens(aperture, focus);
      events: the names self.events, self.last and self.pixel_events report;
      side_margins = False: the estimator as nee_ref.Model, env_ref.EnvModel and lighttree_ref.TreeModel first stated it, for flat
      triangles only -- no near-tie margins on a cosine's sign and no end of the path below the surface (without vertex normals the
      cosine lobe cannot leave the hemisphere, so only the near-tie mask differs)."""

    lens = None

    def __init__(self, verts, normals, mats, mat_of, cam, table=None, margin=1e-4, env=None, vnormals=None, uvs=None, textures=None, mat_tex=None,
                 glossy=False, coated=False, frosted=False, ps_margin=1e-5, fm_margin=1e-5, lights=None, area=None, medium=None, density=None,
                 dense_from=2.0, interiors=None, tree=None, events=(), side_margins=True):
        _bind()
        self.v = np.asarray(verts, dtype=np.float64).reshape(-1, 3, 3)
        self.n = np.asarray(normals, dtype=np.float64)[:, :3] if len(self.v) else np.zeros((0, 3))
        self.mats, self.mat_of, self.cam, self.margin = mats, np.asarray(mat_of), cam, margin
        self.side_margins = side_margins
        self.events = {e: 0 for e in events}
        self.e1 = self.v[:, 1] - self.v[:, 0]
        self.e2 = self.v[:, 2] - self.v[:, 0]
        # the light table
        self.lights, self.psel = R.light_table(self.v, mats, self.mat_of)
        if table is not None:          # Scene.debug_light_table(): the device's (packed) order of the same lights
            order = np.asarray(table[0], dtype=np.int64)
            assert sorted(order.tolist()) == sorted(self.lights.tolist())
            self.lights = order
        self.area = 0.5 * np.linalg.norm(np.cross(self.e1, self.e2), axis=1)
        # the cdf the device searches is the one the host rounded to float: the same selection for the same u0
        self.cdf = np.cumsum(self.psel).astype(np.float32)
        if len(self.cdf):
            self.cdf[-1] = 1.0
        if table is not None:
            self.cdf = np.asarray(table[1], dtype=np.float32)
            self.psel = R.selection_probs(self.cdf)
        self.pdf_area = np.zeros(len(self.v))
        self.pdf_area[self.lights] = self.psel / self.area[self.lights]
        self.tree = tree
        if tree is not None:
            assert sorted(tree.tri.tolist()) == sorted(int(x) for x in self.lights)
        # the environment
        self.rgb, self.pe, self.has_dist = None, 0.0, False
        if env is not None:
            self.rgb = np.asarray(env["rgb"], dtype=np.float32).astype(np.float64)
            self.h, self.w = self.rgb.shape[:2]
            self.scale = float(np.float32(env.get("scale", 1.0)))
            self.yaw_degrees = env.get("yaw_degrees", 0.0)
            self.row_cdf = np.asarray(env["tables"]["row_cdf"], dtype=np.float32)
            self.col_cdf = np.asarray(env["tables"]["col_cdf"], dtype=np.float32)
            self.pdf = np.asarray(env["tables"]["pdf"], dtype=np.float64)
            self.pe = float(env["tables"]["P_env"])
            self.has_dist = bool((self.pdf > 0).any())
        # vertex normals, textures, the rough materials
        if vnormals is None:
            vnormals = np.zeros(self.v.shape, dtype=np.float32)
        self.has = S.has_normals(vnormals)
        self.vn = S.unit64(np.asarray(vnormals, dtype=np.float32).reshape(-1, 3, 3))
        self.textures = None
        if textures is not None:
            self.uv = np.asarray(uvs, dtype=np.float32).reshape(-1, 3, 2)
            self.has_uv = TX.has_uvs(self.uv)
            self.textures = [(np.asarray(t, dtype=np.float32), int(f)) for t, f in textures]
            self.mat_tex = dict(mat_tex)
            self.textured_vertices = 0
        self.glossy, self.coated, self.frosted, self.ps_margin, self.fm_margin = glossy, coated, frosted, ps_margin, fm_margin
        # analytic lights, area lights
        lights = lights if lights is not None else M.NO_LIGHTS
        self.set = L.parse_records(lights["records"])
        self.set_cdf = np.asarray(lights["cdf"], dtype=np.float32)
        self.pa = float(lights["P_ana"])
        self.spheres, self.suns, self.sun_q, self.area_L, self.area_pl, self.par = [], [], [], [], [], 0.0
        if area is not None:
            rec = np.asarray(area["records"], dtype=np.float64)
            ns = int(area["n_sphere"])
            self.spheres = [(rec[j, :3], rec[j, 3]) for j in range(ns)]
            self.suns = [(rec[j, :3], rec[j, 3]) for j in range(ns, len(rec))]
            self.sun_q = [rec[j, 8] for j in range(ns, len(rec))]
            self.area_L = [rec[j, 4:7] for j in range(len(rec))]
            self.area_pl = [float(p) for p in area["P_light"]]
            self.area_cdf = np.asarray(area["cdf"], dtype=np.float32)
            self.par = float(area["P_area"])
        # the medium, its grid, the interiors
        self.medium = M.medium_of(medium)
        self.density = None if density is None or self.medium is None else np.asarray(density, dtype=np.float64)
        self.dense_from = dense_from           # a scatter vertex counts as "dense" in a voxel of at least this density, else "thin"
        self.interiors = {int(k): IR.interior_of(x) for k, x in (interiors or {}).items() if x is not None}

    # ------------------------------------------------------------------------ geometry
    def intersect(self, P, D, limit=np.inf):
        """closest triangle with 0 < t < limit (index, t) and whether the answer is a near-tie (an edge within `margin` in
        barycentric terms, or two hits within a relative 1e-5 of each other)."""
        if not len(self.v):
            return -1, np.inf, False
        pv = np.cross(D, self.e2)
        det = np.einsum("ij,ij->i", self.e1, pv)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            s = P - self.v[:, 0]
            u = np.einsum("ij,ij->i", s, pv) * inv
            q = np.cross(s, self.e1)
            w = (q @ D) * inv
            t = np.einsum("ij,ij->i", self.e2, q) * inv
        ok = np.isfinite(t) & (np.abs(det) > 1e-12)
        bmin = np.minimum(np.minimum(u, w), 1.0 - u - w)
        inside = ok & (bmin >= 0) & (t > 0) & (t < limit)
        near = ok & (np.abs(bmin) < self.margin) & (t > 0) & (t < limit * 1.001)
        if not inside.any():
            return -1, np.inf, bool(near.any())
        tt = np.where(inside, t, np.inf)
        i = int(np.argmin(tt))
        others = np.delete(tt, i)
        tie = bool(near.any()) or bool((np.abs(others - tt[i]) <= 1e-5 * tt[i]).any())
        return i, float(tt[i]), tie

    def set_lens(self, aperture, focus):
        self.lens = (float(aperture), float(focus)) if aperture > 0 else None
        return self

    def camera_ray(self, gid, rnd1, rnd2):
        """the pinhole ray, or once set_lens(aperture > 0, focus) was called the lens ray of the sample whose seed sample() was given"""
        if self.lens is not None:
            P, D, _ = LN.lens_rays(self.cam, self.lens[0], self.lens[1], [gid], [self._lens_key], rnd=([rnd1], [rnd2]))
            return P[0], D[0]
        c = self.cam
        X, Y = int(c["XM"]), int(c["YM"])
        x = float(gid % X) + rnd1
        y = float(gid // X) + rnd2
        right = c["right"][:3].astype(np.float64) * ((2.0 * x) / X - 1.0)
        up = c["up"][:3].astype(np.float64) * ((2.0 * y) / Y - 1.0)
        pp = c["lookat"][:3].astype(np.float64) + right + up
        eye = c["eye"][:3].astype(np.float64)
        d = pp - eye
        return eye, d / np.linalg.norm(d)

    @staticmethod
    def diffuse_dir(N, rnd1, rnd2):
        E = 0.001
        if abs(N[0]) <= E and abs(N[2]) <= E:
            rl = 1.0 / np.sqrt(N[2] * N[2] + N[1] * N[1])
            Z = np.array([0.0, -N[2] * rl, N[1] * rl])
        else:
            rl = 1.0 / np.sqrt(N[2] * N[2] + N[0] * N[0])
            Z = np.array([-N[2] * rl, 0.0, N[0] * rl])
        X = np.cross(N, Z)
        r = np.sqrt(rnd1)
        th = 2.0 * np.pi * rnd2
        d = X * (r * np.cos(th)) + N * np.sqrt(1.0 - rnd1) + Z * (r * np.sin(th))
        return d / np.linalg.norm(d)

    # ------------------------------------------------------------------------ materials
    def _mat(self, ti):
        return self.mats[int(self.mat_of[ti])]

    def albedo_at(self, ti, hp):
        """(kd', near a decision, textured) of a hit at hp on triangle ti"""
        m = self._mat(ti)
        kd = m["kd"][:3].astype(np.float64)
        T = self.mat_tex.get(int(self.mat_of[ti]), -1) if self.textures is not None else -1
        if int(m["type"]) != 0 or T is None or T < 0 or not self.has_uv[ti]:
            return kd, False, False
        texels, filt = self.textures[T]
        out, near = TX.albedo(kd, self.v[ti], self.n[ti], hp, self.uv[ti], texels, filt)
        return out, near, True

    def _update(self, ti, N, hp, w, fL, fB):
        """the diffuse vertex with its Phong lobe: (factor_L, factor_B) after the direction w, and a near tie of the texture lookup"""
        m = self._mat(ti)
        kd, near, textured = self.albedo_at(ti, hp)
        if self.textures is not None:
            self.textured_vertices += int(textured)
        ks = m["ks"][:3].astype(np.float64)
        cosx = max(0.0, float(N @ w))
        fL = fL * (kd * cosx)
        pw = 1.0
        if not int(m["_pad"]):
            view = self.cam["eye"][:3].astype(np.float64) - hp
            view /= np.linalg.norm(view)
            h = view + w
            h /= np.linalg.norm(h)
            pw = max(0.0, float(N @ h)) ** float(m["shininess"])
        return fL, fB * (ks * pw), near

    def _spec(self, m, typ, N, D, inside, rnd):
        """the mirror / dielectric vertex with normal N: (direction before normalisation, refracted, F, prob, near a decision)"""
        F0 = m["F0"][:3].astype(np.float64)
        cosa = abs(float(N @ D))
        F = F0 + (1.0 - F0) * (1.0 - cosa) ** 5
        d = D - N * (2.0 * float(N @ D))
        if typ != 2:
            return d, False, F, 0.0, False
        n = float(m["n"])
        if inside:
            n = 1.0 / n
        c = float(-D @ N)
        disc = 1.0 - (1.0 - c * c) / n / n
        prob = float(F.sum()) / 3.0
        near = abs(disc) < 1e-5 or abs(rnd - prob) < 1e-5
        refr = disc > 0 and rnd > prob
        if refr:
            d = D / n + N * (c / n - np.sqrt(disc))
        return d, refr, F, prob, near

    def _glossy(self, m, N, D, r1=0.0, r2=0.0):
        v = G.vertex(N[None], D[None], [G.roughness(m["shininess"])], [r1], [r2], m["F0"][:3])
        return {k: x[0] for k, x in v.items()}

    def _coated(self, m, N, D, r1=0.0, r2=0.0, us=0.0):
        v = K.vertex(N[None], D[None], [G.roughness(m["shininess"])], m["F0"][:3], m["kd"][:3], [r1], [r2], [us])
        return {k: x[0] for k, x in v.items()}

    def _frosted(self, m, N, D, inside, r1=0.0, r2=0.0, us=0.0):
        n = float(m["n"])
        eta = float(np.float32(1.0) / np.float32(n)) if inside else n
        v = F.vertex(N[None], D[None], [G.roughness(m["shininess"])], m["F0"][:3], [eta], [r1], [r2], [us])
        out = {k: x[0] for k, x in v.items()}
        out["eta"] = float(np.float32(eta))
        return out

    def _rough_eval(self, fam, m, N, D, w, inside, fS, fR):
        """a light sample's direction w at a rough vertex of family fam: (p_b, factor_S and factor_R with the vertex's weight, near a decision)"""
        al = np.array([G.roughness(m["shininess"])])
        F0 = m["F0"][:3].astype(np.float64)[None]
        if fam == "glossy":
            gv = self._glossy(m, N, D)
            wl3 = np.array([w @ gv["X"], w @ gv["Z"], w @ N])
            pbv, h = G.ggx_pdf_of(al, gv["o"][None], wl3[None])
            return float(pbv[0]), fS * G.schlick(F0, h, gv["o"][None])[0] * float(G.ggx_G1(al, wl3[None])[0]), fR, False
        if fam == "coated":
            cv = self._coated(m, N, D)
            wl3 = np.array([w @ cv["X"], w @ cv["Z"], w @ N])
            pbv, gg, _, _ = K.evaluate_of(al, F0, m["kd"][:3].astype(np.float64)[None], cv["o"][None], wl3[None])
            return float(pbv[0]), fS * gg[0], fR, False
        fv = self._frosted(m, N, D, inside)
        wl3 = np.array([w @ fv["X"], w @ fv["Z"], w @ N])
        oo = fv["o"][None]
        hh = G.unit(oo + wl3[None])
        et = np.array([fv["eta"]])
        pbv, gg = F.reflect_terms(al, F0, et, oo, hh, wl3[None])
        _, _, dd, _, _ = F.terms(F0, et, oo, hh)
        return float(pbv[0]), fS, fR * gg[0], abs(float(dd[0])) < self.fm_margin

    # ------------------------------------------------------------------------ the sky
    def sky(self, d):
        """(E(d), p_env(d), near a texel edge)"""
        row, col, dist = E.lookup(self.w, self.h, self.yaw_degrees, d)
        return self.rgb[row, col] * self.scale, float(self.pdf[row, col]), dist < E.EDGE_MARGIN

    def sky_sample(self, u1, u2):
        """(direction, E, p_env) of the texel u1, u2 pick"""
        row = min(int(np.searchsorted(self.row_cdf, np.float32(u1), side="right")), self.h - 1)
        rb = float(self.row_cdf[row - 1]) if row else 0.0
        t1 = (u1 - rb) / (float(self.row_cdf[row]) - rb)
        cc = self.col_cdf[row]
        col = min(int(np.searchsorted(cc, np.float32(u2), side="right")), self.w - 1)
        cb = float(cc[col - 1]) if col else 0.0
        t2 = (u2 - cb) / (float(cc[col]) - cb)
        c0, c1 = np.cos(np.pi * row / self.h), np.cos(np.pi * (row + 1) / self.h)
        ct = c0 - t1 * (c0 - c1)
        sn = np.sqrt(max(0.0, 1.0 - ct * ct))
        phi = 2.0 * np.pi * ((col + t2) / self.w) + E.yaw_radians(self.yaw_degrees)
        return np.array([sn * np.cos(phi), ct, sn * np.sin(phi)]), self.rgb[row, col] * self.scale, float(self.pdf[row, col])

    # ------------------------------------------------------------------------ the medium
    def _walk(self, P, D, t, tau):
        med = self.medium
        w = GR.walk(med["sigma_t"], self.density, med["lo"], med["hi"], P, D, t, tau)
        return w, w["near"] or w["margin"] < GR.SCATTER_MARGIN

    def _flight(self, P, D, t, u, ev):
        """the free flight of a segment that is ell > 0 long inside the medium, as a distance past the clip's entry a: (d, near a decision).
        With a grid the walk decides: (t_cur - a) + d of the voxel that scatters, or +inf, so that `d < ell` and `a + d` decide and place as
        the walk did"""
        if self.density is None:
            return M.flight(self.medium["sigma_t"], u), False
        w, near = self._walk(P, D, t, -np.log1p(-u))
        rho = self.density.reshape(-1)
        crossed = [v for v, t0, t1 in w["voxels"][:-1 if w["scatter"] else None] if t1 > t0]
        ev["grid_empty_crossed"] += int(any(rho[v] == 0.0 for v in crossed) and any(rho[v] > 0.0 for v in crossed))
        if not w["scatter"]:
            return np.inf, near
        ev["grid_scatter_dense" if rho[w["voxel"]] >= self.dense_from else "grid_scatter_thin"] += 1
        return (w["t_cur"] - w["a"]) + w["d"], near

    def _transmittance(self, o, w, cut, inside, ev):
        """T of a light sample taken outside a dielectric: (T, near a decision)"""
        if self.medium is None or inside:
            return 1.0, False
        if self.density is None:
            return M.transmittance(self.medium, o, w, cut)
        k, near = self._walk(o, w, cut, np.inf)
        T = float(np.exp(-k["acc"]))
        lit = {v for v, t0, t1 in k["voxels"] if t1 > t0 and self.density.reshape(-1)[v] > 0.0}
        ev["grid_light_partial"] += int(0.0 < T < 1.0 and len(lit) >= 2)
        return T, near

    # ------------------------------------------------------------------------ light samples
    def _p_triangle(self, ti, o, Ng):
        """the area density with which a light sample from (o, Ng) picks a point of triangle ti, before the 1 - P factors"""
        if self.tree is None:
            return self.pdf_area[ti]
        return self.tree.weight(o, Ng, self.tree.slot_of.get(int(ti), -1)) / self.area[ti]

    def _candidate(self, key, k, o, Ng, ev):
        """the light sample of segment k seen from o: (cand, near a decision); cand = None, or (E, p_l, emitter cosine, w, what the
        shadow ray must return, its cut, delta, the sphere aimed at or -1, of the area set).  The chain: u_area < P_area the area set, else
        u_ana < P_ana the analytic set, else u_sky < P_env the sky, else a triangle of the table or the tree; each later branch carries the
        1 - P of those before it"""
        nkey = ~key & 0xFFFFFFFF
        pe, pa, par = self.pe, self.pa, self.par
        u0 = R.nee_unit(R.nee_rand(key, k, 0))
        u1 = R.nee_unit(R.nee_rand(key, k, 1))
        u2 = R.nee_unit(R.nee_rand(key, k, 2))
        tie = False
        if par > 0:
            uar = R.nee_unit(R.nee_rand((key ^ AREA_KEY) & 0xFFFFFFFF, k, 0))
            tie |= abs(uar - par) < L.SELECT_MARGIN and 0.0 < par < 1.0
            if uar < par:
                j = min(int(np.searchsorted(self.area_cdf, np.float32(u0), side="right")), len(self.area_cdf) - 1)
                ev["area_sample"] += 1
                aim = -1
                if j < len(self.spheres):
                    smp = A.sphere_sample(self.spheres[j][0], self.spheres[j][1], o, u1, u2, np.float64)
                    aim = j
                else:
                    s_ = j - len(self.spheres)
                    smp = A.sun_sample(self.suns[s_][0], self.sun_q[s_], u1, u2, np.float64)
                pl = par * self.area_pl[j]
                if smp is None or not pl > 0:
                    return None, tie
                return (self.area_L[j], pl * float(smp[1]), 1.0, smp[0], -1, float(smp[2]), False, aim, True), tie
        cand = None
        use_ana = False
        if pa > 0:
            ua = R.nee_unit(R.nee_rand(nkey, k, 2))
            tie |= abs(ua - pa) < L.SELECT_MARGIN and 0.0 < pa < 1.0
            use_ana = ua < pa
        if use_ana:
            j = min(int(np.searchsorted(self.set_cdf, np.float32(u0), side="right")), len(self.set_cdf) - 1)
            smp = L.light_sample(self.set[j], o)
            pl = pa * self.set[j]["P_light"]
            if smp is not None and pl > 0:
                cand = (smp[2], pl, 1.0, smp[0], -1, smp[1], True)
        else:
            use_sky = False
            if self.rgb is not None:
                us = R.nee_unit(R.nee_rand(nkey, k, 0))
                tie |= abs(us - pe) < L.SELECT_MARGIN and 0.0 < pe < 1.0
                use_sky = us < pe
            if use_sky:
                w, Ey, penv = self.sky_sample(u1, u2)
                pl = pe * penv * (1.0 - pa)
                if pl > 0:
                    cand = (Ey, pl, 1.0, w, -1, np.inf, False)
            elif len(self.lights):
                if self.tree is None:
                    j = min(int(np.searchsorted(self.cdf, np.float32(u0), side="right")), len(self.cdf) - 1)
                    li = int(self.lights[j])
                    pdf = self.pdf_area[li]
                else:
                    slot, Psel, _ = self.tree.pick(o, Ng, u0)
                    li = int(self.tree.tri[slot])
                    pdf = Psel / self.area[li]
                v = self.v[li]
                su = np.sqrt(u1)
                y = v[0] + (v[1] - v[0]) * (u2 * su) + (v[2] - v[0]) * (su * (1.0 - u2))
                d = y - o
                r = np.linalg.norm(d)
                w = d / r
                cosy = abs(float(w @ self.n[li]))
                if cosy > 0:
                    pl = pdf * (1.0 - pe) * (1.0 - pa) * r * r / cosy
                    if pl > 0:
                        cand = (self._mat(li)["emission"][:3].astype(np.float64), pl, cosy, w, li, r * R.SHADOW_CUT, False)
        if cand is not None:
            cand = (cand[0], cand[1] * (1.0 - par)) + cand[2:] + (-1, False)
        return cand, tie

    def _shadow(self, o, w, want, cut, aim):
        """(the shadow ray returns `want`, a sphere light other than the one aimed at blocks it, near a decision)"""
        hi, _, tie = self.intersect(o, w, cut)
        blk = False
        if self.spheres:
            bj, _, bm = A.sphere_hit([sp for i_, sp in enumerate(self.spheres) if i_ != aim], o, w, cut, np.float64)
            blk = bj >= 0
            tie |= self._near(bm)
        return hi == want, blk, tie

    @staticmethod
    def _near(margins):
        """a sphere decision that a rounding could flip: the origin on the surface, a grazing ray, or two candidates at one distance"""
        return any(min(m) < HIT_MARGIN for m in margins)

    # ------------------------------------------------------------------------ the path
    def sample(self, gid, seed, iterations, strategy):
        """one sample of pixel gid: (colour, new LCG state, near-tie seen); self.last = the sample's events"""
        if iterations == 1 and self.textures is not None:
            raise NotImplementedError("the preview of iterations == 1 is not modelled with textures")
        ev = {e: 0 for e in ALL_EVENTS}
        med, flat = self.medium, not self.side_margins
        self._lens_key = int(seed)
        key = int(seed) & 0xFFFFFFFF
        nkey = ~key & 0xFFFFFFFF
        mkey = key ^ M.STREAM
        tie = False
        seed, r1 = R.lcg(seed)
        seed, r2 = R.lcg(seed)
        P, D = self.camera_ray(gid, r1, r2)
        one = np.ones(3)
        fL, fB, fS, fR, C = one.copy(), one.copy(), one.copy(), one.copy(), np.zeros(3)
        # after_lobe: the previous vertex sampled a direction a light sample competes with; Nprev, NGprev: its normals; pb_prev: the p_b a
        # rough or scatter vertex sampled with (None: cosine lobe) and prev its kind; through: the previous vertex refracted through a
        # type-6 surface (after_lobe is False then)
        after_lobe, Nprev, NGprev, pb_prev, prev, inside, through = False, None, None, None, None, False, False
        scattered_inside, ever_scattered = False, False      # an interior scatter since the path entered / anywhere on the path
        sky = self.rgb is not None
        pe, pa, par = self.pe, self.pa, self.par
        nee = strategy != 0 and (len(self.lights) > 0 or sky or pa > 0 or par > 0)

        def W_b(pl, Dn):
            """the weight of a path that ends on a light whose density from the previous vertex is pl"""
            if not (nee and after_lobe and pl > 0):
                return 1.0
            if strategy == 1:
                return 0.0
            pb = pb_prev if pb_prev is not None else max(0.0, float(Nprev @ Dn)) / np.pi
            return pb * pb / (pb * pb + pl * pl)

        def W_l(pb, pl, delta):
            return pb / pl if strategy == 1 or delta else pb * pl / (pb * pb + pl * pl)

        for k in range(iterations):
            # ---- the segment: the closest hit, cut at the nearest sphere light before any free flight looks at its length
            ti, t, tt = self.intersect(P, D)
            tie |= tt
            sj, tend = -1, (t if ti >= 0 else np.inf)
            if self.spheres:
                sj, tend, marg = A.sphere_hit(self.spheres, P, D, tend, np.float64)
                tie |= self._near(marg)
            if inside and ti >= 0:
                it = self.interiors.get(int(self.mat_of[ti]))
                if it is not None and int(self._mat(ti)["type"]) in (2, 6):          # (the type alone, as the device table: not option frosted)
                    ell, sc = float(t), False
                    if it["sigma_s"] > 0:
                        d = M.flight(it["sigma_s"], R.nee_unit(R.nee_rand(mkey, k, 0)))
                        tie |= abs(d - t) < M.FLIGHT_MARGIN * max(d, t)
                        if d < t:
                            ell, sc = d, True
                    fS = fS * np.exp(-it["sigma_a"] * ell)
                    if not fS.any():
                        break
                    if sc:
                        ev["interior_scatter"] += 1
                        scattered_inside, ever_scattered = True, True
                        nd, _, _ = M.direction(it["g"], D, R.nee_unit(R.nee_rand(mkey, k, 1)), R.nee_unit(R.nee_rand(mkey, k, 2)))
                        P, D = P + D * d, nd
                        after_lobe, Nprev, pb_prev, prev, through = False, None, None, None, False
                        continue
                    ev["interior_absorbed"] += int(it["sigma_a"].any())
            if med is not None and not inside:
                a, b, near = M.clip(med["lo"], med["hi"], P, D, tend)
                tie |= near
                ell = max(b - a, 0.0)
                if ell > 0:
                    d, near = self._flight(P, D, tend, R.nee_unit(R.nee_rand(mkey, k, 0)), ev)
                    tie |= near
                    if np.isfinite(ell):
                        tie |= abs(d - ell) < M.FLIGHT_MARGIN * max(d, ell)
                    if d < ell:                     # the scatter vertex
                        ev["scatter"] += 1
                        x = P + D * (a + d)
                        fS = fS * med["albedo"]
                        if not fS.any():
                            break
                        if nee and k + 1 < iterations:
                            cand, near = self._candidate(key, k, x, None, ev)
                            tie |= near
                            if cand is not None:
                                Ey, pl, g, w, want, cut, delta, aim, _ = cand
                                hit, blk, near = self._shadow(x, w, want, cut, aim)
                                tie |= near
                                if hit and not blk:
                                    T, near = self._transmittance(x, w, cut, inside, ev)
                                    tie |= near
                                    ev["scatter_light"] += 1
                                    ev["scatter_delta"] += int(delta)
                                    C = C + Ey * (fL + fB) * fS * fR * (g * W_l(M.hg(med["g"], float(D @ w)), pl, delta)) * T
                        nd, pb_prev, _ = M.direction(med["g"], D, R.nee_unit(R.nee_rand(mkey, k, 1)), R.nee_unit(R.nee_rand(mkey, k, 2)))
                        P, D = x, nd
                        after_lobe, Nprev, NGprev, prev, through = True, None, None, "scatter", False
                        continue
            rough_prev = after_lobe and prev in ("glossy", "coated", "frosted")
            if sj >= 0:                        # the segment reaches the sphere light: the path ends on it
                Ls = self.area_L[sj]
                if k == 0:
                    C = C + Ls
                else:
                    q = A.sphere_q(self.spheres[sj][0], self.spheres[sj][1], P, np.float64)[0]
                    C = C + Ls * (fL + fB) * fS * fR * W_b(par * self.area_pl[sj] / (2.0 * np.pi * q), D)
                ev["sphere_end"] += 1
                ev["sphere_end_rough"] += int(k > 0 and rough_prev)
                ev["sphere_end_scatter"] += int(k > 0 and prev == "scatter")
                break
            # ---- the miss: suns and sky
            if ti < 0:
                if self.suns:
                    mask, smarg = A.sun_mask(self.suns, D, np.float64)
                    tie |= any(m_ < SUN_RIM_MARGIN * (1.0 - ca) for m_, (_, ca) in zip(smarg, self.suns))
                    for s_ in range(len(self.suns)):
                        if mask >> s_ & 1:
                            j_ = len(self.spheres) + s_
                            Ls = self.area_L[j_]
                            C = C + (Ls if k == 0 else Ls * (fL + fB) * fS * fR * W_b(par * self.area_pl[j_] / (2.0 * np.pi * self.sun_q[s_]), D))
                            ev["sun_miss"] += 1
                if sky:
                    Esky, penv, edge = self.sky(D)
                    tie |= edge
                    if k == 0:
                        C = C + Esky
                    else:
                        wb = W_b(pe * penv * (1.0 - pa) * (1.0 - par), D)
                        if after_lobe and prev is not None:
                            ev[prev + "_sky"] += 1
                        ev["frosted_through_sky"] += int(through)
                        ev["interior_then_light"] += int(ever_scattered)
                        C = C + Esky * (fL + fB) * fS * fR * wb
                break
            # ---- the surface vertex
            m = self._mat(ti)
            typ = int(m["type"])
            fam = ROUGH.get(typ) if getattr(self, ROUGH.get(typ, ""), False) else None
            N0 = self.n[ti].copy()
            hp = P + D * t
            Em = m["emission"][:3].astype(np.float64)
            if iterations == 1:
                C = (m["F0"][:3] if fam == "glossy" else m["kd"][:3]).astype(np.float64) + Em
            Ng = -N0 if D @ N0 > 0 else N0
            N, _, near = S.shading_normal(self.v[ti], N0, self.vn[ti], bool(self.has[ti]), D, hp)
            tie |= near
            if typ in (0, 3) or fam:
                inten = max(0.0, float(-D @ N))
                wb = 1.0
                ev["frosted_through_emitter"] += int(typ == 3 and through)
                if typ == 3 and nee and after_lobe and inten > 0:
                    parea = self._p_triangle(ti, P, NGprev) * (1.0 - pe) * (1.0 - pa) * (1.0 - par)
                    if parea > 0:
                        wb = W_b(parea * t * t / inten, D)
                        if prev is not None and wb < 1.0:
                            ev[prev + "_emitter_wb"] += 1
                o = hp + Ng * 0.001
                if nee and k + 1 < iterations:
                    cand, near = self._candidate(key, k, o, Ng, ev)
                    tie |= near
                    if cand is not None:
                        Ey, pl, g, w, want, cut, delta, aim, of_area = cand
                        cosx, cosg = float(N @ w), float(Ng @ w)
                        if not flat:
                            tie |= abs(cosx) < S.SIDE_MARGIN or abs(cosg) < S.SIDE_MARGIN
                        if cosx > 0 and not cosg > 0:
                            ev["ng_reject"] += 1
                            ev["area_ng_reject"] += int(of_area)
                            ev["delta_ng_reject"] += int(delta)
                        if cosx > 0 and cosg > 0:
                            hit, blk, near = self._shadow(o, w, want, cut, aim)
                            tie |= near
                            ev["sphere_blocks"] += int(blk and hit)
                            if hit and not blk:
                                T, near = self._transmittance(o, w, cut, inside, ev)
                                tie |= near
                                fs, frr = fS, fR
                                if fam:
                                    pb, fs, frr, near = self._rough_eval(fam, m, N, D, w, inside, fS, fR)
                                    tie |= near
                                    ev[fam + "_light"] += 1
                                    if fam == "glossy":
                                        ev["area_glossy"] += int(of_area and pb > 0)
                                        ev["delta_glossy"] += int(delta and pb > 0)
                                else:
                                    pb = cosx / np.pi
                                if pb > 0:                   # (a rough vertex with no density adds nothing)
                                    ev["delta"] += int(delta)
                                    fl, fb = fL, fB
                                    if typ == 0:
                                        fl, fb, near = self._update(ti, N, hp, w, fL, fB)
                                        tie |= near
                                    C = C + Ey * (fl + fb) * fs * frr * (g * W_l(pb, pl, delta)) * T
                seed, r1 = R.lcg(seed)
                seed, r2 = R.lcg(seed)
                ended, refr = False, False
                if fam == "glossy":
                    gv = self._glossy(m, N, D, r1, r2)
                    ev["glossy_vertex"] += 1
                    tie |= bool(gv["l2"] < G.DEGENERATE_L2) or abs(float(gv["w"][2])) < S.SIDE_MARGIN
                    nd = gv["world"] / np.linalg.norm(gv["world"])
                    fS = fS * gv["g"]
                    pb_prev = float(gv["pb"])
                    ended = not gv["w"][2] > 0
                elif fam == "coated":
                    us = R.nee_unit(R.nee_rand(nkey, k, 1))
                    cv = self._coated(m, N, D, r1, r2, us)
                    tie |= abs(us - float(cv["ps"])) < self.ps_margin
                    ev["coated_coat" if cv["coat"] else "coated_base"] += 1
                    tie |= (bool(cv["coat"]) and bool(cv["l2"] < G.DEGENERATE_L2)) or abs(float(cv["w"][2])) < S.SIDE_MARGIN
                    nd = cv["world"] / np.linalg.norm(cv["world"])
                    fS = fS * cv["g"]
                    pb_prev = float(cv["pb"])
                    ended = not (cv["w"][2] > 0 and cv["pb"] > 0)
                elif fam == "frosted":
                    us = R.nee_unit(R.nee_rand(nkey, k, 1))
                    fv = self._frosted(m, N, D, inside, r1, r2, us)
                    tie |= abs(us - float(fv["Fm"])) < self.fm_margin and not bool(fv["tir"])
                    tie |= abs(float(fv["disc"])) < self.fm_margin
                    tie |= bool(fv["l2"] < G.DEGENERATE_L2) or abs(float(fv["w"][2])) < S.SIDE_MARGIN
                    refr = not bool(fv["refl"])
                    ev["frosted_refract" if refr else "frosted_reflect"] += 1
                    ev["frosted_tir"] += int(bool(fv["tir"]))
                    ev["frosted_inside"] += int(inside)
                    nd = fv["world"] / np.linalg.norm(fv["world"])
                    fR = fR * fv["g"]
                    pb_prev = float(fv["pb"])
                    if refr:
                        ev["interior_exit"] += int(inside and scattered_inside)
                        inside = not inside
                        scattered_inside = False
                    ended = not (fv["w"][2] < 0 if refr else fv["w"][2] > 0)
                else:
                    nd = self.diffuse_dir(N, r1, r2)
                    pb_prev = None
                    if typ == 0:
                        fL, fB, near = self._update(ti, N, hp, nd, fL, fB)
                        tie |= near
                    else:
                        C = C + Em * (fL + fB) * fS * fR * (inten * wb)
                        ev["interior_then_light"] += int(ever_scattered and bool(Em.any()) and inten * wb > 0)
                if ended:
                    ev[fam + "_end_wz"] += 1
                P, D = hp + Ng * (-0.001 if refr else 0.001), nd
                after_lobe, Nprev, NGprev, prev, through = not refr, N, Ng, fam, refr
                if refr:
                    pb_prev, prev = None, None
                if flat:
                    continue
                below = float(nd @ Ng)
                tie |= abs(below) < S.SIDE_MARGIN
                if ended:
                    break
                if (below >= 0) if refr else (below <= 0):
                    ev[fam + "_end_ng" if fam else "lobe_end"] += 1
                    break
            elif typ in (1, 2):
                rnd = 0.0
                if typ == 2:
                    seed, rnd = R.lcg(seed)
                d, refr, Fr, prob, near = self._spec(m, typ, N, D, inside, rnd)
                tie |= near
                g = float(d @ Ng) / np.linalg.norm(d)
                if not flat:
                    tie |= abs(g) < S.SIDE_MARGIN
                if (g >= 0) if refr else (g <= 0):
                    ev["spec_fallback"] += 1
                    d, refr, Fr, prob, near = self._spec(m, typ, Ng, D, inside, rnd)
                    tie |= near
                if typ == 1:
                    fS = fS * Fr
                elif refr:
                    fR = fR * (1.0 - Fr) / (1.0 - prob)
                    ev["interior_exit"] += int(inside and scattered_inside)
                    inside = not inside
                    scattered_inside = False
                else:
                    fR = fR * Fr / prob
                P, D = hp + Ng * (-0.001 if refr else 0.001), d / np.linalg.norm(d)
                after_lobe, pb_prev, prev, through = False, None, None, False
            # any other type: the ray is left unchanged and the loop hits the same surface again
        self.last = {e: ev[e] for e in self.events}
        return C, seed, bool(tie)

    def render(self, seeds, iterations, nsamples, strategy):
        """colors (npix, 3) float64, final LCG states, near-tie mask; pixel i is global pixel i (world 1); self.pixel_events[name] =
        per-pixel counts"""
        n = len(seeds)
        cols = np.zeros((n, 3))
        out_seeds = np.zeros(n, dtype=np.int64)
        ties = np.zeros(n, dtype=bool)
        self.pixel_events = {e: np.zeros(n, dtype=np.int64) for e in self.events}
        for i in range(n):
            s = int(seeds[i])
            acc = np.zeros(3)
            for _ in range(nsamples):
                c, s, t = self.sample(i, s, iterations, strategy)
                acc += c
                ties[i] |= t
                for e, x in self.last.items():
                    self.pixel_events[e][i] += x
            cols[i] = acc / nsamples
            out_seeds[i] = s
        return cols, out_seeds.astype(np.int32), ties
