"""A numpy restatement of the area lights of render_nee (include/pt_api.h): the table as pt_set_area_lights builds it,
and the sample and hit functions of the kernel, each in a precision f of the caller's choice (float64: the reference; float32: the same
formulas in the device's precision, whose distance from float64 is the rounding spread the GPU test's tolerance is built from).  The hit
function reports its decisions' margins (sphere-hit discriminants and distances, sun-disc cosines) so that a test can refuse items whose
outcome a rounding could flip.  AreaLightsModel, below, is the float64 path model: medium_ref.MediumModel (lights_ref.LightsModel plus a medium) with the area set added."""

import numpy as np

SPHERE, SUN = 0, 1


def table(lights):
    """lights: api.AreaLight structures as given to set_area_lights -> order, records (n, 12) float32, cdf, P_light, weights (float64)"""
    n = len(lights)
    order = [i for i, l in enumerate(lights) if l.type == SPHERE] + [i for i, l in enumerate(lights) if l.type == SUN]
    rec = np.zeros((n, 12), dtype=np.float32)
    w = np.zeros(n)
    for k, i in enumerate(order):
        l = lights[i]
        L = np.array(list(l.radiance), dtype=np.float64)
        s = (L[0] + L[1]) + L[2]
        if l.type == SPHERE:
            rec[k, :3] = list(l.position)
            rec[k, 3] = l.size
            auto = s * (4.0 * np.pi * np.pi) * (float(l.size) * float(l.size))
        else:
            d = np.array(list(l.direction), dtype=np.float64)
            rec[k, :3] = -d / np.sqrt((d * d).sum())
            q = 2.0 * np.sin(0.5 * float(l.size)) ** 2
            rec[k, 3] = np.cos(float(l.size))
            rec[k, 8] = q
            auto = s * (2.0 * np.pi) * q
        rec[k, 4:7] = L
        w[k] = float(l.weight) if l.weight > 0 else auto
        if s == 0.0 or not np.isfinite(w[k]):
            w[k] = 0.0
    total = w.sum()
    any_ = total > 0 and np.isfinite(total)
    last = int(np.nonzero(w > 0)[0].max()) if any_ else 0
    cdf = np.zeros(n, dtype=np.float32)
    run = 0.0
    for k in range(n):
        run += w[k] if any_ else 1.0
        cdf[k] = 1.0 if (k >= last or k + 1 == n) else np.float32(run / (total if any_ else n))
    upto = np.ceil(cdf.astype(np.float64) * 2 ** 24)
    pl = (np.diff(np.concatenate([[0.0], upto])) / 2 ** 24).astype(np.float32) if any_ else np.zeros(n, dtype=np.float32)
    rec[:, 7] = pl
    return {"order": np.asarray(order, dtype=np.int32), "records": rec, "cdf": cdf, "P_light": pl, "weights": w}


def cone_density(q):
    return 1.0 / (2.0 * np.pi * q)


def _dot(a, b, f):
    return f(a[0] * b[0] + a[1] * b[1] + a[2] * b[2])


def tangent_frame(N, f):
    """prog.cl:205-212 as the kernel's tangent_frame states it"""
    E = f(0.001)
    yaxis = abs(N[0]) <= E and abs(N[2]) <= E
    other = N[1] if yaxis else N[0]
    rl = f(1) / np.sqrt(f(N[2] * N[2] + other * other))
    Z = np.array([f(0), -N[2] * rl, N[1] * rl], dtype=f) if yaxis else np.array([-N[2] * rl, f(0), N[0] * rl], dtype=f)
    X = np.cross(N, Z).astype(f)
    return Z, X


def cone_direction(A, q, u1, u2, f):
    A = np.asarray(A, dtype=f)
    q, u1, u2 = f(q), f(u1), f(u2)
    c = f(1) - u1 * q
    s = np.sqrt(max(f(0), f(1) - c * c))
    phi = f(2 * np.pi) * u2
    Z, X = tangent_frame(A, f)
    return (A * c + (Z * (s * np.sin(phi)) + X * (s * np.cos(phi)))).astype(f)


def sphere_q(C, R, o, f):
    c = np.asarray(C, dtype=f) - np.asarray(o, dtype=f)
    d2, R2 = _dot(c, c, f), f(R) * f(R)
    if not (np.isfinite(d2) and d2 > R2):
        return None, c, d2, R2
    s2 = R2 / d2
    cm = np.sqrt(max(f(0), f(1) - s2))
    return s2 / (f(1) + cm), c, d2, R2


def sphere_sample(C, R, o, u1, u2, f):
    """-> None (rejected) or (w, p_omega, t_s)"""
    q, c, d2, R2 = sphere_q(C, R, o, f)
    if q is None or not q > 0:
        return None
    w = cone_direction(c / np.sqrt(d2), q, u1, u2, f)
    b = _dot(c, w, f)
    return w, f(1) / (f(2 * np.pi) * q), b - np.sqrt(max(f(0), b * b - (d2 - R2)))


def sun_sample(axis, q, u1, u2, f):
    return cone_direction(axis, q, u1, u2, f), f(1) / (f(2 * np.pi) * f(q)), f(np.inf)


def sphere_hit(spheres, o, d, tmax, f):
    """spheres: [(C, R)] -> (index or -1, t, margins): margins lists, per sphere, the relative distance of each decision from its other outcome
    (outside / inside, the discriminant's sign, t against 0 and against the best so far)"""
    best, bt, margins = -1, f(tmax), []
    o, d = np.asarray(o, dtype=f), np.asarray(d, dtype=f)
    for j, (C, R) in enumerate(spheres):
        c = np.asarray(C, dtype=f) - o
        d2, b, R2 = _dot(c, c, f), _dot(c, d, f), f(R) * f(R)
        disc = b * b - (d2 - R2)
        t = b - np.sqrt(max(f(0), disc))
        margins.append((abs(d2 - R2) / R2, abs(disc) / max(b * b, R2), abs(t - bt) / max(abs(bt), abs(t)) if np.isfinite(bt) else 1.0))
        if d2 > R2 and disc >= 0 and t > 0 and t < bt:
            best, bt = j, t
    return best, bt, margins


def sun_mask(suns, d, f):
    """suns: [(axis, cos a)] -> (mask, margins |cos - cos a|)"""
    mask, margins = 0, []
    for s, (axis, ca) in enumerate(suns):
        c = _dot(np.asarray(d, dtype=f), np.asarray(axis, dtype=f), f)
        margins.append(abs(float(c) - float(ca)))
        if c >= f(ca):
            mask |= 1 << s
    return mask, margins


# ---------------------------------------------------------------------------- the path model
import glossy_ref as G          # noqa: E402
import lights_ref as L          # noqa: E402
import medium_ref as M          # noqa: E402
import nee_ref as R             # noqa: E402
import smooth_ref as S          # noqa: E402
from medium_ref import FLIGHT_MARGIN, STREAM, clip, direction, flight, hg, transmittance          # noqa: E402

AREA_KEY = 0x9e3779b9
SELECT_MARGIN = L.SELECT_MARGIN
HIT_MARGIN = 1e-4               # a sphere decision nearer than this (relative) to its other outcome is a near-tie
SUN_RIM_MARGIN = 1e-4           # ... and a direction nearer than this share of 1 - cos a to a sun's rim


class AreaLightsModel(M.MediumModel):
    """medium_ref.MediumModel (lights_ref.LightsModel plus a medium; medium = None: LightsModel itself) plus an area set, area =
    Scene.debug_area_lights(): the area branch in front of every other light sample and 1 - P_area on their p_l (_candidate), and in sample()
    the spheres as the end of a segment -- cut before the free flight -- and as blockers of every shadow ray, and the suns on a miss.
    sample() is MediumModel.sample with those statements added."""

    EVENTS = M.MediumModel.EVENTS + ("sphere_end", "sphere_end_rough", "sphere_end_scatter", "sun_miss", "area_sample", "area_glossy", "area_ng_reject",
                                     "sphere_blocks")

    def __init__(self, verts, normals, mats, mat_of, cam, lights, area, medium=None, **kw):
        super().__init__(verts, normals, mats, mat_of, cam, lights, medium, **kw)
        rec = np.asarray(area["records"], dtype=np.float64)
        ns = int(area["n_sphere"])
        self.spheres = [(rec[j, :3], rec[j, 3]) for j in range(ns)]
        self.suns = [(rec[j, :3], rec[j, 3]) for j in range(ns, len(rec))]
        self.sun_q = [rec[j, 8] for j in range(ns, len(rec))]
        self.area_L = [rec[j, 4:7] for j in range(len(rec))]
        self.area_pl = [float(p) for p in area["P_light"]]
        self.area_cdf = np.asarray(area["cdf"], dtype=np.float32)
        self.par = float(area["P_area"])
        self._aj, self._area = -1, False

    @staticmethod
    def _near(margins):
        """a sphere decision that a rounding could flip: the origin on the surface, a grazing ray, or two candidates at one distance"""
        return any(min(m) < HIT_MARGIN for m in margins)

    def _candidate(self, key, nkey, k, o, sky, tie):
        """MediumModel._candidate behind the area branch: u_area < P_area samples the set (self._aj: the sphere aimed at, whose own surface
        does not block the sample; self._area: the sample is the set's), else the other lights with p_l times 1 - P_area"""
        par = self.par
        self._aj, self._area = -1, False
        uar = R.nee_unit(R.nee_rand((key ^ AREA_KEY) & 0xFFFFFFFF, k, 0))
        tie |= abs(uar - par) < SELECT_MARGIN and 0.0 < par < 1.0
        if uar < par:
            u0 = R.nee_unit(R.nee_rand(key, k, 0))
            u1 = R.nee_unit(R.nee_rand(key, k, 1))
            u2 = R.nee_unit(R.nee_rand(key, k, 2))
            j = min(int(np.searchsorted(self.area_cdf, np.float32(u0), side="right")), len(self.area_cdf) - 1)
            self.last["area_sample"] += 1
            self._area = True
            if j < len(self.spheres):
                smp = sphere_sample(self.spheres[j][0], self.spheres[j][1], o, u1, u2, np.float64)
                self._aj = j
            else:
                s_ = j - len(self.spheres)
                smp = sun_sample(self.suns[s_][0], self.sun_q[s_], u1, u2, np.float64)
            pl = par * self.area_pl[j]
            if smp is None or not pl > 0:
                return None, tie
            return (self.area_L[j], pl * float(smp[1]), 1.0, smp[0], -1, float(smp[2]), False), tie
        cand, tie = super()._candidate(key, nkey, k, o, sky, tie)
        if cand is not None:
            cand = (cand[0], cand[1] * (1.0 - par)) + tuple(cand[2:])
        return cand, tie

    def sample(self, gid, seed, iterations, strategy):
        """one sample of pixel gid: (colour, new LCG state, near-tie seen); self.last = the sample's events"""
        ev = {k: 0 for k in self.events}
        self.last = ev
        med = self.medium
        key = int(seed) & 0xFFFFFFFF
        nkey = ~key & 0xFFFFFFFF
        mkey = key ^ STREAM
        tie = False
        seed, r1 = R.lcg(seed)
        seed, r2 = R.lcg(seed)
        P, D = self.camera_ray(gid, r1, r2)
        one = np.ones(3)
        fL, fB, fS, fR, C = one.copy(), one.copy(), one.copy(), one.copy(), np.zeros(3)
        after_lobe, Nprev, pb_prev, inside = False, None, None, False      # pb_prev: the p_b a rough or scatter vertex sampled with (None: cosine lobe)
        after_scatter = False
        sky = hasattr(self, "rgb")
        pe, pa, par = self.pe, self.pa, self.par
        nee = strategy != 0 and (len(self.lights) > 0 or sky or pa > 0 or par > 0)

        def prev_pb(Dn):
            return pb_prev if pb_prev is not None else max(0.0, float(Nprev @ Dn)) / np.pi

        def through(o, w, cut):
            """T of a light sample taken outside a dielectric"""
            if med is None or inside:
                return 1.0, False
            return transmittance(med, o, w, cut)

        def end_weight(pl, Dn):            # W_b of a path that ends on an area light whose density from the segment's origin is pl
            if not (nee and after_lobe and pl > 0):
                return 1.0
            if strategy == 1:
                return 0.0
            pb = prev_pb(Dn)
            return pb * pb / (pb * pb + pl * pl)

        def blocked(o, w, cut):            # a sphere light other than the one sampled is met before the shadow ray's cut
            others = [sp for i_, sp in enumerate(self.spheres) if i_ != self._aj]
            bj, _, bm = sphere_hit(others, o, w, cut, np.float64)
            return bj >= 0, self._near(bm)

        for k in range(iterations):
            ti, t, tt = self.intersect(P, D)
            tie |= tt
            # the nearest sphere light in front of the hit ends the segment in its place, before the free flight looks at its length
            sj, tend, marg = sphere_hit(self.spheres, P, D, t if ti >= 0 else np.inf, np.float64)
            tie |= self._near(marg)
            if med is not None and not inside:
                a, b, near = clip(med["lo"], med["hi"], P, D, tend)
                tie |= near
                ell = max(b - a, 0.0)
                if ell > 0:
                    d = flight(med["sigma_t"], R.nee_unit(R.nee_rand(mkey, k, 0)))
                    if np.isfinite(ell):
                        tie |= abs(d - ell) < FLIGHT_MARGIN * max(d, ell)
                    if d < ell:
                        ev["scatter"] += 1
                        x = P + D * (a + d)
                        fS = fS * med["albedo"]
                        if not fS.any():
                            break
                        if nee and k + 1 < iterations:
                            cand, tie = self._candidate(key, nkey, k, x, sky, tie)
                            if cand is not None:
                                Ey, pl, g, w, want, cut, delta = cand
                                hi, _, st = self.intersect(x, w, cut)
                                tie |= st
                                blk, near = blocked(x, w, cut)
                                tie |= near
                                if hi == want and not blk:
                                    T, near = through(x, w, cut)
                                    tie |= near
                                    pb = hg(med["g"], float(D @ w))
                                    wl = pb / pl if strategy == 1 or delta else pb * pl / (pb * pb + pl * pl)
                                    ev["scatter_light"] += 1
                                    ev["scatter_delta"] += int(delta)
                                    C = C + Ey * (fL + fB) * fS * fR * (g * wl) * T
                        nd, pb_prev, _ = direction(med["g"], D, R.nee_unit(R.nee_rand(mkey, k, 1)), R.nee_unit(R.nee_rand(mkey, k, 2)))
                        P, D = x, nd
                        after_lobe, Nprev, after_scatter = True, None, True
                        continue
            if sj >= 0:                        # the segment reaches the sphere light: the path ends on it
                Ls = self.area_L[sj]
                if k == 0:
                    C = C + Ls
                else:
                    q = sphere_q(self.spheres[sj][0], self.spheres[sj][1], P, np.float64)[0]
                    C = C + Ls * (fL + fB) * fS * fR * end_weight(par * self.area_pl[sj] / (2.0 * np.pi * q), D)
                ev["sphere_end"] += 1
                ev["sphere_end_rough"] += int(k > 0 and after_lobe and pb_prev is not None and not after_scatter)
                ev["sphere_end_scatter"] += int(k > 0 and after_scatter)
                break
            if ti < 0:
                mask, smarg = sun_mask(self.suns, D, np.float64)
                tie |= any(m < SUN_RIM_MARGIN * (1.0 - ca) for m, (_, ca) in zip(smarg, self.suns))
                for s_ in range(len(self.suns)):
                    if mask >> s_ & 1:
                        j_ = len(self.spheres) + s_
                        Ls = self.area_L[j_]
                        C = C + (Ls if k == 0 else Ls * (fL + fB) * fS * fR * end_weight(par * self.area_pl[j_] / (2.0 * np.pi * self.sun_q[s_]), D))
                        ev["sun_miss"] += 1
                if sky:
                    Esky, penv, edge = self.sky(D)
                    tie |= edge
                    if k == 0:
                        C = C + Esky
                    else:
                        wb = 1.0
                        pl = pe * penv * (1.0 - pa) * (1.0 - par)
                        if nee and after_lobe and pl > 0:
                            if strategy == 1:
                                wb = 0.0
                            else:
                                pb = prev_pb(D)
                                wb = pb * pb / (pb * pb + pl * pl)
                        if after_lobe and pb_prev is not None and not after_scatter:
                            ev["glossy_sky"] += 1
                        ev["scatter_sky"] += int(after_scatter)
                        C = C + Esky * (fL + fB) * fS * fR * wb
                break
            m = self._mat(ti)
            typ = int(m["type"])
            gl = typ == 4 and self.glossy
            N0 = self.n[ti].copy()
            hp = P + D * t
            Em = m["emission"][:3].astype(np.float64)
            if iterations == 1:
                C = (m["F0"][:3] if gl else m["kd"][:3]).astype(np.float64) + Em
            Ng = -N0 if D @ N0 > 0 else N0
            N, _, near = S.shading_normal(self.v[ti], N0, self.vn[ti], bool(self.has[ti]), D, hp)
            tie |= near
            if typ in (0, 3) or gl:
                inten = max(0.0, float(-D @ N))
                wb = 1.0
                parea = self.pdf_area[ti] * (1.0 - pe) * (1.0 - pa) * (1.0 - par)
                if typ == 3 and nee and after_lobe and parea > 0 and inten > 0:
                    if strategy == 1:
                        wb = 0.0
                    else:
                        pb = prev_pb(D)
                        pl = parea * t * t / inten
                        wb = pb * pb / (pb * pb + pl * pl)
                    if pb_prev is not None and wb < 1.0:
                        ev["scatter_emitter_wb" if after_scatter else "glossy_emitter_wb"] += 1
                if nee and k + 1 < iterations:
                    o = hp + Ng * 0.001
                    cand, tie = self._candidate(key, nkey, k, o, sky, tie)
                    if cand is not None:
                        Ey, pl, g, w, want, cut, delta = cand
                        cosx, cosg = float(N @ w), float(Ng @ w)
                        tie |= abs(cosx) < S.SIDE_MARGIN or abs(cosg) < S.SIDE_MARGIN
                        if cosx > 0 and not cosg > 0:
                            ev["ng_reject"] += 1
                            ev["area_ng_reject"] += int(self._area)
                            ev["delta_ng_reject"] += int(delta)
                        if cosx > 0 and cosg > 0:
                            hi, _, st = self.intersect(o, w, cut)
                            tie |= st
                            blk, near = blocked(o, w, cut)
                            tie |= near
                            ev["sphere_blocks"] += int(blk and hi == want)
                            if hi == want and not blk:
                                T, near = through(o, w, cut)
                                tie |= near
                                fs = fS
                                if gl:
                                    gv = self._glossy(m, N, D)
                                    alpha = np.array([G.roughness(m["shininess"])])
                                    wl3 = np.array([w @ gv["X"], w @ gv["Z"], w @ N])
                                    pbv, h = G.ggx_pdf_of(alpha, gv["o"][None], wl3[None])
                                    pb = float(pbv[0])
                                    F = G.schlick(m["F0"][:3].astype(np.float64)[None], h, gv["o"][None])[0]
                                    fs = fS * F * float(G.ggx_G1(alpha, wl3[None])[0])
                                    ev["glossy_light"] += 1
                                    ev["area_glossy"] += int(self._area and pb > 0)
                                    ev["delta_glossy"] += int(delta and pb > 0)
                                else:
                                    pb = cosx / np.pi
                                if pb > 0:                   # (a rough vertex with no density adds nothing)
                                    ev["delta"] += int(delta)
                                    wl = pb / pl if strategy == 1 or delta else pb * pl / (pb * pb + pl * pl)
                                    fl, fb = (self._update(m, N, hp, w, fL, fB) if typ == 0 else (fL, fB))
                                    C = C + Ey * (fl + fb) * fs * fR * (g * wl) * T
                seed, r1 = R.lcg(seed)
                seed, r2 = R.lcg(seed)
                ended = False
                if gl:
                    gv = self._glossy(m, N, D, r1, r2)
                    ev["glossy_vertex"] += 1
                    tie |= bool(gv["l2"] < G.DEGENERATE_L2) or abs(float(gv["w"][2])) < S.SIDE_MARGIN
                    nd = gv["world"] / np.linalg.norm(gv["world"])
                    fS = fS * gv["g"]
                    pb_prev = float(gv["pb"])
                    if not gv["w"][2] > 0:
                        ev["glossy_end_wz"] += 1
                        ended = True
                else:
                    nd = self.diffuse_dir(N, r1, r2)
                    pb_prev = None
                    if typ == 0:
                        fL, fB = self._update(m, N, hp, nd, fL, fB)
                    else:
                        C = C + Em * (fL + fB) * fS * fR * (inten * wb)
                P, D = hp + Ng * 0.001, nd
                after_lobe, Nprev, after_scatter = True, N, False
                below = float(nd @ Ng)
                tie |= abs(below) < S.SIDE_MARGIN
                if ended:
                    break
                if below <= 0:
                    ev["glossy_end_ng" if gl else "lobe_end"] += 1
                    break
            elif typ in (1, 2):
                rnd = 0.0
                if typ == 2:
                    seed, rnd = R.lcg(seed)
                d, refr, F, prob, near = self._spec(m, typ, N, D, inside, rnd)
                tie |= near
                g = float(d @ Ng) / np.linalg.norm(d)
                tie |= abs(g) < S.SIDE_MARGIN
                if (g >= 0) if refr else (g <= 0):
                    ev["spec_fallback"] += 1
                    d, refr, F, prob, near = self._spec(m, typ, Ng, D, inside, rnd)
                    tie |= near
                if typ == 1:
                    fS = fS * F
                elif refr:
                    fR = fR * (1.0 - F) / (1.0 - prob)
                    inside = not inside
                else:
                    fR = fR * F / prob
                P, D = hp + Ng * (-0.001 if refr else 0.001), d / np.linalg.norm(d)
                after_lobe, after_scatter = False, False
            # any other type: the ray is left unchanged and the loop hits the same surface again
        return C, seed, tie
