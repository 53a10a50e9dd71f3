"""Float64 numpy model of Scene.render_nee with analytic lights (include/pt_api.h pins the set, the selection and the estimator), built on
tests/env_ref.py's EnvModel through tests/glossy_ref.py's GlossyModel (vertex normals and the rough metal of type 4 on top of it): the same
LCG stream, the same hashes, brute-force intersection; the tables come from Scene.debug_lights(), Scene.debug_light_table() and
Scene.debug_environment().  Also the numpy statements of the cone, of the selection table and of a diffuse
floor's radiance under one light in a chosen precision (tests/test_lights_host.py, tests/test_gpu_lights.py)."""
import numpy as np

import env_ref as E
import glossy_ref as G
import nee_ref as R
import smooth_ref as S

SELECT_MARGIN = E.SELECT_MARGIN
POINT, DIRECTIONAL = 0, 1


def cone_factor(c, cos_inner, cos_outer):
    """1 inside cos_inner, 0 outside cos_outer, s^2 (3 - 2 s) between, tested in that order (-1, -1: always 1); in c's precision"""
    if c >= cos_inner:
        return c * 0 + 1
    if c <= cos_outer:
        return c * 0
    s = (c - cos_outer) / (cos_inner - cos_outer)
    return s * s * (3 - 2 * s)


def selection_table(weights):
    """(float32 cdf, P_light) of a set with these selection weights: the double-precision build of pt_set_lights and the counting rule"""
    w = np.asarray(weights, dtype=np.float64)
    n = len(w)
    if not (w.sum() > 0):
        return np.ones(n, dtype=np.float32), np.zeros(n)
    cdf = (np.cumsum(w) / w.sum()).astype(np.float32)
    cdf[int(np.nonzero(w > 0)[0][-1]):] = 1.0
    return cdf, R.selection_probs(cdf)


def parse_records(rec):
    """Scene.debug_lights()["records"] (n, 16) -> list of dicts in float64"""
    rec = np.asarray(rec, dtype=np.float32).reshape(-1, 16)
    out = []
    for r in rec:
        out.append(dict(type=int(r[3:4].view(np.int32)[0]), position=r[0:3].astype(np.float64), axis=r[4:7].astype(np.float64),
                        cos_inner=float(r[7]), intensity=r[8:11].astype(np.float64), cos_outer=float(r[11]), P_light=float(r[12])))
    return out


def light_sample(light, o, dtype=np.float64):
    """The sample of `light` seen from o, in `dtype`: None if rejected, else (w, cut, intensity x cone / d)"""
    f = dtype
    o = np.asarray(o, dtype=f)
    axis = light["axis"].astype(f)
    if light["type"] == DIRECTIONAL:
        w, d, cut = -axis, f(1), np.inf
    else:
        dv = light["position"].astype(f) - o
        d = (dv * dv).sum(dtype=f)
        if not (d > 0 and np.isfinite(d)):
            return None
        r = np.sqrt(d)
        w, cut = dv / r, float(r)
    cone = cone_factor((-w * axis).sum(dtype=f), f(light["cos_inner"]), f(light["cos_outer"]))
    if not cone > 0:
        return None
    return w, cut, light["intensity"].astype(f) * (cone / d)


def floor_radiance(kd, light, hp, N, dtype=np.float64):
    """What one light sample adds at a diffuse vertex hp (normal N, albedo kd, all factors 1) with P_ana = P_light = 1, in `dtype`:
    kd cos x (intensity cone / d) x (cos / pi) / 1 -- the closed forms of tests/test_gpu_lights.py"""
    f = dtype
    hp, N = np.asarray(hp, dtype=f), np.asarray(N, dtype=f)
    s = light_sample(light, hp + N * f(0.001), f)
    if s is None:
        return np.zeros(3, dtype=f)
    w, _, e = s
    cosx = (N * w).sum(dtype=f)
    if not cosx > 0:
        return np.zeros(3, dtype=f)
    pb = cosx * f(1.0 / np.pi)
    return (e * (f(kd) * cosx)) * pb


class LightsModel(G.GlossyModel):
    """glossy_ref.GlossyModel (material types 0-4, vertex normals, with or without an environment) plus a light set: lights =
    Scene.debug_lights(); vnormals = None: no triangle has vertex normals; env as smooth_ref.SmoothModel takes it.  sample() is
    GlossyModel.sample with the analytic branch in front of the sky / triangle one and 1 - P_ana on the latter's p_l."""

    EVENTS = G.GlossyModel.EVENTS + ("delta", "delta_glossy", "delta_ng_reject")

    def __init__(self, verts, normals, mats, mat_of, cam, lights, vnormals=None, env=None, table=None, margin=1e-4, glossy=True):
        if vnormals is None:
            vnormals = np.zeros(np.asarray(verts).shape, dtype=np.float32)
        super().__init__(verts, normals, mats, mat_of, cam, vnormals, env=env, table=table, margin=margin, glossy=glossy)
        self.set = parse_records(lights["records"])
        self.set_cdf = np.asarray(lights["cdf"], dtype=np.float32)
        self.pa = float(lights["P_ana"])

    def sample(self, gid, seed, iterations, strategy):
        """one sample of pixel gid: (colour, new LCG state, near-tie seen); self.last = the sample's events"""
        ev = {k: 0 for k in self.events}
        self.last = ev
        key = int(seed) & 0xFFFFFFFF
        nkey = ~key & 0xFFFFFFFF
        tie = False
        seed, r1 = R.lcg(seed)
        seed, r2 = R.lcg(seed)
        P, D = self.camera_ray(gid, r1, r2)
        one = np.ones(3)
        fL, fB, fS, fR, C = one.copy(), one.copy(), one.copy(), one.copy(), np.zeros(3)
        after_lobe, Nprev, pb_prev, inside = False, None, None, False      # pb_prev: the p_b a glossy vertex sampled with (None: cosine lobe)
        sky = hasattr(self, "rgb")
        nee = strategy != 0
        pe, pa = self.pe, self.pa

        def prev_pb(Dn):
            return pb_prev if pb_prev is not None else max(0.0, float(Nprev @ Dn)) / np.pi

        for k in range(iterations):
            ti, t, tt = self.intersect(P, D)
            tie |= tt
            if ti < 0:
                if sky:
                    Esky, penv, edge = self.sky(D)
                    tie |= edge
                    if k == 0:
                        C = C + Esky
                    else:
                        wb = 1.0
                        pl = pe * penv * (1.0 - pa)
                        if nee and after_lobe and pl > 0:
                            if strategy == 1:
                                wb = 0.0
                            else:
                                pb = prev_pb(D)
                                wb = pb * pb / (pb * pb + pl * pl)
                        if after_lobe and pb_prev is not None:
                            ev["glossy_sky"] += 1
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
                parea = self.pdf_area[ti] * (1.0 - pe) * (1.0 - pa)
                if typ == 3 and nee and after_lobe and parea > 0 and inten > 0:
                    if strategy == 1:
                        wb = 0.0
                    else:
                        pb = prev_pb(D)
                        pl = parea * t * t / inten
                        wb = pb * pb / (pb * pb + pl * pl)
                    if pb_prev is not None and wb < 1.0:
                        ev["glossy_emitter_wb"] += 1
                if nee and k + 1 < iterations:
                    u0 = R.nee_unit(R.nee_rand(key, k, 0))
                    u1 = R.nee_unit(R.nee_rand(key, k, 1))
                    u2 = R.nee_unit(R.nee_rand(key, k, 2))
                    ua = R.nee_unit(R.nee_rand(nkey, k, 2))
                    tie |= abs(ua - pa) < SELECT_MARGIN and 0.0 < pa < 1.0
                    o = hp + Ng * 0.001
                    cand = None                      # (E, p_l, emitter cosine, w, what the shadow ray must return, its cut, delta)
                    if ua < pa:
                        j = min(int(np.searchsorted(self.set_cdf, np.float32(u0), side="right")), len(self.set_cdf) - 1)
                        smp = light_sample(self.set[j], o)
                        pl = pa * self.set[j]["P_light"]
                        if smp is not None and pl > 0:
                            cand = (smp[2], pl, 1.0, smp[0], -1, smp[1], True)
                    else:
                        use_sky = False
                        if sky:
                            us = R.nee_unit(R.nee_rand(nkey, k, 0))
                            tie |= abs(us - pe) < SELECT_MARGIN and 0.0 < pe < 1.0
                            use_sky = us < pe
                        if use_sky:
                            w, Ey, penv = self.sky_sample(u1, u2)
                            pl = pe * penv * (1.0 - pa)
                            if pl > 0:
                                cand = (Ey, pl, 1.0, w, -1, np.inf, False)
                        elif len(self.lights):
                            j = min(int(np.searchsorted(self.cdf, np.float32(u0), side="right")), len(self.cdf) - 1)
                            li = int(self.lights[j])
                            v = self.v[li]
                            su = np.sqrt(u1)
                            y = v[0] + (v[1] - v[0]) * (u2 * su) + (v[2] - v[0]) * (su * (1.0 - u2))
                            d = y - o
                            r = np.linalg.norm(d)
                            w = d / r
                            cosy = abs(float(w @ self.n[li]))
                            if cosy > 0:
                                pl = self.pdf_area[li] * (1.0 - pe) * (1.0 - pa) * r * r / cosy
                                if pl > 0:
                                    cand = (self._mat(li)["emission"][:3].astype(np.float64), pl, cosy, w, li, r * R.SHADOW_CUT, False)
                    if cand is not None:
                        Ey, pl, g, w, want, cut, delta = cand
                        cosx, cosg = float(N @ w), float(Ng @ w)
                        tie |= abs(cosx) < S.SIDE_MARGIN or abs(cosg) < S.SIDE_MARGIN
                        if cosx > 0 and not cosg > 0:
                            ev["ng_reject"] += 1
                            ev["delta_ng_reject"] += int(delta)
                        if cosx > 0 and cosg > 0:
                            hi, _, st = self.intersect(o, w, cut)
                            tie |= st
                            if hi == want:
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
                                    ev["delta_glossy"] += int(delta and pb > 0)
                                else:
                                    pb = cosx / np.pi
                                if pb > 0:                   # (a rough vertex with no density adds nothing)
                                    ev["delta"] += int(delta)
                                    wl = pb / pl if strategy == 1 or delta else pb * pl / (pb * pb + pl * pl)
                                    fl, fb = (self._update(m, N, hp, w, fL, fB) if typ == 0 else (fL, fB))
                                    C = C + Ey * (fl + fb) * fs * fR * (g * wl)
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
                after_lobe, Nprev = True, N
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
                after_lobe = False
            # any other type: the ray is left unchanged and the loop hits the same surface again
        return C, seed, tie
