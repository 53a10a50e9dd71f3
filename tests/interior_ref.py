"""Float64 numpy model of Scene.render_nee with interiors bound to glass (include/pt_api.h pins the free flight, the absorption factor and
the scatter vertex): tests/medium_ref.py's MediumModel -- its own estimator, restated statement for statement,
the same LCG stream, hashes, selection rules and brute-force intersection -- with the interior rule added where `inside` is true.  Also
the float64 statements of the pieces that tests/test_interior_host.py checks against a brute-force integration and
tests/test_gpu_interior.py holds pt_debug_interior to.  MediumModel shades types 0 to 4, so a bound material of InteriorModel is of
type 2; InteriorFrostedModel adds the same rule to tests/frosted_ref.py's FrostedModel for a type-6 boundary."""
import numpy as np

import coated_ref as K
import frosted_ref as F
import glossy_ref as G
import lights_ref as L
import medium_ref as M
import nee_ref as R
import smooth_ref as S
from frosted_ref import reflect_terms, terms
from medium_ref import FLIGHT_MARGIN, STREAM, clip, direction, flight, hg, transmittance


def interior_of(d):
    """Scene.material_interior() -> the model's record in float64"""
    return dict(sigma_a=np.asarray(d["sigma_a"], dtype=np.float64), sigma_s=float(d["sigma_s"]), g=float(d["g"]))


def absorb(sigma_a, ell):
    """Beer-Lambert per channel over the length ell"""
    return np.exp(-np.asarray(sigma_a, dtype=np.float64) * ell)


def segment(it, t, u):
    """the interior rule on one segment whose hit is at t, u the free-flight number: (scatters, l, absorption factor)"""
    ell, sc = float(t), False
    if it["sigma_s"] > 0:
        d = flight(it["sigma_s"], u)
        if d < t:
            ell, sc = d, True
    return sc, ell, absorb(it["sigma_a"], ell)


class InteriorModel(M.MediumModel):
    """medium_ref.MediumModel plus interiors = {material index: Scene.material_interior(index)} (a binding on a material that is not of
    type 2 is ignored, as the device table ignores it).  sample() is MediumModel.sample with the interior rule at the top of a segment
    that runs inside a dielectric: with no binding, or an all-zero one, it is MediumModel's sample for sample."""

    EVENTS = M.MediumModel.EVENTS + ("interior_scatter", "interior_absorbed", "interior_exit", "interior_then_light")

    def __init__(self, verts, normals, mats, mat_of, cam, lights, medium, interiors, vnormals=None, env=None, table=None, margin=1e-4, glossy=True):
        super().__init__(verts, normals, mats, mat_of, cam, lights, medium, vnormals=vnormals, env=env, table=table, margin=margin, glossy=glossy)
        self.interiors = {int(k): interior_of(v) for k, v in (interiors or {}).items() if v is not None}
        self.mat_of = np.asarray(mat_of)
        self.events.update({e: 0 for e in self.EVENTS})

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
        scattered_inside, ever_scattered = False, False      # an interior scatter since the path entered / anywhere on the path
        sky = hasattr(self, "rgb")
        pe, pa = self.pe, self.pa
        nee = strategy != 0 and (len(self.lights) > 0 or sky or pa > 0)

        def prev_pb(Dn):
            return pb_prev if pb_prev is not None else max(0.0, float(Nprev @ Dn)) / np.pi

        def through(o, w, cut):
            """T of a light sample taken outside a dielectric"""
            if med is None or inside:
                return 1.0, False
            return transmittance(med, o, w, cut)

        for k in range(iterations):
            ti, t, tt = self.intersect(P, D)
            tie |= tt
            if inside and ti >= 0:
                it = self.interiors.get(int(self.mat_of[ti]))
                if it is not None and int(self._mat(ti)["type"]) in (2, 6):
                    ell, sc = float(t), False
                    if it["sigma_s"] > 0:
                        d = flight(it["sigma_s"], R.nee_unit(R.nee_rand(mkey, k, 0)))
                        tie |= abs(d - t) < FLIGHT_MARGIN * max(d, t)
                        if d < t:
                            ell, sc = d, True
                    fS = fS * np.exp(-it["sigma_a"] * ell)
                    if not fS.any():
                        break
                    if sc:
                        ev["interior_scatter"] += 1
                        scattered_inside, ever_scattered = True, True
                        nd, _, _ = direction(it["g"], D, R.nee_unit(R.nee_rand(mkey, k, 1)), R.nee_unit(R.nee_rand(mkey, k, 2)))
                        P, D = P + D * d, nd
                        after_lobe, Nprev, pb_prev, after_scatter = False, None, None, False
                        continue
                    ev["interior_absorbed"] += int(it["sigma_a"].any())
            if med is not None and not inside:
                a, b, near = clip(med["lo"], med["hi"], P, D, t if ti >= 0 else np.inf)
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
                                if hi == want:
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
                        if after_lobe and pb_prev is not None and not after_scatter:
                            ev["glossy_sky"] += 1
                        ev["scatter_sky"] += int(after_scatter)
                        ev["interior_then_light"] += int(ever_scattered)
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
                            ev["delta_ng_reject"] += int(delta)
                        if cosx > 0 and cosg > 0:
                            hi, _, st = self.intersect(o, w, cut)
                            tie |= st
                            if hi == want:
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
                        ev["interior_then_light"] += int(ever_scattered and bool(Em.any()) and inten * wb > 0)
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
                    ev["interior_exit"] += int(inside and scattered_inside)
                    inside = not inside
                    scattered_inside = False
                else:
                    fR = fR * F / prob
                P, D = hp + Ng * (-0.001 if refr else 0.001), d / np.linalg.norm(d)
                after_lobe, after_scatter = False, False
            # any other type: the ray is left unchanged and the loop hits the same surface again
        return C, seed, tie


INTERIOR_EVENTS = ("interior_scatter", "interior_absorbed", "interior_exit", "interior_then_light")


class InteriorFrostedModel(F.FrostedModel):
    """frosted_ref.FrostedModel (types 0 to 6, emitters and a sky, no analytic lights and no medium) plus interiors, for a type-6 boundary
    under option frosted: FrostedModel.sample restated statement for statement with the same interior rule at the top of a segment that
    runs inside a dielectric.  A binding counts on a material of type 2 or 6 by its type alone, as the device table reads it
    (with `frosted` off a type-6 surface is inert, but a segment inside type-2 glass that ends on it still takes its interior)."""

    def __init__(self, *a, interiors=None, **k):
        super().__init__(*a, **k)
        self.interiors = {int(m): interior_of(v) for m, v in (interiors or {}).items() if v is not None}
        self.events.update({e: 0 for e in INTERIOR_EVENTS})

    def sample(self, gid, seed, iterations, strategy):
        ev = {k: 0 for k in self.events}
        self.last = ev
        key = int(seed) & 0xFFFFFFFF
        mkey = key ^ STREAM
        tie = False
        seed, r1 = R.lcg(seed)
        seed, r2 = R.lcg(seed)
        P, D = self.camera_ray(gid, r1, r2)
        one = np.ones(3)
        fL, fB, fS, fR, C = one.copy(), one.copy(), one.copy(), one.copy(), np.zeros(3)
        # pb_prev: the p_b a glossy, coated or frosted vertex sampled with (None: cosine lobe); prev: its kind or None; through: the
        # previous vertex refracted (after_lobe is False then)
        after_lobe, Nprev, pb_prev, prev, inside, through = False, None, None, None, False, False
        sky = hasattr(self, "rgb")
        nee = strategy != 0 and (len(self.lights) > 0 or self.has_dist)
        pe = self.pe
        scattered_inside, ever_scattered = False, False      # an interior scatter since the path entered / anywhere on the path

        def prev_pb(Dn):
            return pb_prev if pb_prev is not None else max(0.0, float(Nprev @ Dn)) / np.pi

        for k in range(iterations):
            ti, t, tt = self.intersect(P, D)
            tie |= tt
            if inside and ti >= 0:
                it = self.interiors.get(int(self.mat_of[ti]))
                bt = int(self._mat(ti)["type"])
                if it is not None and bt in (2, 6):          # (the type alone, as the device table: not option frosted)
                    ell, sc = float(t), False
                    if it["sigma_s"] > 0:
                        d = flight(it["sigma_s"], R.nee_unit(R.nee_rand(mkey, k, 0)))
                        tie |= abs(d - t) < FLIGHT_MARGIN * max(d, t)
                        if d < t:
                            ell, sc = d, True
                    fS = fS * np.exp(-it["sigma_a"] * ell)
                    if not fS.any():
                        break
                    if sc:
                        ev["interior_scatter"] += 1
                        scattered_inside, ever_scattered = True, True
                        nd, _, _ = direction(it["g"], D, R.nee_unit(R.nee_rand(mkey, k, 1)), R.nee_unit(R.nee_rand(mkey, k, 2)))
                        P, D = P + D * d, nd
                        after_lobe, Nprev, pb_prev, prev, through = False, None, None, None, False
                        continue
                    ev["interior_absorbed"] += int(it["sigma_a"].any())
            if ti < 0:
                if sky:
                    Esky, penv, edge = self.sky(D)
                    tie |= edge
                    if k == 0:
                        C = C + Esky
                    else:
                        wb = 1.0
                        pl = pe * penv
                        if nee and after_lobe and pl > 0:
                            if strategy == 1:
                                wb = 0.0
                            else:
                                pb = prev_pb(D)
                                wb = pb * pb / (pb * pb + pl * pl)
                        if after_lobe and prev is not None:
                            ev[prev + "_sky"] += 1
                        if through:
                            ev["frosted_through_sky"] += 1
                        C = C + Esky * (fL + fB) * fS * fR * wb
                        ev["interior_then_light"] += int(ever_scattered)
                break
            m = self._mat(ti)
            typ = int(m["type"])
            gl = typ == 4 and self.glossy
            ct = typ == 5 and self.coated
            fr = typ == 6 and self.frosted
            N0 = self.n[ti].copy()
            hp = P + D * t
            Em = m["emission"][:3].astype(np.float64)
            if iterations == 1:
                C = (m["F0"][:3] if gl else m["kd"][:3]).astype(np.float64) + Em
            Ng = -N0 if D @ N0 > 0 else N0
            N, _, near = S.shading_normal(self.v[ti], N0, self.vn[ti], bool(self.has[ti]), D, hp)
            tie |= near
            if typ in (0, 3) or gl or ct or fr:
                inten = max(0.0, float(-D @ N))
                wb = 1.0
                pa = self.pdf_area[ti] * (1.0 - pe)
                if typ == 3 and through:
                    ev["frosted_through_emitter"] += 1
                if typ == 3 and nee and after_lobe and pa > 0 and inten > 0:
                    if strategy == 1:
                        wb = 0.0
                    else:
                        pb = prev_pb(D)
                        pl = pa * t * t / inten
                        wb = pb * pb / (pb * pb + pl * pl)
                    if prev is not None and wb < 1.0:
                        ev[prev + "_emitter_wb"] += 1
                if nee and k + 1 < iterations:
                    u0 = R.nee_unit(R.nee_rand(key, k, 0))
                    u1 = R.nee_unit(R.nee_rand(key, k, 1))
                    u2 = R.nee_unit(R.nee_rand(key, k, 2))
                    o = hp + Ng * 0.001
                    cand = None
                    use_sky = False
                    if sky:
                        us = R.nee_unit(R.nee_rand(~key & 0xFFFFFFFF, k, 0))
                        tie |= abs(us - pe) < S.E.SELECT_MARGIN and 0.0 < pe < 1.0
                        use_sky = us < pe
                    if use_sky:
                        w, Ey, penv = self.sky_sample(u1, u2)
                        if pe * penv > 0:
                            cand = (Ey, pe * penv, 1.0, w, -1, np.inf)
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
                            pl = self.pdf_area[li] * (1.0 - pe) * r * r / cosy
                            if pl > 0:
                                cand = (self._mat(li)["emission"][:3].astype(np.float64), pl, cosy, w, li, r * R.SHADOW_CUT)
                    if cand is not None:
                        Ey, pl, g, w, want, cut = cand
                        cosx, cosg = float(N @ w), float(Ng @ w)
                        tie |= abs(cosx) < S.SIDE_MARGIN or abs(cosg) < S.SIDE_MARGIN
                        if cosx > 0 and not cosg > 0:
                            ev["ng_reject"] += 1
                        if cosx > 0 and cosg > 0:
                            hi, _, st = self.intersect(o, w, cut)
                            tie |= st
                            if hi == want:
                                fs, frr = fS, fR
                                if gl:
                                    gv = self._glossy(m, N, D)
                                    wl3 = np.array([w @ gv["X"], w @ gv["Z"], w @ N])
                                    al = np.array([G.roughness(m["shininess"])])
                                    pbv, h = G.ggx_pdf_of(al, gv["o"][None], wl3[None])
                                    pb = float(pbv[0])
                                    F = G.schlick(m["F0"][:3].astype(np.float64)[None], h, gv["o"][None])[0]
                                    fs = fS * F * float(G.ggx_G1(al, wl3[None])[0])
                                    ev["glossy_light"] += 1
                                elif ct:
                                    cv = self._coated(m, N, D)
                                    wl3 = np.array([w @ cv["X"], w @ cv["Z"], w @ N])
                                    al = np.array([G.roughness(m["shininess"])])
                                    pbv, gg, _, _ = K.evaluate_of(al, m["F0"][:3].astype(np.float64)[None], m["kd"][:3].astype(np.float64)[None], cv["o"][None], wl3[None])
                                    pb = float(pbv[0])
                                    fs = fS * gg[0]
                                    ev["coated_light"] += 1
                                elif fr:
                                    fv = self._frosted(m, N, D, inside)
                                    wl3 = np.array([w @ fv["X"], w @ fv["Z"], w @ N])
                                    al = np.array([G.roughness(m["shininess"])])
                                    oo = fv["o"][None]
                                    hh = G.unit(oo + wl3[None])
                                    et = np.array([fv["eta"]])
                                    pbv, gg = reflect_terms(al, m["F0"][:3].astype(np.float64)[None], et, oo, hh, wl3[None])
                                    _, _, dd, _, _ = terms(m["F0"][:3].astype(np.float64)[None], et, oo, hh)
                                    tie |= abs(float(dd[0])) < self.fm_margin
                                    pb = float(pbv[0])
                                    frr = fR * gg[0]
                                    ev["frosted_light"] += 1
                                else:
                                    pb = cosx / np.pi
                                if pb > 0:
                                    wl = pb / pl if strategy == 1 else pb * pl / (pb * pb + pl * pl)
                                    fl, fb = (self._update(m, N, hp, w, fL, fB) if typ == 0 else (fL, fB))
                                    C = C + Ey * (fl + fb) * fs * frr * (g * wl)
                seed, r1 = R.lcg(seed)
                seed, r2 = R.lcg(seed)
                ended = False
                refr = False
                if gl:
                    gv = self._glossy(m, N, D, r1, r2)
                    ev["glossy_vertex"] += 1
                    tie |= bool(gv["l2"] < G.DEGENERATE_L2) or abs(float(gv["w"][2])) < S.SIDE_MARGIN
                    nd = gv["world"] / np.linalg.norm(gv["world"])
                    fS = fS * gv["g"]
                    pb_prev, prev = float(gv["pb"]), "glossy"
                    if not gv["w"][2] > 0:
                        ev["glossy_end_wz"] += 1
                        ended = True
                elif ct:
                    us = R.nee_unit(R.nee_rand(~key & 0xFFFFFFFF, k, 1))
                    cv = self._coated(m, N, D, r1, r2, us)
                    tie |= abs(us - float(cv["ps"])) < self.ps_margin
                    ev["coated_coat" if cv["coat"] else "coated_base"] += 1
                    tie |= (bool(cv["coat"]) and bool(cv["l2"] < G.DEGENERATE_L2)) or abs(float(cv["w"][2])) < S.SIDE_MARGIN
                    nd = cv["world"] / np.linalg.norm(cv["world"])
                    fS = fS * cv["g"]
                    pb_prev, prev = float(cv["pb"]), "coated"
                    if not (cv["w"][2] > 0 and cv["pb"] > 0):
                        ev["coated_end_wz"] += 1
                        ended = True
                elif fr:
                    us = R.nee_unit(R.nee_rand(~key & 0xFFFFFFFF, k, 1))
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
                    pb_prev, prev = float(fv["pb"]), "frosted"
                    if refr:
                        ev["interior_exit"] += int(inside and scattered_inside)
                        inside = not inside
                        scattered_inside = False
                    if not (fv["w"][2] < 0 if refr else fv["w"][2] > 0):
                        ev["frosted_end_wz"] += 1
                        ended = True
                else:
                    nd = self.diffuse_dir(N, r1, r2)
                    pb_prev, prev = None, None
                    if typ == 0:
                        fL, fB = self._update(m, N, hp, nd, fL, fB)
                    else:
                        C = C + Em * (fL + fB) * fS * fR * (inten * wb)
                        ev["interior_then_light"] += int(ever_scattered and bool(Em.any()) and inten * wb > 0)
                P, D = hp + Ng * (-0.001 if refr else 0.001), nd
                after_lobe, Nprev, through = not refr, N, refr
                if refr:
                    pb_prev, prev = None, None
                below = float(nd @ Ng)
                tie |= abs(below) < S.SIDE_MARGIN
                if ended:
                    break
                if (below >= 0) if refr else (below <= 0):
                    ev["glossy_end_ng" if gl else "coated_end_ng" if ct else "frosted_end_ng" if fr else "lobe_end"] += 1
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
                    ev["interior_exit"] += int(inside and scattered_inside)
                    inside = not inside
                    scattered_inside = False
                else:
                    fR = fR * F / prob
                P, D = hp + Ng * (-0.001 if refr else 0.001), d / np.linalg.norm(d)
                after_lobe, through = False, False
            # any other type: the ray is left unchanged and the loop hits the same surface again
        return C, seed, tie
