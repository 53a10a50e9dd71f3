"""Float64 numpy model of Scene.render_nee under option frosted (include/pt_api.h pins the vertex), on top of tests/coated_ref.py: the
CoatedModel with material type 6 shaded as a rough dielectric (GGX reflection and refraction through one visible-normal half vector) and
the `inside` flag it toggles.  It shares no code with the library.  vertex() is the frosted vertex itself, vectorised and in a chosen
precision: float64 is the reference, float32 the restatement of the pinned sequence that the tests measure their tolerances with."""
import numpy as np

import coated_ref as K
import glossy_ref as G
import nee_ref as R
import smooth_ref as S


def terms(F0, eta, o, h):
    """(c, F, disc, Fm, tir) at half vectors h: Schlick, type 2's discriminant, the mean; total internal reflection makes F and Fm 1"""
    t = o.dtype.type
    c = G.dot(o, h)
    F = G.schlick(F0, h, o)
    disc = 1 - ((1 - c * c) / eta) / eta
    Fm = ((F[:, 0] + F[:, 1]) + F[:, 2]) / t(3)
    tir = disc <= 0
    Fm = np.where(tir, t(1), Fm).astype(o.dtype)
    F = np.where(tir[:, None], t(1), F).astype(o.dtype)
    return c, F, disc, Fm, tir


def mirrored(w):
    return np.stack([w[:, 0], w[:, 1], -w[:, 2]], 1)


def reflect_terms(alpha, F0, eta, o, h, w):
    """(p_b, g) of reflected directions w with half vectors h"""
    c, F, disc, Fm, _ = terms(F0, eta, o, h)
    pb = Fm * G.ggx_pdf(alpha, o, h)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = F * (G.ggx_G1(alpha, w) / Fm)[:, None]
    return pb.astype(o.dtype), g.astype(o.dtype)


def refract_half(eta, o, w):
    """the half vector (h.z >= 0) that refracts o into w, and whether the pair is one: o.h > 0 > w.h"""
    h = G.unit(o + w * np.reshape(eta, (-1, 1)))
    h = np.where((h[:, 2] < 0)[:, None], -h, h)
    return h, (G.dot(o, h) > 0) & (G.dot(w, h) < 0)


def refract_density(alpha, F0, eta, o, w):
    """the density of refracted directions w (w.z < 0), which only the model needs: (1 - Fm) G1(o) D(h) (o.h) / o.z x
    eta^2 |w.h| / (o.h + eta w.h)^2; and the weight g(w) = (1 - F) G1(w mirrored) / (1 - Fm)"""
    h, ok = refract_half(eta, o, w)
    c, F, disc, Fm, tir = terms(F0, eta, o, h)
    wh = G.dot(w, h)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = (1 - Fm) * G.ggx_G1(alpha, o) * G.ggx_D(alpha, h) * c / o[:, 2] * eta * eta * np.abs(wh) / (c + eta * wh) ** 2
        g = (1 - F) * (G.ggx_G1(alpha, mirrored(w)) / (1 - Fm))[:, None]
    ok = ok & ~tir & (w[:, 2] < 0) & (o[:, 2] > 0)
    return np.where(ok, p, 0.0), np.where(ok[:, None], g, 0.0)


def evaluate_of(alpha, F0, eta, o, w):
    """(p, g) of given unit directions w in both hemispheres: above the surface the reflection lobe the way a light sample evaluates it
    (h = normalize(o + w) and the terms from scratch), below it the refraction lobe's density and weight"""
    up = w[:, 2] > 0
    wu = np.where(up[:, None], w, mirrored(w))
    pr, gr = reflect_terms(alpha, F0, eta, o, G.unit(o + wu), wu)
    pt, gt = refract_density(alpha, F0, eta, o, np.where(up[:, None], mirrored(w), w))
    return np.where(up, pr, pt), np.where(up[:, None], gr, gt)


def vertex(N, D, alpha, F0, eta, rnd1, rnd2, u_sel, dtype=np.float64):
    """The sampled vertex for n items: N, D (n, 3), alpha, eta, rnd1, rnd2, u_sel (n,), F0 (n, 3) or (3,), all first rounded to float32 (the
    values the device gets) and then evaluated in `dtype`.  Returns a dict of arrays."""
    f = lambda a: np.asarray(a, dtype=np.float32).astype(dtype)
    N, D, alpha, eta, rnd1, rnd2, u_sel = f(N), f(D), f(alpha), f(eta), f(rnd1), f(rnd2), f(u_sel)
    F0 = np.broadcast_to(f(F0), N.shape)
    gv = G.vertex(N, D, alpha, rnd1, rnd2, F0, dtype=dtype)       # the half vector: visible normals on the disc point of rnd1, rnd2
    X, Z, o, h = gv["X"], gv["Z"], gv["o"], gv["h"]
    c, F, disc, Fm, tir = terms(F0, eta, o, h)
    refl = u_sel < Fm
    with np.errstate(invalid="ignore"):
        wt = h * (c / eta - np.sqrt(np.where(disc > 0, disc, 0)))[:, None] - o / eta[:, None]
    w = np.where(refl[:, None], gv["w"], wt)
    world = X * w[:, 0:1] + N * w[:, 2:3] + Z * w[:, 1:2]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(refl[:, None], F * (G.ggx_G1(alpha, w) / Fm)[:, None], (1 - F) * (G.ggx_G1(alpha, mirrored(w)) / (1 - Fm))[:, None]).astype(dtype)
    pb = np.where(refl, Fm * G.ggx_pdf(alpha, o, h), 0).astype(dtype)
    wl = G.local(G.unit(world), X, Z, N)
    pb2, g2 = reflect_terms(alpha, F0, eta, o, G.unit(o + wl), wl)
    pb_again = np.where(refl, pb2, 0).astype(dtype)
    g_again = np.where(refl[:, None], g2, 0).astype(dtype)
    return dict(world=world, w=w, h=h, o=o, Fm=Fm, refl=refl, pb=pb, g=g, pb_again=pb_again, g_again=g_again, l2=gv["l2"], X=X, Z=Z, c=c, disc=disc,
                tir=tir)


def debug_columns(v):
    """vertex()'s result in the layout of pt_debug_frosted: (n, 10)"""
    return np.concatenate([v["world"], v["Fm"][:, None], v["refl"].astype(v["world"].dtype)[:, None], v["pb"][:, None], v["g"][:, 0:1], v["pb_again"][:, None],
                           v["g_again"][:, 0:1], v["o"][:, 2:3]], 1)


COLUMNS = ("direction", "Fm", "p_b sampled", "g.x sampled", "p_b again", "g.x again", "o.z")
COLUMN_INDEX = (3, 5, 6, 7, 8, 9)      # where COLUMNS[1:] sit in the layout of pt_debug_frosted
column_errors = K.column_errors        # (the same layout: direction, a scalar, the lobe flag, four values, o.z)


class FrostedModel(K.CoatedModel):
    """coated_ref.CoatedModel with material type 6 shaded as the rough dielectric (frosted = False: inert, as without the option) and the
    `inside` flag a refraction toggles.  fm_margin: a lobe choice whose |u_sel - Fm|, or a discriminant whose |disc|, is below it is a
    near tie (the float32 restatement's error of them)."""

    FROSTED_EVENTS = ("frosted_reflect", "frosted_refract", "frosted_tir", "frosted_inside", "frosted_end_wz", "frosted_end_ng", "frosted_light",
                      "frosted_emitter_wb", "frosted_sky", "frosted_through_emitter", "frosted_through_sky")

    def __init__(self, *a, frosted=True, fm_margin=1e-5, **k):
        super().__init__(*a, **k)
        self.frosted = frosted
        self.fm_margin = fm_margin
        self.events.update({e: 0 for e in self.FROSTED_EVENTS})

    def _frosted(self, m, N, D, inside, r1=0.0, r2=0.0, us=0.0):
        n = float(m["n"])
        eta = float(np.float32(1.0) / np.float32(n)) if inside else n
        v = vertex(N[None], D[None], [G.roughness(m["shininess"])], m["F0"][:3], [eta], [r1], [r2], [us])
        out = {k: x[0] for k, x in v.items()}
        out["eta"] = float(np.float32(eta))
        return out

    def sample(self, gid, seed, iterations, strategy):
        ev = {k: 0 for k in self.events}
        self.last = ev
        key = int(seed) & 0xFFFFFFFF
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
                        inside = not inside
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
                    inside = not inside
                else:
                    fR = fR * F / prob
                P, D = hp + Ng * (-0.001 if refr else 0.001), d / np.linalg.norm(d)
                after_lobe, through = False, False
            # any other type: the ray is left unchanged and the loop hits the same surface again
        return C, seed, tie
