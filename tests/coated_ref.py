"""Float64 numpy model of Scene.render_nee under option coated (include/pt_api.h pins the vertex), on top of tests/glossy_ref.py: the
GlossyModel with material type 5 shaded as a diffuse base under a rough dielectric coat.  It shares no code with the library.  vertex()
is the coated vertex itself, vectorised and in a chosen precision: float64 is the reference, float32 the restatement of the pinned
sequence that the tests measure their tolerances with."""
import numpy as np

import glossy_ref as G
import nee_ref as R
import smooth_ref as S


def schlick_c(F0, c):
    """F(c): Schlick on |c|, F0 (n, 3), c (n,)"""
    return F0 + (1 - F0) * ((1 - np.abs(c)) ** 5)[:, None]


def lobe_probability(F0, kd, oz):
    """ps: the probability of the coat lobe"""
    Fo = schlick_c(F0, oz)
    three = oz.dtype.type(3)
    fm = ((Fo[:, 0] + Fo[:, 1]) + Fo[:, 2]) / three
    km = ((kd[:, 0] + kd[:, 1]) + kd[:, 2]) / three
    s = (1 - fm) * km + fm
    with np.errstate(divide="ignore", invalid="ignore"):
        ps = np.where(s > 0, fm / np.where(s > 0, s, 1), oz.dtype.type(0.5))
    return np.clip(ps, oz.dtype.type(0.1), oz.dtype.type(0.9)).astype(oz.dtype)


def evaluate(alpha, F0, kd, ps, o, h, w):
    """(p_b, g, spec, diff) of local directions w (n, 3) with half vectors h: the mixture density and the weight (spec + diff) / p_b"""
    t = o.dtype.type
    pg = G.ggx_pdf(alpha, o, h)
    c = np.maximum(w[:, 2], 0)
    pb = ps * pg + ((1 - ps) * c) * t(1 / np.pi)
    spec = G.schlick(F0, h, o) * (G.ggx_G1(alpha, w) * pg)[:, None]
    diff = ((1 - schlick_c(F0, o[:, 2])) * (1 - schlick_c(F0, c))) * kd * (c * (c * t(1 / np.pi)))[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where((pb > 0)[:, None], (spec + diff) / np.where(pb > 0, pb, 1)[:, None], 0).astype(o.dtype)
    return pb.astype(o.dtype), g, spec, diff


def evaluate_of(alpha, F0, kd, o, w):
    """evaluate() for given unit directions w, the way a light sample does it: ps and h = normalize(o + w) from scratch"""
    return evaluate(alpha, F0, kd, lobe_probability(F0, kd, o[:, 2]), o, G.unit(o + w), w)


def vertex(N, D, alpha, F0, kd, rnd1, rnd2, u_sel, dtype=np.float64):
    """The sampled vertex for n items: N, D (n, 3), alpha, rnd1, rnd2, u_sel (n,), F0 and kd (n, 3) or (3,), all first rounded to float32
    (the values the device gets) and then evaluated in `dtype`.  Returns a dict of arrays."""
    f = lambda a: np.asarray(a, dtype=np.float32).astype(dtype)
    N, D, alpha, rnd1, rnd2, u_sel = f(N), f(D), f(alpha), f(rnd1), f(rnd2), f(u_sel)
    F0 = np.broadcast_to(f(F0), N.shape)
    kd = np.broadcast_to(f(kd), N.shape)
    gv = G.vertex(N, D, alpha, rnd1, rnd2, F0, dtype=dtype)       # the coat lobe's draw: visible normals on the disc point of rnd1, rnd2
    X, Z, o = gv["X"], gv["Z"], gv["o"]
    ps = lobe_probability(F0, kd, o[:, 2])
    coat = u_sel < ps
    r = np.sqrt(rnd1)
    theta = (2.0 * np.pi * rnd2.astype(np.float64)).astype(np.float32).astype(np.float64)
    sn, cs = np.sin(theta).astype(dtype), np.cos(theta).astype(dtype)
    base = np.stack([r * cs, r * sn, np.sqrt(1 - rnd1)], 1)         # the base lobe's: diffuse_direction's cosine lobe
    w = np.where(coat[:, None], gv["w"], base)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = np.where(coat[:, None], gv["h"], G.unit(o + base))
    world = X * w[:, 0:1] + N * w[:, 2:3] + Z * w[:, 1:2]
    pb, g, spec, diff = evaluate(alpha, F0, kd, ps, o, h, w)
    pb_again, g_again, _, _ = evaluate_of(alpha, F0, kd, o, G.local(G.unit(world), X, Z, N))
    return dict(world=world, w=w, h=h, o=o, ps=ps, coat=coat, pb=pb, g=g, pb_again=pb_again, g_again=g_again, l2=gv["l2"], X=X, Z=Z)


def debug_columns(v):
    """vertex()'s result in the layout of pt_debug_coated: (n, 10)"""
    return np.concatenate([v["world"], v["ps"][:, None], v["coat"].astype(v["world"].dtype)[:, None], v["pb"][:, None], v["g"][:, 0:1], v["pb_again"][:, None],
                           v["g_again"][:, 0:1], v["o"][:, 2:3]], 1)


COLUMNS = ("direction", "ps", "p_b sampled", "g.x sampled", "p_b again", "g.x again", "o.z")
COLUMN_INDEX = (3, 5, 6, 7, 8, 9)      # where COLUMNS[1:] sit in the layout of pt_debug_coated


def column_errors(got, want):
    """Relative errors per item, (n, 7) in the order of COLUMNS: the direction as a vector, the others |got - want| / |want| (|got| itself
    where `want` is 0).  The lobe column is compared separately (it is a decision, not a value)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    out = np.zeros((len(want), 7))
    out[:, 0] = np.linalg.norm(got[:, :3] - want[:, :3], axis=1) / np.linalg.norm(want[:, :3], axis=1)
    for k, c in enumerate(COLUMN_INDEX):
        d = np.abs(got[:, c] - want[:, c])
        den = np.abs(want[:, c])
        out[:, k + 1] = np.where(den > 0, d / np.where(den > 0, den, 1.0), d)
    return out


class CoatedModel(G.GlossyModel):
    """glossy_ref.GlossyModel with material type 5 shaded as the coated diffuse (coated = False: inert, as without the option).  ps_margin:
    a lobe choice whose |u_sel - ps| is below it is a near tie (the float32 restatement's error of ps)."""

    COATED_EVENTS = ("coated_coat", "coated_base", "coated_end_wz", "coated_end_ng", "coated_light", "coated_emitter_wb", "coated_sky")

    def __init__(self, *a, coated=True, ps_margin=1e-5, **k):
        super().__init__(*a, **k)
        self.coated = coated
        self.ps_margin = ps_margin
        self.events.update({e: 0 for e in self.COATED_EVENTS})

    def _coated(self, m, N, D, r1=0.0, r2=0.0, us=0.0):
        v = vertex(N[None], D[None], [G.roughness(m["shininess"])], m["F0"][:3], m["kd"][:3], [r1], [r2], [us])
        return {k: x[0] for k, x in v.items()}

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
        # pb_prev: the p_b a glossy or coated vertex sampled with (None: cosine lobe); prev: "glossy" / "coated" / None
        after_lobe, Nprev, pb_prev, prev, inside = False, None, None, None, False
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
                        C = C + Esky * (fL + fB) * fS * fR * wb
                break
            m = self._mat(ti)
            typ = int(m["type"])
            gl = typ == 4 and self.glossy
            ct = typ == 5 and self.coated
            N0 = self.n[ti].copy()
            hp = P + D * t
            Em = m["emission"][:3].astype(np.float64)
            if iterations == 1:
                C = (m["F0"][:3] if gl else m["kd"][:3]).astype(np.float64) + Em
            Ng = -N0 if D @ N0 > 0 else N0
            N, _, near = S.shading_normal(self.v[ti], N0, self.vn[ti], bool(self.has[ti]), D, hp)
            tie |= near
            if typ in (0, 3) or gl or ct:
                inten = max(0.0, float(-D @ N))
                wb = 1.0
                pa = self.pdf_area[ti] * (1.0 - pe)
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
                                fs = fS
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
                                    pbv, gg, _, _ = evaluate_of(al, m["F0"][:3].astype(np.float64)[None], m["kd"][:3].astype(np.float64)[None], cv["o"][None], wl3[None])
                                    pb = float(pbv[0])
                                    fs = fS * gg[0]
                                    ev["coated_light"] += 1
                                else:
                                    pb = cosx / np.pi
                                if pb > 0:
                                    wl = pb / pl if strategy == 1 else pb * pl / (pb * pb + pl * pl)
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
                else:
                    nd = self.diffuse_dir(N, r1, r2)
                    pb_prev, prev = None, None
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
                    ev["glossy_end_ng" if gl else "coated_end_ng" if ct else "lobe_end"] += 1
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
