"""Float64 numpy model of Scene.render_nee under option glossy (include/pt_api.h pins the vertex), on top of tests/smooth_ref.py: the
same LCG stream, the same hashes, brute-force intersection, with or without an environment and vertex normals, material types 0-4.  It
shares no code with the library.  vertex() is the rough-metal vertex itself, vectorised and in a chosen precision: float64 is the
reference, float32 the restatement of the pinned sequence that the tests measure their tolerance with."""
import numpy as np

import nee_ref as R
import smooth_ref as S

DEGENERATE_L2 = 1e-9      # Vh this close to the normal: the tangent T1 is rounding noise, float32 may pick any rotation


def roughness(shininess):
    s = float(np.float32(shininess))
    if not np.isfinite(s) or s < 0:
        return 1.0
    return float(np.float32(min(1.0, max(0.03, np.sqrt(2.0 / (s + 2.0))))))


def frame(N):
    """(X, Z) of diffuse_direction for normals N (n, 3), in N's dtype"""
    E = 0.001
    yaxis = (np.abs(N[:, 0]) <= E) & (np.abs(N[:, 2]) <= E)
    other = np.where(yaxis, N[:, 1], N[:, 0])
    rl = 1 / np.sqrt(N[:, 2] * N[:, 2] + other * other)
    zero = np.zeros_like(rl)
    Z = np.where(yaxis[:, None], np.stack([zero, -N[:, 2] * rl, N[:, 1] * rl], 1), np.stack([-N[:, 2] * rl, zero, N[:, 0] * rl], 1))
    return np.cross(N, Z), Z


def dot(a, b):
    return (a * b).sum(axis=1)


def unit(v):
    return v / np.sqrt(dot(v, v))[:, None]


def ggx_D(alpha, h):
    a2 = alpha * alpha
    d = a2 * h[:, 2] ** 2 + (h[:, 0] ** 2 + h[:, 1] ** 2)
    return a2 / (h.dtype.type(np.pi) * (d * d))


def ggx_G1(alpha, v):
    with np.errstate(divide="ignore", invalid="ignore"):
        g = 2 * v[:, 2] / (v[:, 2] + np.sqrt(alpha * alpha * (v[:, 0] ** 2 + v[:, 1] ** 2) + v[:, 2] ** 2))
    return np.where(v[:, 2] > 0, g, 0).astype(v.dtype)


def ggx_pdf(alpha, o, h):
    with np.errstate(divide="ignore", invalid="ignore"):
        p = ggx_G1(alpha, o) * ggx_D(alpha, h) / (4 * o[:, 2])
    return np.where(o[:, 2] > 0, p, 0).astype(o.dtype)


def ggx_pdf_of(alpha, o, w):
    h = unit(o + w)
    return ggx_pdf(alpha, o, h), h


def schlick(F0, h, o):
    c = np.abs(dot(h, o))
    return F0 + (1 - F0) * ((1 - c) ** 5)[:, None]


def local(v, X, Z, N):
    return np.stack([dot(v, X), dot(v, Z), dot(v, N)], 1)


def vertex(N, D, alpha, rnd1, rnd2, F0, dtype=np.float64):
    """The sampled vertex for n items: N, D (n, 3), alpha, rnd1, rnd2 (n,), F0 (n, 3) or (3,), all first rounded to float32 (the values the
    device gets) and then evaluated in `dtype`.  Returns a dict of arrays."""
    f = lambda a: np.asarray(a, dtype=np.float32).astype(dtype)
    N, D, alpha, rnd1, rnd2 = f(N), f(D), f(alpha), f(rnd1), f(rnd2)
    F0 = np.broadcast_to(f(F0), N.shape)
    X, Z = frame(N)
    o = local(-D, X, Z, N)
    Vh = unit(np.stack([alpha * o[:, 0], alpha * o[:, 1], o[:, 2]], 1))
    l2 = Vh[:, 0] ** 2 + Vh[:, 1] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sqrt(l2)
        T1 = np.where((l2 > 0)[:, None], np.stack([-Vh[:, 1] / s, Vh[:, 0] / s, np.zeros_like(s)], 1), np.array([1, 0, 0], dtype=dtype))
    T2 = np.cross(Vh, T1)
    r = np.sqrt(rnd1)
    theta = (2.0 * np.pi * rnd2.astype(np.float64)).astype(np.float32).astype(np.float64)      # the float angle, as the device rounds it
    sn, cs = np.sin(theta).astype(dtype), np.cos(theta).astype(dtype)
    t1, t2 = r * cs, r * sn
    q = dtype(0.5) * (1 + Vh[:, 2])
    t2 = (1 - q) * np.sqrt(np.maximum(1 - t1 * t1, 0)) + q * t2
    t3 = np.sqrt(np.maximum(1 - t1 * t1 - t2 * t2, 0))
    Nh = T1 * t1[:, None] + T2 * t2[:, None] + Vh * t3[:, None]
    h = unit(np.stack([alpha * Nh[:, 0], alpha * Nh[:, 1], np.maximum(Nh[:, 2], 0)], 1))
    w = h * (2 * dot(o, h))[:, None] - o
    world = X * w[:, 0:1] + N * w[:, 2:3] + Z * w[:, 1:2]
    pb = ggx_pdf(alpha, o, h)
    g1w = ggx_G1(alpha, w)
    F = schlick(F0, h, o)
    pb_again, _ = ggx_pdf_of(alpha, o, local(unit(world), X, Z, N))
    return dict(world=world, w=w, h=h, o=o, pb=pb, g1w=g1w, F=F, g=F * g1w[:, None], pb_again=pb_again, l2=l2, X=X, Z=Z)


def debug_columns(v):
    """vertex()'s result in the layout of pt_debug_glossy: (n, 8)"""
    return np.concatenate([v["world"], v["pb"][:, None], v["g1w"][:, None], v["F"][:, 0:1], v["pb_again"][:, None], v["o"][:, 2:3]], 1)


COLUMNS = ("direction", "p_b sampled", "G1(w)", "F.x", "p_b again", "o.z")


def column_errors(got, want):
    """Relative errors per item, (n, 6) in the order of COLUMNS, of pt_debug_glossy's layout: the direction as a vector (|got - want| /
    |want|), the others |got - want| / |want|; where G1(w) is 0 in `want` (w.z <= 0) the entry is |got| itself."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    out = np.zeros((len(want), 6))
    out[:, 0] = np.linalg.norm(got[:, :3] - want[:, :3], axis=1) / np.linalg.norm(want[:, :3], axis=1)
    for k, c in ((1, 3), (2, 4), (3, 5), (4, 6), (5, 7)):
        d = np.abs(got[:, c] - want[:, c])
        den = np.abs(want[:, c])
        out[:, k] = np.where(den > 0, d / np.where(den > 0, den, 1.0), d)
    return out


class GlossyModel(S.SmoothModel):
    """smooth_ref.SmoothModel with material type 4 shaded as the rough metal (glossy = False: inert, as without the option)."""

    EVENTS = ("glossy_vertex", "glossy_end_wz", "glossy_end_ng", "glossy_light", "glossy_emitter_wb", "glossy_sky")

    def __init__(self, *a, glossy=True, **k):
        super().__init__(*a, **k)
        self.glossy = glossy
        self.events = {"spec_fallback": 0, "lobe_end": 0, "ng_reject": 0, **{e: 0 for e in self.EVENTS}}

    def _glossy(self, m, N, D, r1=0.0, r2=0.0):
        v = vertex(N[None], D[None], [roughness(m["shininess"])], [r1], [r2], m["F0"][:3])
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
        after_lobe, Nprev, pb_prev, inside = False, None, None, False      # pb_prev: the p_b a glossy vertex sampled with (None: cosine lobe)
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
                pa = self.pdf_area[ti] * (1.0 - pe)
                if typ == 3 and nee and after_lobe and pa > 0 and inten > 0:
                    if strategy == 1:
                        wb = 0.0
                    else:
                        pb = prev_pb(D)
                        pl = pa * t * t / inten
                        wb = pb * pb / (pb * pb + pl * pl)
                    if pb_prev is not None and wb < 1.0:
                        ev["glossy_emitter_wb"] += 1
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
                                    pbv, h = ggx_pdf_of(np.array([roughness(m["shininess"])]), gv["o"][None], wl3[None])
                                    pb = float(pbv[0])
                                    F = schlick(m["F0"][:3].astype(np.float64)[None], h, gv["o"][None])[0]
                                    fs = fS * F * float(ggx_G1(np.array([roughness(m["shininess"])]), wl3[None])[0])
                                    ev["glossy_light"] += 1
                                else:
                                    pb = cosx / np.pi
                                wl = pb / pl if strategy == 1 else pb * pl / (pb * pb + pl * pl)
                                fl, fb = (self._update(m, N, hp, w, fL, fB) if typ == 0 else (fL, fB))
                                C = C + Ey * (fl + fb) * fs * fR * (g * wl)
                seed, r1 = R.lcg(seed)
                seed, r2 = R.lcg(seed)
                ended = False
                if gl:
                    gv = self._glossy(m, N, D, r1, r2)
                    ev["glossy_vertex"] += 1
                    tie |= bool(gv["l2"] < DEGENERATE_L2) or abs(float(gv["w"][2])) < S.SIDE_MARGIN
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
