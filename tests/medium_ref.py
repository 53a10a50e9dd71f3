"""Float64 numpy model of Scene.render_nee with a homogeneous medium (include/pt_api.h pins the free flight, the scatter vertex and the
transmittance of light samples), built on tests/lights_ref.py's LightsModel: the same LCG stream, the same hashes of S and ~S, the same
selection rules, brute-force intersection, plus the medium's own stream S ^ 0x5bd1e995.  Also the float64 statements of the pieces --
the slab clip, the free flight, Henyey-Greenstein and its inverse cdf, the transmittance -- that tests/test_medium_host.py checks
against closed forms and tests/test_gpu_medium.py holds pt_debug_medium to."""
import numpy as np

import glossy_ref as G
import lights_ref as L
import nee_ref as R
import smooth_ref as S

STREAM = 0x5BD1E995
FLIGHT_MARGIN = 2e-5          # d < L is a near tie when |d - L| is within this share of the larger: float32 logf, the divide, the clip
SLAB_MARGIN = 1e-5            # ... and the slab ordering when the clipped interval is this short against its ends, or a ray this parallel


def hg(g, c):
    """Henyey-Greenstein's density (per steradian) of the cosine c between the directions of travel before and after the vertex"""
    return (1.0 - g * g) / (4.0 * np.pi * (1.0 + g * g - 2.0 * g * c) ** 1.5)


def hg_cos(g, u1):
    """the inverse cdf: the cosine that u1 in [0, 1) draws (-1 at u1 = 0, towards +1 at 1; the isotropic branch runs the other way)"""
    if abs(g) < 1e-3:
        return 1.0 - 2.0 * u1
    r = (1.0 - g * g) / (1.0 - g + 2.0 * g * u1)
    return (1.0 + g * g - r * r) / (2.0 * g)


def hg_cdf(g, c):
    """P(cosine <= c), in closed form"""
    if abs(g) < 1e-3:
        return (1.0 + c) / 2.0
    return (1.0 - g * g) / (2.0 * g) * (1.0 / np.sqrt(1.0 + g * g - 2.0 * g * c) - 1.0 / (1.0 + g))


def clip(lo, hi, P, D, t):
    """the part (a, b) of [0, t] of the ray (P, D) inside the box [lo, hi] by slabs, and whether the ordering is a near tie; the length
    inside is max(b - a, 0); b = -inf when the ray is parallel to a slab and outside it"""
    a, b, near = 0.0, float(t), False
    for ax in range(3):
        p, d = float(P[ax]), float(D[ax])
        near |= 0.0 < abs(d) < SLAB_MARGIN
        if d != 0.0 and np.isfinite(1.0 / d):
            t0, t1 = (lo[ax] - p) / d, (hi[ax] - p) / d
            a, b = max(a, min(t0, t1)), min(b, max(t0, t1))
        elif not (lo[ax] <= p <= hi[ax]):
            b = -np.inf
        for edge in (lo[ax], hi[ax]):
            near |= bool(np.isfinite(edge)) and d == 0.0 and abs(p - edge) < SLAB_MARGIN * (1.0 + abs(edge))
    if np.isfinite(a) and np.isfinite(b):
        near |= abs(b - a) < SLAB_MARGIN * (1.0 + abs(a) + abs(b)) and b != a
    return a, b, near


def flight(sigma_t, u):
    return -np.log1p(-u) / sigma_t


def frame(D):
    """(Z, X) of the tangent frame the diffuse vertex builds around its normal (nee_ref.Model.diffuse_dir), here around D"""
    E = 0.001
    if abs(D[0]) <= E and abs(D[2]) <= E:
        rl = 1.0 / np.sqrt(D[2] * D[2] + D[1] * D[1])
        Z = np.array([0.0, -D[2] * rl, D[1] * rl])
    else:
        rl = 1.0 / np.sqrt(D[2] * D[2] + D[0] * D[0])
        Z = np.array([-D[2] * rl, 0.0, D[0] * rl])
    return Z, np.cross(D, Z)


def direction(g, D, u1, u2):
    """the scatter vertex's new direction (unit) from (u1, u2) around the unit direction D, its p_b and its cosine"""
    D = np.asarray(D, dtype=np.float64)
    c = hg_cos(g, u1)
    s = np.sqrt(max(0.0, 1.0 - c * c))
    phi = 2.0 * np.pi * u2
    Z, X = frame(D)
    w = X * (s * np.cos(phi)) + Z * (s * np.sin(phi)) + D * c
    return w / np.linalg.norm(w), hg(g, c), c


def transmittance(med, o, w, limit):
    a, b, near = clip(med["lo"], med["hi"], o, w, limit)
    ell = max(b - a, 0.0)
    return (np.exp(-med["sigma_t"] * ell) if ell > 0 else 1.0), near


def medium_of(d):
    """Scene.medium() -> the model's record in float64 (None: no medium)"""
    if d is None or not d["sigma_t"] > 0:
        return None
    return dict(sigma_t=float(d["sigma_t"]), albedo=np.asarray(d["albedo"], dtype=np.float64), g=float(d["g"]),
                lo=np.asarray(d["lo"], dtype=np.float64), hi=np.asarray(d["hi"], dtype=np.float64))


NO_LIGHTS = dict(records=np.zeros((0, 16), dtype=np.float32), cdf=np.zeros(0, dtype=np.float32), P_ana=0.0)


class MediumModel(L.LightsModel):
    """lights_ref.LightsModel plus a medium: medium = Scene.medium() (None or sigma_t = 0: the model is LightsModel's); lights =
    Scene.debug_lights(), or None when no set is held.  sample() is LightsModel.sample with the free flight after the closest hit, the
    scatter vertex, and T on every light sample taken outside a dielectric."""

    EVENTS = L.LightsModel.EVENTS + ("scatter", "scatter_light", "scatter_delta", "scatter_emitter_wb", "scatter_sky")

    def __init__(self, verts, normals, mats, mat_of, cam, lights, medium, vnormals=None, env=None, table=None, margin=1e-4, glossy=True):
        super().__init__(verts, normals, mats, mat_of, cam, lights if lights is not None else NO_LIGHTS, vnormals=vnormals, env=env, table=table,
                         margin=margin, glossy=glossy)
        self.medium = medium_of(medium)

    def _candidate(self, key, nkey, k, o, sky, tie):
        """the light sample of segment k seen from o: (cand, tie); cand = None, or (E, p_l, emitter cosine, w, what the shadow ray must
        return, its cut, delta) -- LightsModel.sample's three-way selection"""
        pe, pa = self.pe, self.pa
        u0 = R.nee_unit(R.nee_rand(key, k, 0))
        u1 = R.nee_unit(R.nee_rand(key, k, 1))
        u2 = R.nee_unit(R.nee_rand(key, k, 2))
        ua = R.nee_unit(R.nee_rand(nkey, k, 2))
        tie |= abs(ua - pa) < L.SELECT_MARGIN and 0.0 < pa < 1.0
        cand = None
        if ua < pa:
            j = min(int(np.searchsorted(self.set_cdf, np.float32(u0), side="right")), len(self.set_cdf) - 1)
            smp = L.light_sample(self.set[j], o)
            pl = pa * self.set[j]["P_light"]
            if smp is not None and pl > 0:
                cand = (smp[2], pl, 1.0, smp[0], -1, smp[1], True)
        else:
            use_sky = False
            if sky:
                us = R.nee_unit(R.nee_rand(nkey, k, 0))
                tie |= abs(us - pe) < L.SELECT_MARGIN and 0.0 < pe < 1.0
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
