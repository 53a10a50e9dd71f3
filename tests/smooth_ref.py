"""Float64 numpy model of Scene.render_nee under option smooth_normals (include/pt_api.h pins the estimator), on top of
tests/nee_ref.py and tests/env_ref.py: the same LCG stream, the same hashes, brute-force intersection, with or without an environment,
material types 0, 1, 2 and 3.  It shares no code with the library.  Also the float64 statement of the shading normal itself
(shading_normal) for tests of Scene.debug_shading_normals."""
import numpy as np

import env_ref as E
import nee_ref as R

SIDE_MARGIN = 1e-5        # a sign decision on a cosine this close to 0 may fall the other way in float32


def unit64(n):
    """the packed normals: each divided by its float64 length, rounded once to float32"""
    n = np.asarray(n, dtype=np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32).astype(np.float64)


def has_normals(n):
    n = np.asarray(n, dtype=np.float32).reshape(-1, 3, 3)
    return np.isfinite(n).all(axis=(1, 2)) & (n != 0).any(axis=2).all(axis=1)


def shading_normal(v, N, vn, has, D, hp):
    """(Ns, used the vertex normals, near a sign decision) for a hit at hp on the triangle v (3,3) with record normal N and packed
    normals vn (3,3): the pinned formula in float64."""
    Ng = -N if D @ N > 0 else N
    if not has:
        return Ng, False, False
    r1, r2, r3 = v
    a1 = max(0.0, float(np.cross(r3 - r2, hp - r2) @ N))
    a2 = max(0.0, float(np.cross(r1 - r3, hp - r3) @ N))
    a3 = max(0.0, float(np.cross(r2 - r1, hp - r1) @ N))
    s = vn[0] * a1 + vn[1] * a2 + vn[2] * a3
    l2 = float(s @ s)
    if not (0.0 < l2 < np.inf):
        return Ng, False, False
    Ns = s / np.sqrt(l2)
    near = abs(float(Ns @ Ng)) < SIDE_MARGIN
    if Ns @ Ng < 0:
        Ns = -Ns
    c = float(-D @ Ns)
    near |= abs(c) < SIDE_MARGIN
    if not c > 0:
        return Ng, False, near
    return Ns, True, near


class SmoothModel(E.EnvModel):
    """env_ref.EnvModel (env = None: nee_ref.Model) shading with vertex normals: vnormals (n,3,3) as recorded (add order), zero or
    non-finite where a triangle has none.  env = dict(rgb=, tables=Scene.debug_environment(), scale=, yaw_degrees=)."""

    def __init__(self, verts, normals, mats, mat_of, cam, vnormals, env=None, table=None, margin=1e-4):
        if env is not None:
            super().__init__(verts, normals, mats, mat_of, cam, env["rgb"], env["tables"], scale=env.get("scale", 1.0),
                             yaw_degrees=env.get("yaw_degrees", 0.0), table=table, margin=margin)
        else:
            R.Model.__init__(self, verts, normals, mats, mat_of, cam, table=table, margin=margin)
            self.pe, self.has_dist = 0.0, False
        self.has = has_normals(vnormals)
        self.vn = unit64(np.asarray(vnormals, dtype=np.float32).reshape(-1, 3, 3))
        self.events = {"spec_fallback": 0, "lobe_end": 0, "ng_reject": 0}

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

    def sample(self, gid, seed, iterations, strategy):
        """one sample of pixel gid: (colour, new LCG state, near-tie seen); self.last = the sample's events"""
        ev = {"spec_fallback": 0, "lobe_end": 0, "ng_reject": 0}
        self.last = ev
        key = int(seed) & 0xFFFFFFFF
        tie = False
        seed, r1 = R.lcg(seed)
        seed, r2 = R.lcg(seed)
        P, D = self.camera_ray(gid, r1, r2)
        one = np.ones(3)
        fL, fB, fS, fR, C = one.copy(), one.copy(), one.copy(), one.copy(), np.zeros(3)
        after_lobe, Nprev, inside = False, None, False
        sky = hasattr(self, "rgb")
        nee = strategy != 0 and (len(self.lights) > 0 or self.has_dist)
        pe = self.pe
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
                                pb = max(0.0, float(Nprev @ D)) / np.pi
                                wb = pb * pb / (pb * pb + pl * pl)
                        C = C + Esky * (fL + fB) * fS * fR * wb
                break
            m = self._mat(ti)
            typ = int(m["type"])
            N0 = self.n[ti].copy()
            hp = P + D * t
            Em = m["emission"][:3].astype(np.float64)
            if iterations == 1:
                C = m["kd"][:3].astype(np.float64) + Em
            Ng = -N0 if D @ N0 > 0 else N0
            N, _, near = shading_normal(self.v[ti], N0, self.vn[ti], bool(self.has[ti]), D, hp)
            tie |= near
            if typ in (0, 3):
                inten = max(0.0, float(-D @ N))
                wb = 1.0
                pa = self.pdf_area[ti] * (1.0 - pe)
                if typ == 3 and nee and after_lobe and pa > 0 and inten > 0:
                    if strategy == 1:
                        wb = 0.0
                    else:
                        pb = max(0.0, float(Nprev @ D)) / np.pi
                        pl = pa * t * t / inten
                        wb = pb * pb / (pb * pb + pl * pl)
                if nee and k + 1 < iterations:
                    u0 = R.nee_unit(R.nee_rand(key, k, 0))
                    u1 = R.nee_unit(R.nee_rand(key, k, 1))
                    u2 = R.nee_unit(R.nee_rand(key, k, 2))
                    o = hp + Ng * 0.001
                    cand = None                      # (E, p_l, emitter cosine, w, what the shadow ray must return, its cut)
                    use_sky = False
                    if sky:
                        us = R.nee_unit(R.nee_rand(~key & 0xFFFFFFFF, k, 0))
                        tie |= abs(us - pe) < E.SELECT_MARGIN and 0.0 < pe < 1.0
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
                        tie |= abs(cosx) < SIDE_MARGIN or abs(cosg) < SIDE_MARGIN
                        if cosx > 0 and not cosg > 0:
                            ev["ng_reject"] += 1
                        if cosx > 0 and cosg > 0:
                            hi, _, st = self.intersect(o, w, cut)
                            tie |= st
                            if hi == want:
                                pb = cosx / np.pi
                                wl = pb / pl if strategy == 1 else pb * pl / (pb * pb + pl * pl)
                                fl, fb = (self._update(m, N, hp, w, fL, fB) if typ == 0 else (fL, fB))
                                C = C + Ey * (fl + fb) * fS * fR * (g * wl)
                seed, r1 = R.lcg(seed)
                seed, r2 = R.lcg(seed)
                nd = self.diffuse_dir(N, r1, r2)
                if typ == 0:
                    fL, fB = self._update(m, N, hp, nd, fL, fB)
                else:
                    C = C + Em * (fL + fB) * fS * fR * (inten * wb)
                P, D = hp + Ng * 0.001, nd
                after_lobe, Nprev = True, N
                below = float(nd @ Ng)
                tie |= abs(below) < SIDE_MARGIN
                if below <= 0:
                    ev["lobe_end"] += 1
                    break
            elif typ in (1, 2):
                rnd = 0.0
                if typ == 2:
                    seed, rnd = R.lcg(seed)
                d, refr, F, prob, near = self._spec(m, typ, N, D, inside, rnd)
                tie |= near
                g = float(d @ Ng) / np.linalg.norm(d)
                tie |= abs(g) < SIDE_MARGIN
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

    def render(self, seeds, iterations, nsamples, strategy):
        """colors (npix, 3) float64, final LCG states, near-tie mask; self.pixel_events[name] = per-pixel counts"""
        n = len(seeds)
        cols = np.zeros((n, 3))
        out_seeds = np.zeros(n, dtype=np.int64)
        ties = np.zeros(n, dtype=bool)
        self.pixel_events = {k: np.zeros(n, dtype=np.int64) for k in self.events}
        for i in range(n):
            s = int(seeds[i])
            acc = np.zeros(3)
            for _ in range(nsamples):
                c, s, t = self.sample(i, s, iterations, strategy)
                acc += c
                ties[i] |= t
                for k2, v2 in self.last.items():
                    self.pixel_events[k2][i] += v2
            cols[i] = acc / nsamples
            out_seeds[i] = s
        return cols, out_seeds.astype(np.int32), ties
