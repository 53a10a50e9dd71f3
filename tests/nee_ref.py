"""Float64 numpy model of Scene.render_nee (include/pt_api.h pins the estimator): the same LCG stream, the same light-sample
hash, brute-force intersection.  For scenes of a few dozen triangles (tests/test_gpu_nee.py); also the host replay of
pt_nee_rand and of the light table."""
import numpy as np

M31 = 2147483647
SHADOW_CUT = 1.0001


def lowbias32(x):
    x = np.asarray(x, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
    return x


def nee_rand(state, segment, dim):
    """pt_nee_rand, vectorised: lowbias32(lowbias32(state) + 0x9e3779b9 * (3 segment + dim + 1)) in uint32."""
    state = np.asarray(state).astype(np.int64).astype(np.uint32)
    c = (np.asarray(segment, dtype=np.int64) * 3 + np.asarray(dim, dtype=np.int64) + 1).astype(np.uint32)
    with np.errstate(over="ignore"):
        return lowbias32(lowbias32(state) + np.uint32(0x9E3779B9) * c)


def nee_unit(h):
    return float(np.float32(int(h) >> 8) * np.float32(2.0 ** -24))


def lcg(seed):
    """prog.cl:72-77 on one int state: (new state, float32 value as a Python float)"""
    n = (int(seed) * 48271) % M31 if seed >= 0 else ((int(seed) % (1 << 64)) * 48271) % M31
    return n, float(np.float32(n) / np.float32(2147483648.0))


def light_table(verts, mats, mat_of):
    """(tri indices, P_sel) of the lights in add order: type 3, emission sum > 0, area > 0; P_sel ~ area x emission sum."""
    idx, w = [], []
    for i, v in enumerate(np.asarray(verts, dtype=np.float64)):
        m = mats[int(mat_of[i])]
        es = float(m["emission"][0]) + float(m["emission"][1]) + float(m["emission"][2])
        area = 0.5 * np.linalg.norm(np.cross(v[1] - v[0], v[2] - v[0]))
        if int(m["type"]) == 3 and es > 0 and area > 0:
            idx.append(i)
            w.append(area * es)
    w = np.asarray(w, dtype=np.float64)
    return np.asarray(idx, dtype=np.int64), (w / w.sum() if len(w) else w)


def selection_probs(cdf):
    """The probability that u0 = m 2^-24 (m < 2^24) picks light j -- the first j with cdf[j] > u0 -- as P_sel of pt_api.h"""
    up = np.ceil(np.asarray(cdf, dtype=np.float64) * 2.0 ** 24)
    return np.diff(np.concatenate([[0.0], up])) / 2.0 ** 24


class Model:
    """verts (n,3,3), normals (n,3) (the Triangle records' N), mats (MATERIAL records), mat_of (n,), camera (CAMERA record)."""

    def __init__(self, verts, normals, mats, mat_of, cam, table=None, margin=1e-4):
        self.v = np.asarray(verts, dtype=np.float64)
        self.n = np.asarray(normals, dtype=np.float64)[:, :3]
        self.mats = mats
        self.mat_of = np.asarray(mat_of)
        self.cam = cam
        self.margin = margin
        self.e1 = self.v[:, 1] - self.v[:, 0]
        self.e2 = self.v[:, 2] - self.v[:, 0]
        self.lights, self.psel = light_table(self.v, mats, self.mat_of)
        if table is not None:          # Scene.debug_light_table(): the device's (packed) order of the same lights
            order = np.asarray(table[0], dtype=np.int64)
            assert sorted(order.tolist()) == sorted(self.lights.tolist())
            pos = {int(t): j for j, t in enumerate(self.lights)}
            self.psel = np.array([self.psel[pos[int(t)]] for t in order])
            self.lights = order
        self.area = 0.5 * np.linalg.norm(np.cross(self.e1, self.e2), axis=1)
        self.pdf_area = np.zeros(len(self.v))
        self.pdf_area[self.lights] = self.psel / self.area[self.lights]
        # the cdf the device searches is the one the host rounded to float: the same selection for the same u0
        self.cdf = np.cumsum(self.psel).astype(np.float32)
        if len(self.cdf):
            self.cdf[-1] = 1.0
        if table is not None:
            self.cdf = np.asarray(table[1], dtype=np.float32)
            self.psel = selection_probs(self.cdf)
            self.pdf_area[self.lights] = self.psel / self.area[self.lights]

    def intersect(self, P, D, limit=np.inf):
        """closest triangle with 0 < t < limit (index, t) and whether the answer is a near-tie (an edge within `margin` in
        barycentric terms, or two hits within a relative 1e-5 of each other)."""
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

    def camera_ray(self, gid, rnd1, rnd2):
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

    def _mat(self, ti):
        return self.mats[int(self.mat_of[ti])]

    def _update(self, m, N, hp, w, fL, fB):
        kd, ks = m["kd"][:3].astype(np.float64), m["ks"][:3].astype(np.float64)
        cosx = max(0.0, float(N @ w))
        fL = fL * (kd * cosx)
        pw = 1.0
        if not int(m["_pad"]):
            view = self.cam["eye"][:3].astype(np.float64) - hp
            view /= np.linalg.norm(view)
            h = view + w
            h /= np.linalg.norm(h)
            pw = max(0.0, float(N @ h)) ** float(m["shininess"])
        return fL, fB * (ks * pw)

    def sample(self, gid, seed, iterations, strategy):
        """one sample of pixel gid: (colour, new LCG state, near-tie seen)"""
        key = int(seed) & 0xFFFFFFFF
        tie = False
        seed, r1 = lcg(seed)
        seed, r2 = lcg(seed)
        P, D = self.camera_ray(gid, r1, r2)
        one = np.ones(3)
        fL, fB, fS, fR, C = one.copy(), one.copy(), one.copy(), one.copy(), np.zeros(3)
        after_lobe, Nprev = False, None
        nee = len(self.lights) > 0 and strategy != 0
        for k in range(iterations):
            ti, t, tt = self.intersect(P, D)
            tie |= tt
            if ti < 0:
                break
            m = self._mat(ti)
            typ = int(m["type"])
            N = self.n[ti].copy()
            hp = P + D * t
            E = m["emission"][:3].astype(np.float64)
            if iterations == 1:
                C = m["kd"][:3].astype(np.float64) + E
            if D @ N > 0:
                N = -N
            if typ in (0, 3):
                inten = max(0.0, float(-D @ N))
                wb = 1.0
                if typ == 3 and nee and after_lobe and self.pdf_area[ti] > 0 and inten > 0:
                    if strategy == 1:
                        wb = 0.0
                    else:
                        pb = max(0.0, float(Nprev @ D)) / np.pi
                        pl = self.pdf_area[ti] * t * t / inten
                        wb = pb * pb / (pb * pb + pl * pl)
                if nee and k + 1 < iterations:
                    u0 = nee_unit(nee_rand(key, k, 0))
                    u1 = nee_unit(nee_rand(key, k, 1))
                    u2 = nee_unit(nee_rand(key, k, 2))
                    j = min(int(np.searchsorted(self.cdf, np.float32(u0), side="right")), len(self.cdf) - 1)
                    li = int(self.lights[j])
                    v = self.v[li]
                    su = np.sqrt(u1)
                    y = v[0] + (v[1] - v[0]) * (u2 * su) + (v[2] - v[0]) * (su * (1.0 - u2))
                    o = hp + N * 0.001
                    d = y - o
                    r = np.linalg.norm(d)
                    w = d / r
                    cosx = float(N @ w)
                    cosy = abs(float(w @ self.n[li]))
                    if cosx > 0 and cosy > 0:
                        hi, _, st = self.intersect(o, w, r * SHADOW_CUT)
                        tie |= st
                        if hi == li:
                            pb = cosx / np.pi
                            pl = self.pdf_area[li] * r * r / cosy
                            wl = pb / pl if strategy == 1 else pb * pl / (pb * pb + pl * pl)
                            fl, fb = (self._update(m, N, hp, w, fL, fB) if typ == 0 else (fL, fB))
                            Ey = self._mat(li)["emission"][:3].astype(np.float64)
                            C = C + Ey * (fl + fb) * fS * fR * (cosy * wl)
                seed, r1 = lcg(seed)
                seed, r2 = lcg(seed)
                nd = self.diffuse_dir(N, r1, r2)
                if typ == 0:
                    fL, fB = self._update(m, N, hp, nd, fL, fB)
                else:
                    C = C + E * (fL + fB) * fS * fR * (inten * wb)
                P, D = hp + N * 0.001, nd
                after_lobe, Nprev = True, N
            elif typ == 1:
                F0 = m["F0"][:3].astype(np.float64)
                cosa = abs(float(N @ D))
                F = F0 + (1.0 - F0) * (1.0 - cosa) ** 5
                fS = fS * F
                nd = D - N * (2.0 * float(N @ D))
                P, D = hp + N * 0.001, nd / np.linalg.norm(nd)
                after_lobe = False
            else:
                raise NotImplementedError("the model covers material types 0, 1 and 3")
        return C, seed, tie

    def render(self, seeds, iterations, nsamples, strategy):
        """colors (npix, 3) float64, final LCG states, near-tie mask; pixel i is global pixel i (world 1)"""
        n = len(seeds)
        cols = np.zeros((n, 3))
        out_seeds = np.zeros(n, dtype=np.int64)
        ties = np.zeros(n, dtype=bool)
        for i in range(n):
            s = int(seeds[i])
            acc = np.zeros(3)
            for k in range(nsamples):
                c, s, t = self.sample(i, s, iterations, strategy)
                acc += c
                ties[i] |= t
            cols[i] = acc / nsamples
            out_seeds[i] = s
        return cols, out_seeds.astype(np.int32), ties
