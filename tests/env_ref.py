"""Float64 numpy model of Scene.render_nee under an environment map (include/pt_api.h pins the estimator), built on
tests/nee_ref.py's Model: the same LCG stream, the same hashes, brute-force intersection; the sampling tables come from
Scene.debug_environment() as nee_ref takes the light table.  Also the numpy statements of the direction -> texel mapping and of
the tables themselves (tests/test_env_host.py)."""
import numpy as np

import nee_ref as R

EDGE_MARGIN = 1e-4          # radians: a miss direction this close to a texel edge may read the neighbour in float32
SELECT_MARGIN = 2.0 ** -20


def yaw_radians(yaw_degrees):
    return float(np.float32(float(np.float32(yaw_degrees)) * np.pi / 180.0))


def lookup(w, h, yaw_degrees, d):
    """(row, col, angular distance to the nearest texel edge) of unit direction d, in float64."""
    d = np.asarray(d, dtype=np.float64)
    theta = float(np.arccos(np.clip(d[1], -1.0, 1.0)))
    phi = float(np.arctan2(d[2], d[0])) - yaw_radians(yaw_degrees)
    fr = theta / np.pi * h
    row = min(h - 1, int(np.floor(fr)))
    turn = phi / (2.0 * np.pi)
    fc = (turn - np.floor(turn)) * w
    col = min(w - 1, int(np.floor(fc)))
    dist = np.inf
    k = np.rint(fr)
    if 0 < k < h:                                   # the poles are no edges
        dist = abs(fr - k) * np.pi / h
    if w > 1:
        dist = min(dist, abs(fc - np.rint(fc)) * (2.0 * np.pi / w) * np.sin(theta))
    return row, col, float(dist)


def luminance(rgb):
    rgb = np.asarray(rgb, dtype=np.float64)
    return 0.2126 * rgb[..., 0] + 0.7152 * rgb[..., 1] + 0.0722 * rgb[..., 2]


def solid_angles(w, h):
    th = np.arange(h + 1) * np.pi / h
    return (2.0 * np.pi / w) * (np.cos(th[:-1]) - np.cos(th[1:]))


def tables(rgb):
    """The double-precision build of the distribution: (row_cdf (h,), col_cdf (h, w), has_distribution); rows of weight 0 get a
    uniform column cdf, a map without a distribution uniform tables."""
    rgb = np.asarray(rgb, dtype=np.float64)
    h, w = rgb.shape[:2]
    lum = luminance(rgb)
    rs = lum.sum(axis=1)
    col = np.where(rs[:, None] > 0, np.cumsum(lum, axis=1) / np.where(rs > 0, rs, 1.0)[:, None], (np.arange(w) + 1.0)[None, :] / w)
    col[:, -1] = 1.0
    roww = rs * solid_angles(w, h) * w / (2.0 * np.pi)
    has = bool(roww.sum() > 0)
    row = np.cumsum(roww) / roww.sum() if has else (np.arange(h) + 1.0) / h
    row[-1] = 1.0
    return row, col, has


def texel_pdf(row_cdf, col_cdf):
    """p_env per texel from the stored float cdfs' own steps."""
    row_cdf = np.asarray(row_cdf, dtype=np.float64)
    col_cdf = np.asarray(col_cdf, dtype=np.float64)
    h, w = col_cdf.shape
    pr = np.diff(np.concatenate([[0.0], row_cdf]))
    pc = np.diff(np.concatenate([np.zeros((h, 1)), col_cdf], axis=1), axis=1)
    return pr[:, None] * pc / solid_angles(w, h)[:, None]


class EnvModel(R.Model):
    """nee_ref.Model plus an environment: rgb (h, w, 3), scale, yaw_degrees, and Scene.debug_environment()'s tables."""

    def __init__(self, verts, normals, mats, mat_of, cam, rgb, env_tables, scale=1.0, yaw_degrees=0.0, table=None, margin=1e-4):
        if len(verts):
            super().__init__(verts, normals, mats, mat_of, cam, table=table, margin=margin)
        else:                                   # no triangles at all: only the camera and the sky
            self.v = np.zeros((0, 3, 3))
            self.cam, self.lights, self.mats = cam, np.zeros(0, dtype=np.int64), mats
        self.rgb = np.asarray(rgb, dtype=np.float32).astype(np.float64)
        self.h, self.w = self.rgb.shape[:2]
        self.scale = float(np.float32(scale))
        self.yaw_degrees = yaw_degrees
        self.row_cdf = np.asarray(env_tables["row_cdf"], dtype=np.float32)
        self.col_cdf = np.asarray(env_tables["col_cdf"], dtype=np.float32)
        self.pdf = np.asarray(env_tables["pdf"], dtype=np.float64)
        self.pe = float(env_tables["P_env"])
        self.has_dist = bool((self.pdf > 0).any())

    def intersect(self, P, D, limit=np.inf):
        if not len(self.v):
            return -1, np.inf, False
        return super().intersect(P, D, limit)

    def sky(self, d):
        """(E(d), p_env(d), near a texel edge)"""
        row, col, dist = lookup(self.w, self.h, self.yaw_degrees, d)
        return self.rgb[row, col] * self.scale, float(self.pdf[row, col]), dist < EDGE_MARGIN

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
        phi = 2.0 * np.pi * ((col + t2) / self.w) + yaw_radians(self.yaw_degrees)
        return np.array([sn * np.cos(phi), ct, sn * np.sin(phi)]), self.rgb[row, col] * self.scale, float(self.pdf[row, col])

    def sample(self, gid, seed, iterations, strategy):
        """one sample of pixel gid: (colour, new LCG state, near-tie seen)"""
        key = int(seed) & 0xFFFFFFFF
        tie = False
        seed, r1 = R.lcg(seed)
        seed, r2 = R.lcg(seed)
        P, D = self.camera_ray(gid, r1, r2)
        one = np.ones(3)
        fL, fB, fS, fR, C = one.copy(), one.copy(), one.copy(), one.copy(), np.zeros(3)
        after_lobe, Nprev = False, None
        nee = strategy != 0 and (len(self.lights) > 0 or self.has_dist)
        pe = self.pe
        for k in range(iterations):
            ti, t, tt = self.intersect(P, D)
            tie |= tt
            if ti < 0:
                E, penv, edge = self.sky(D)
                tie |= edge
                if k == 0:
                    C = C + E
                else:
                    wb = 1.0
                    pl = pe * penv
                    if nee and after_lobe and pl > 0:
                        if strategy == 1:
                            wb = 0.0
                        else:
                            pb = max(0.0, float(Nprev @ D)) / np.pi
                            wb = pb * pb / (pb * pb + pl * pl)
                    C = C + E * (fL + fB) * fS * fR * wb
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
                    us = R.nee_unit(R.nee_rand(~key & 0xFFFFFFFF, k, 0))
                    tie |= abs(us - pe) < SELECT_MARGIN and 0.0 < pe < 1.0
                    o = hp + N * 0.001
                    add = None
                    if us < pe:
                        w, Ey, penv = self.sky_sample(u1, u2)
                        cosx = float(N @ w)
                        pl = pe * penv
                        if cosx > 0 and pl > 0:
                            hi, _, st = self.intersect(o, w)
                            tie |= st
                            if hi < 0:
                                add = (Ey, pl, 1.0, cosx, w)
                    elif len(self.lights):
                        j = min(int(np.searchsorted(self.cdf, np.float32(u0), side="right")), len(self.cdf) - 1)
                        li = int(self.lights[j])
                        v = self.v[li]
                        su = np.sqrt(u1)
                        y = v[0] + (v[1] - v[0]) * (u2 * su) + (v[2] - v[0]) * (su * (1.0 - u2))
                        d = y - o
                        r = np.linalg.norm(d)
                        w = d / r
                        cosx = float(N @ w)
                        cosy = abs(float(w @ self.n[li]))
                        if cosx > 0 and cosy > 0:
                            pl = self.pdf_area[li] * (1.0 - pe) * r * r / cosy
                            if pl > 0:
                                hi, _, st = self.intersect(o, w, r * R.SHADOW_CUT)
                                tie |= st
                                if hi == li:
                                    add = (self._mat(li)["emission"][:3].astype(np.float64), pl, cosy, cosx, w)
                    if add is not None:
                        Ey, pl, g, cosx, w = add
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
