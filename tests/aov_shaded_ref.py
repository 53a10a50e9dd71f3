"""Float64 replay of the shaded guide buffers (pt_render_aovs_ex with PT_AOV_SHADED; include/pt_api.h pins them).

denoise_ref._trace_chain restated in float64 on the brute-force models of tests/smooth_ref.py and tests/texture_ref.py, extended by
what the shaded guides add: the shading normal Ns at every hit of the chain (smooth_ref.shading_normal), the specular step evaluated
with Ns and once more with Ng when its direction lies on the wrong geometric side, offsets along Ng, and the textured albedo of a
terminal type-0 hit (texture_ref.albedo through TextureModel.albedo_at).  It shares no code with the library."""
import numpy as np

import smooth_ref as S


def trace_chain(model, gid, rnd1, rnd2, specular_depth, smooth=True, textured=True):
    """One sub-pixel ray of pixel gid through a texture_ref.TextureModel: dict(t = the primary hit's distance or None, albedo (3,),
    normal (3,), mat = material index or -1, near = the chain came within a margin of a decision, fallback / refraction = how often
    the specular step fell back to Ng / refracted)."""
    out = dict(t=None, albedo=np.zeros(3), normal=np.zeros(3), mat=-1, near=False, fallback=0, refraction=0)
    P, D = model.camera_ray(gid, float(rnd1), float(rnd2))
    ti, t, tie = model.intersect(P, D)
    out["near"] |= tie
    if ti < 0:
        return out
    out["t"] = t
    tint = np.ones(3)
    inside = False
    d = 0
    while True:
        mi = int(model.mat_of[ti])
        m = model.mats[mi]
        typ = int(m["type"])
        N0 = model.n[ti].copy()
        hp = P + D * t
        side = float(D @ N0)
        out["near"] |= abs(side) < S.SIDE_MARGIN
        Ng = -N0 if side > 0 else N0
        Ns, _, near = S.shading_normal(model.v[ti], N0, model.vn[ti], bool(model.has[ti]) and smooth, D, hp)
        out["near"] |= near
        if typ in (1, 2) and d < specular_depth:
            # rnd = 2 > prob: the dielectric refracts exactly when disc > 0, as the guide pass does (no LCG draw)
            w, refr, _, _, near = model._spec(m, typ, Ns, D, inside, 2.0)
            out["near"] |= near
            g = float(w @ Ng) / np.linalg.norm(w)
            out["near"] |= abs(g) < S.SIDE_MARGIN
            if (g >= 0) if refr else (g <= 0):
                out["fallback"] += 1
                w, refr, _, _, near = model._spec(m, typ, Ng, D, inside, 2.0)
                out["near"] |= near
            if typ == 1:
                tint = tint * m["F0"][:3].astype(np.float64)
            if refr:
                inside = not inside
                out["refraction"] += 1
            P, D = hp + Ng * (-0.001 if refr else 0.001), w / np.linalg.norm(w)
            d += 1
            ti, t, tie = model.intersect(P, D)
            out["near"] |= tie
            if ti < 0:
                return out                       # escaped: albedo 0, normal 0, material -1
            continue
        if typ == 1:
            a = m["F0"][:3].astype(np.float64)
        elif typ == 2:
            a = np.ones(3)
        else:
            kd = m["kd"][:3].astype(np.float64)
            if typ == 0 and textured:
                kd, near, _ = model.albedo_at(ti, hp)
                out["near"] |= near
            a = kd + m["emission"][:3].astype(np.float64)
        out["albedo"], out["normal"], out["mat"] = tint * a, Ns, mi
        return out


def replay(model, pixel_ids, offsets, specular_depth, smooth=True, textured=True):
    """The guides of those global pixel ids in float64: albedo_rgbm (n, 4), normal_depth (n, 4), near (n,) bool (a pixel any of whose
    sub-pixel chains came near a decision), and the per-pixel counts of Ng fall-backs and refractions."""
    n = len(pixel_ids)
    alb, nd = np.zeros((n, 4)), np.zeros((n, 4))
    near = np.zeros(n, bool)
    fallback, refraction = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for p, gid in enumerate(pixel_ids):
        sa, sn, st, hits, mat0 = np.zeros(3), np.zeros(3), 0.0, 0, -1
        for k, (r1, r2) in enumerate(offsets):
            c = trace_chain(model, int(gid), r1, r2, specular_depth, smooth, textured)
            near[p] |= c["near"]
            fallback[p] += c["fallback"]
            refraction[p] += c["refraction"]
            if c["t"] is not None:
                st += c["t"]
                hits += 1
            if k == 0:
                mat0 = c["mat"]
            sa += c["albedo"]
            sn += c["normal"]
        alb[p, :3] = sa / len(offsets)
        alb[p, 3] = mat0
        l = np.linalg.norm(sn)
        if l > 0:
            nd[p, :3] = sn / l
        nd[p, 3] = st / hits if hits else -1.0
    return alb, nd, near, fallback, refraction
