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


EVENTS = G.EVENTS + ("delta", "delta_glossy", "delta_ng_reject")


class LightsModel(G.GlossyModel):
    """glossy_ref.GlossyModel (material types 0-4, vertex normals, with or without an environment) plus a light set: lights =
    Scene.debug_lights(); vnormals = None: no triangle has vertex normals; env as smooth_ref.SmoothModel takes it."""

    EVENTS = EVENTS

    def __init__(self, verts, normals, mats, mat_of, cam, lights, vnormals=None, env=None, table=None, margin=1e-4, glossy=True, **settings):
        settings.setdefault("events", S.BASE_EVENTS + EVENTS)
        super().__init__(verts, normals, mats, mat_of, cam, vnormals, env=env, table=table, margin=margin, glossy=glossy, lights=lights, **settings)
