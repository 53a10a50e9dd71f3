"""Float64 numpy model of Scene.render_nee under option smooth_normals (include/pt_api.h pins the estimator), on top of
tests/nee_ref.py and tests/env_ref.py: the same LCG stream, the same hashes, brute-force intersection, with or without an environment,
material types 0, 1, 2 and 3.  It shares no code with the library.  Also the float64 statement of the shading normal itself
(shading_normal) for tests of Scene.debug_shading_normals."""
import numpy as np

import env_ref as E
import nee_ref as R
from path_ref import PathModel

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


BASE_EVENTS = ("spec_fallback", "lobe_end", "ng_reject")


class SmoothModel(PathModel):
    """PathModel shading with vertex normals: vnormals (n,3,3) as recorded (add order), zero or non-finite where a triangle has none.
    env = dict(rgb=, tables=Scene.debug_environment(), scale=, yaw_degrees=)."""

    def __init__(self, verts, normals, mats, mat_of, cam, vnormals, env=None, table=None, margin=1e-4, **settings):
        settings.setdefault("events", BASE_EVENTS)
        super().__init__(verts, normals, mats, mat_of, cam, table=table, margin=margin, env=env, vnormals=vnormals, **settings)
