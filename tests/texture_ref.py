"""Float64 numpy model of Scene.render_nee under option textures (include/pt_api.h pins the lookup), on top of
tests/smooth_ref.SmoothModel: the albedo of a type-0 vertex is kd times the texel the pinned formula reads, from the stored texels of
Scene.debug_texture.  It shares no code with the library.  Also the float64 statement of the lookup itself (albedo) for tests of
Scene.debug_albedo.  The preview of iterations == 1 is not modelled (tests/test_gpu_texture.py checks it against the formula directly)."""
import numpy as np

import smooth_ref as S

NEAREST_MARGIN = 1e-4     # nearest filtering: a texel coordinate this close to an integer may fall into the neighbour in float32
WRAP_MARGIN = 1e-6        # the argument of the wrap's floor this close to an integer may wrap the other way in float32


def has_uvs(uv):
    uv = np.asarray(uv, dtype=np.float32).reshape(-1, 6)
    with np.errstate(invalid="ignore"):
        return (np.abs(uv) <= 65536.0).all(axis=1)


def weights(v, N, hp):
    """the three weights of the shading normal (smooth_ref.shading_normal), each the weight of the opposite vertex"""
    r1, r2, r3 = v
    return (max(0.0, float(np.cross(r3 - r2, hp - r2) @ N)), max(0.0, float(np.cross(r1 - r3, hp - r3) @ N)),
            max(0.0, float(np.cross(r2 - r1, hp - r1) @ N)))


def _near_integer(x, margin):
    return abs(x - np.round(x)) < margin


def lookup(texels, filt, u, v):
    """(rgb, near a decision) of a (h, w, 3) texture at (u, v): repeat wrap, row 0 at the top, nearest (0) or bilinear (1)"""
    h, w = texels.shape[:2]
    near = _near_integer(u, WRAP_MARGIN) or _near_integer(v, WRAP_MARGIN)
    fu, fv = u - np.floor(u), v - np.floor(v)
    if filt == 0:
        ax, ay = fu * w, (1.0 - fv) * h
        near = near or _near_integer(ax, NEAREST_MARGIN) or _near_integer(ay, NEAREST_MARGIN)
        x, y = min(w - 1, int(np.floor(ax))), min(h - 1, int(np.floor(ay)))
        return texels[y, x].astype(np.float64), bool(near)
    px, py = fu * w - 0.5, (1.0 - fv) * h - 0.5
    x0, y0 = np.floor(px), np.floor(py)
    tx, ty = px - x0, py - y0
    xa, ya = (int(x0) % w + w) % w, (int(y0) % h + h) % h
    xb, yb = (xa + 1) % w, (ya + 1) % h
    t = texels.astype(np.float64)
    top = t[ya, xa] + tx * (t[ya, xb] - t[ya, xa])
    bot = t[yb, xa] + tx * (t[yb, xb] - t[yb, xa])
    return top + ty * (bot - top), bool(near)


def albedo(kd, v, N, hp, uv, texels, filt):
    """(kd', near a decision) at hp on the triangle v (3,3) with record normal N and corner uvs uv (3,2): the pinned formula in float64"""
    a1, a2, a3 = weights(v, N, hp)
    A = a1 + a2 + a3
    if not (0.0 < A < np.inf):
        return np.asarray(kd, dtype=np.float64), True
    uv = np.asarray(uv, dtype=np.float64)
    u = (uv[0, 0] * a1 + uv[1, 0] * a2 + uv[2, 0] * a3) / A
    vv = (uv[0, 1] * a1 + uv[1, 1] * a2 + uv[2, 1] * a3) / A
    tex, near = lookup(texels, filt, u, vv)
    return np.asarray(kd, dtype=np.float64) * tex, near


class TextureModel(S.SmoothModel):
    """smooth_ref.SmoothModel with albedo textures: uvs (n,3,2) as recorded (add order; non-finite where a triangle has none),
    textures = [(texels (h,w,3) of Scene.debug_texture, filter)], mat_tex = {material index: texture index}."""

    def __init__(self, verts, normals, mats, mat_of, cam, vnormals, uvs, textures, mat_tex, env=None, table=None, margin=1e-4):
        super().__init__(verts, normals, mats, mat_of, cam, vnormals, env=env, table=table, margin=margin, uvs=uvs, textures=textures, mat_tex=mat_tex)
