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


EVENTS = L.EVENTS + ("scatter", "scatter_light", "scatter_delta", "scatter_emitter_wb", "scatter_sky")


class MediumModel(L.LightsModel):
    """lights_ref.LightsModel plus a medium: medium = Scene.medium() (None or sigma_t = 0: the model is LightsModel's); lights =
    Scene.debug_lights(), or None when no set is held."""

    EVENTS = EVENTS

    def __init__(self, verts, normals, mats, mat_of, cam, lights, medium, **settings):
        settings.setdefault("events", S.BASE_EVENTS + EVENTS)
        super().__init__(verts, normals, mats, mat_of, cam, lights, medium=medium, **settings)
