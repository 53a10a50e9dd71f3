"""A numpy restatement of the area lights of render_nee (include/pt_api.h): the table as pt_set_area_lights builds it,
and the sample and hit functions of the kernel, each in a precision f of the caller's choice (float64: the reference; float32: the same
formulas in the device's precision, whose distance from float64 is the rounding spread the GPU test's tolerance is built from).  The hit
function reports its decisions' margins (sphere-hit discriminants and distances, sun-disc cosines) so that a test can refuse items whose
outcome a rounding could flip.  AreaLightsModel, below, is the float64 path model: medium_ref.MediumModel (lights_ref.LightsModel plus a medium) with the area set added."""

import numpy as np

SPHERE, SUN = 0, 1


def table(lights):
    """lights: api.AreaLight structures as given to set_area_lights -> order, records (n, 12) float32, cdf, P_light, weights (float64)"""
    n = len(lights)
    order = [i for i, l in enumerate(lights) if l.type == SPHERE] + [i for i, l in enumerate(lights) if l.type == SUN]
    rec = np.zeros((n, 12), dtype=np.float32)
    w = np.zeros(n)
    for k, i in enumerate(order):
        l = lights[i]
        L = np.array(list(l.radiance), dtype=np.float64)
        s = (L[0] + L[1]) + L[2]
        if l.type == SPHERE:
            rec[k, :3] = list(l.position)
            rec[k, 3] = l.size
            auto = s * (4.0 * np.pi * np.pi) * (float(l.size) * float(l.size))
        else:
            d = np.array(list(l.direction), dtype=np.float64)
            rec[k, :3] = -d / np.sqrt((d * d).sum())
            q = 2.0 * np.sin(0.5 * float(l.size)) ** 2
            rec[k, 3] = np.cos(float(l.size))
            rec[k, 8] = q
            auto = s * (2.0 * np.pi) * q
        rec[k, 4:7] = L
        w[k] = float(l.weight) if l.weight > 0 else auto
        if s == 0.0 or not np.isfinite(w[k]):
            w[k] = 0.0
    total = w.sum()
    any_ = total > 0 and np.isfinite(total)
    last = int(np.nonzero(w > 0)[0].max()) if any_ else 0
    cdf = np.zeros(n, dtype=np.float32)
    run = 0.0
    for k in range(n):
        run += w[k] if any_ else 1.0
        cdf[k] = 1.0 if (k >= last or k + 1 == n) else np.float32(run / (total if any_ else n))
    upto = np.ceil(cdf.astype(np.float64) * 2 ** 24)
    pl = (np.diff(np.concatenate([[0.0], upto])) / 2 ** 24).astype(np.float32) if any_ else np.zeros(n, dtype=np.float32)
    rec[:, 7] = pl
    return {"order": np.asarray(order, dtype=np.int32), "records": rec, "cdf": cdf, "P_light": pl, "weights": w}


def cone_density(q):
    return 1.0 / (2.0 * np.pi * q)


def _dot(a, b, f):
    return f(a[0] * b[0] + a[1] * b[1] + a[2] * b[2])


def tangent_frame(N, f):
    """prog.cl:205-212 as the kernel's tangent_frame states it"""
    E = f(0.001)
    yaxis = abs(N[0]) <= E and abs(N[2]) <= E
    other = N[1] if yaxis else N[0]
    rl = f(1) / np.sqrt(f(N[2] * N[2] + other * other))
    Z = np.array([f(0), -N[2] * rl, N[1] * rl], dtype=f) if yaxis else np.array([-N[2] * rl, f(0), N[0] * rl], dtype=f)
    X = np.cross(N, Z).astype(f)
    return Z, X


def cone_direction(A, q, u1, u2, f):
    A = np.asarray(A, dtype=f)
    q, u1, u2 = f(q), f(u1), f(u2)
    c = f(1) - u1 * q
    s = np.sqrt(max(f(0), f(1) - c * c))
    phi = f(2 * np.pi) * u2
    Z, X = tangent_frame(A, f)
    return (A * c + (Z * (s * np.sin(phi)) + X * (s * np.cos(phi)))).astype(f)


def sphere_q(C, R, o, f):
    c = np.asarray(C, dtype=f) - np.asarray(o, dtype=f)
    d2, R2 = _dot(c, c, f), f(R) * f(R)
    if not (np.isfinite(d2) and d2 > R2):
        return None, c, d2, R2
    s2 = R2 / d2
    cm = np.sqrt(max(f(0), f(1) - s2))
    return s2 / (f(1) + cm), c, d2, R2


def sphere_sample(C, R, o, u1, u2, f):
    """-> None (rejected) or (w, p_omega, t_s)"""
    q, c, d2, R2 = sphere_q(C, R, o, f)
    if q is None or not q > 0:
        return None
    w = cone_direction(c / np.sqrt(d2), q, u1, u2, f)
    b = _dot(c, w, f)
    return w, f(1) / (f(2 * np.pi) * q), b - np.sqrt(max(f(0), b * b - (d2 - R2)))


def sun_sample(axis, q, u1, u2, f):
    return cone_direction(axis, q, u1, u2, f), f(1) / (f(2 * np.pi) * f(q)), f(np.inf)


def sphere_hit(spheres, o, d, tmax, f):
    """spheres: [(C, R)] -> (index or -1, t, margins): margins lists, per sphere, the relative distance of each decision from its other outcome
    (outside / inside, the discriminant's sign, t against 0 and against the best so far)"""
    best, bt, margins = -1, f(tmax), []
    o, d = np.asarray(o, dtype=f), np.asarray(d, dtype=f)
    for j, (C, R) in enumerate(spheres):
        c = np.asarray(C, dtype=f) - o
        d2, b, R2 = _dot(c, c, f), _dot(c, d, f), f(R) * f(R)
        disc = b * b - (d2 - R2)
        t = b - np.sqrt(max(f(0), disc))
        margins.append((abs(d2 - R2) / R2, abs(disc) / max(b * b, R2), abs(t - bt) / max(abs(bt), abs(t)) if np.isfinite(bt) else 1.0))
        if d2 > R2 and disc >= 0 and t > 0 and t < bt:
            best, bt = j, t
    return best, bt, margins


def sun_mask(suns, d, f):
    """suns: [(axis, cos a)] -> (mask, margins |cos - cos a|)"""
    mask, margins = 0, []
    for s, (axis, ca) in enumerate(suns):
        c = _dot(np.asarray(d, dtype=f), np.asarray(axis, dtype=f), f)
        margins.append(abs(float(c) - float(ca)))
        if c >= f(ca):
            mask |= 1 << s
    return mask, margins


# ---------------------------------------------------------------------------- the path model
import medium_ref as M          # noqa: E402

EVENTS = M.EVENTS + ("sphere_end", "sphere_end_rough", "sphere_end_scatter", "sun_miss", "area_sample", "area_glossy", "area_ng_reject", "sphere_blocks")


class AreaLightsModel(M.MediumModel):
    """medium_ref.MediumModel (lights_ref.LightsModel plus a medium; medium = None: LightsModel itself) plus an area set, area =
    Scene.debug_area_lights(): the area branch in front of every other light sample and 1 - P_area on their p_l, the spheres as the end of
    a segment -- cut before the free flight -- and as blockers of every shadow ray, and the suns on a miss."""

    EVENTS = EVENTS

    def __init__(self, verts, normals, mats, mat_of, cam, lights, area, medium=None, **settings):
        settings.setdefault("events", M.S.BASE_EVENTS + EVENTS)
        super().__init__(verts, normals, mats, mat_of, cam, lights, medium, area=area, **settings)
