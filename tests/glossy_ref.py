"""Float64 numpy model of Scene.render_nee under option glossy (include/pt_api.h pins the vertex), on top of tests/smooth_ref.py: the
same LCG stream, the same hashes, brute-force intersection, with or without an environment and vertex normals, material types 0-4.  It
shares no code with the library.  vertex() is the rough-metal vertex itself, vectorised and in a chosen precision: float64 is the
reference, float32 the restatement of the pinned sequence that the tests measure their tolerance with."""
import numpy as np

import nee_ref as R
import smooth_ref as S

DEGENERATE_L2 = 1e-9      # Vh this close to the normal: the tangent T1 is rounding noise, float32 may pick any rotation


def roughness(shininess):
    s = float(np.float32(shininess))
    if not np.isfinite(s) or s < 0:
        return 1.0
    return float(np.float32(min(1.0, max(0.03, np.sqrt(2.0 / (s + 2.0))))))


def frame(N):
    """(X, Z) of diffuse_direction for normals N (n, 3), in N's dtype"""
    E = 0.001
    yaxis = (np.abs(N[:, 0]) <= E) & (np.abs(N[:, 2]) <= E)
    other = np.where(yaxis, N[:, 1], N[:, 0])
    rl = 1 / np.sqrt(N[:, 2] * N[:, 2] + other * other)
    zero = np.zeros_like(rl)
    Z = np.where(yaxis[:, None], np.stack([zero, -N[:, 2] * rl, N[:, 1] * rl], 1), np.stack([-N[:, 2] * rl, zero, N[:, 0] * rl], 1))
    return np.cross(N, Z), Z


def dot(a, b):
    return (a * b).sum(axis=1)


def unit(v):
    return v / np.sqrt(dot(v, v))[:, None]


def ggx_D(alpha, h):
    a2 = alpha * alpha
    d = a2 * h[:, 2] ** 2 + (h[:, 0] ** 2 + h[:, 1] ** 2)
    return a2 / (h.dtype.type(np.pi) * (d * d))


def ggx_G1(alpha, v):
    with np.errstate(divide="ignore", invalid="ignore"):
        g = 2 * v[:, 2] / (v[:, 2] + np.sqrt(alpha * alpha * (v[:, 0] ** 2 + v[:, 1] ** 2) + v[:, 2] ** 2))
    return np.where(v[:, 2] > 0, g, 0).astype(v.dtype)


def ggx_pdf(alpha, o, h):
    with np.errstate(divide="ignore", invalid="ignore"):
        p = ggx_G1(alpha, o) * ggx_D(alpha, h) / (4 * o[:, 2])
    return np.where(o[:, 2] > 0, p, 0).astype(o.dtype)


def ggx_pdf_of(alpha, o, w):
    h = unit(o + w)
    return ggx_pdf(alpha, o, h), h


def schlick(F0, h, o):
    c = np.abs(dot(h, o))
    return F0 + (1 - F0) * ((1 - c) ** 5)[:, None]


def local(v, X, Z, N):
    return np.stack([dot(v, X), dot(v, Z), dot(v, N)], 1)


def vertex(N, D, alpha, rnd1, rnd2, F0, dtype=np.float64):
    """The sampled vertex for n items: N, D (n, 3), alpha, rnd1, rnd2 (n,), F0 (n, 3) or (3,), all first rounded to float32 (the values the
    device gets) and then evaluated in `dtype`.  Returns a dict of arrays."""
    f = lambda a: np.asarray(a, dtype=np.float32).astype(dtype)
    N, D, alpha, rnd1, rnd2 = f(N), f(D), f(alpha), f(rnd1), f(rnd2)
    F0 = np.broadcast_to(f(F0), N.shape)
    X, Z = frame(N)
    o = local(-D, X, Z, N)
    Vh = unit(np.stack([alpha * o[:, 0], alpha * o[:, 1], o[:, 2]], 1))
    l2 = Vh[:, 0] ** 2 + Vh[:, 1] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sqrt(l2)
        T1 = np.where((l2 > 0)[:, None], np.stack([-Vh[:, 1] / s, Vh[:, 0] / s, np.zeros_like(s)], 1), np.array([1, 0, 0], dtype=dtype))
    T2 = np.cross(Vh, T1)
    r = np.sqrt(rnd1)
    theta = (2.0 * np.pi * rnd2.astype(np.float64)).astype(np.float32).astype(np.float64)      # the float angle, as the device rounds it
    sn, cs = np.sin(theta).astype(dtype), np.cos(theta).astype(dtype)
    t1, t2 = r * cs, r * sn
    q = dtype(0.5) * (1 + Vh[:, 2])
    t2 = (1 - q) * np.sqrt(np.maximum(1 - t1 * t1, 0)) + q * t2
    t3 = np.sqrt(np.maximum(1 - t1 * t1 - t2 * t2, 0))
    Nh = T1 * t1[:, None] + T2 * t2[:, None] + Vh * t3[:, None]
    h = unit(np.stack([alpha * Nh[:, 0], alpha * Nh[:, 1], np.maximum(Nh[:, 2], 0)], 1))
    w = h * (2 * dot(o, h))[:, None] - o
    world = X * w[:, 0:1] + N * w[:, 2:3] + Z * w[:, 1:2]
    pb = ggx_pdf(alpha, o, h)
    g1w = ggx_G1(alpha, w)
    F = schlick(F0, h, o)
    pb_again, _ = ggx_pdf_of(alpha, o, local(unit(world), X, Z, N))
    return dict(world=world, w=w, h=h, o=o, pb=pb, g1w=g1w, F=F, g=F * g1w[:, None], pb_again=pb_again, l2=l2, X=X, Z=Z)


def debug_columns(v):
    """vertex()'s result in the layout of pt_debug_glossy: (n, 8)"""
    return np.concatenate([v["world"], v["pb"][:, None], v["g1w"][:, None], v["F"][:, 0:1], v["pb_again"][:, None], v["o"][:, 2:3]], 1)


COLUMNS = ("direction", "p_b sampled", "G1(w)", "F.x", "p_b again", "o.z")


def column_errors(got, want):
    """Relative errors per item, (n, 6) in the order of COLUMNS, of pt_debug_glossy's layout: the direction as a vector (|got - want| /
    |want|), the others |got - want| / |want|; where G1(w) is 0 in `want` (w.z <= 0) the entry is |got| itself."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    out = np.zeros((len(want), 6))
    out[:, 0] = np.linalg.norm(got[:, :3] - want[:, :3], axis=1) / np.linalg.norm(want[:, :3], axis=1)
    for k, c in ((1, 3), (2, 4), (3, 5), (4, 6), (5, 7)):
        d = np.abs(got[:, c] - want[:, c])
        den = np.abs(want[:, c])
        out[:, k] = np.where(den > 0, d / np.where(den > 0, den, 1.0), d)
    return out


EVENTS = ("glossy_vertex", "glossy_end_wz", "glossy_end_ng", "glossy_light", "glossy_emitter_wb", "glossy_sky")


class GlossyModel(S.SmoothModel):
    """smooth_ref.SmoothModel with material type 4 shaded as the rough metal (glossy = False: inert, as without the option)."""

    EVENTS = EVENTS

    def __init__(self, *a, glossy=True, **settings):
        settings.setdefault("events", S.BASE_EVENTS + EVENTS)
        super().__init__(*a, glossy=glossy, **settings)
