"""Float64 numpy model of Scene.render_nee under option coated (include/pt_api.h pins the vertex), on top of tests/glossy_ref.py: the
GlossyModel with material type 5 shaded as a diffuse base under a rough dielectric coat.  It shares no code with the library.  vertex()
is the coated vertex itself, vectorised and in a chosen precision: float64 is the reference, float32 the restatement of the pinned
sequence that the tests measure their tolerances with."""
import numpy as np

import glossy_ref as G
import nee_ref as R
import smooth_ref as S


def schlick_c(F0, c):
    """F(c): Schlick on |c|, F0 (n, 3), c (n,)"""
    return F0 + (1 - F0) * ((1 - np.abs(c)) ** 5)[:, None]


def lobe_probability(F0, kd, oz):
    """ps: the probability of the coat lobe"""
    Fo = schlick_c(F0, oz)
    three = oz.dtype.type(3)
    fm = ((Fo[:, 0] + Fo[:, 1]) + Fo[:, 2]) / three
    km = ((kd[:, 0] + kd[:, 1]) + kd[:, 2]) / three
    s = (1 - fm) * km + fm
    with np.errstate(divide="ignore", invalid="ignore"):
        ps = np.where(s > 0, fm / np.where(s > 0, s, 1), oz.dtype.type(0.5))
    return np.clip(ps, oz.dtype.type(0.1), oz.dtype.type(0.9)).astype(oz.dtype)


def evaluate(alpha, F0, kd, ps, o, h, w):
    """(p_b, g, spec, diff) of local directions w (n, 3) with half vectors h: the mixture density and the weight (spec + diff) / p_b"""
    t = o.dtype.type
    pg = G.ggx_pdf(alpha, o, h)
    c = np.maximum(w[:, 2], 0)
    pb = ps * pg + ((1 - ps) * c) * t(1 / np.pi)
    spec = G.schlick(F0, h, o) * (G.ggx_G1(alpha, w) * pg)[:, None]
    diff = ((1 - schlick_c(F0, o[:, 2])) * (1 - schlick_c(F0, c))) * kd * (c * (c * t(1 / np.pi)))[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where((pb > 0)[:, None], (spec + diff) / np.where(pb > 0, pb, 1)[:, None], 0).astype(o.dtype)
    return pb.astype(o.dtype), g, spec, diff


def evaluate_of(alpha, F0, kd, o, w):
    """evaluate() for given unit directions w, the way a light sample does it: ps and h = normalize(o + w) from scratch"""
    return evaluate(alpha, F0, kd, lobe_probability(F0, kd, o[:, 2]), o, G.unit(o + w), w)


def vertex(N, D, alpha, F0, kd, rnd1, rnd2, u_sel, dtype=np.float64):
    """The sampled vertex for n items: N, D (n, 3), alpha, rnd1, rnd2, u_sel (n,), F0 and kd (n, 3) or (3,), all first rounded to float32
    (the values the device gets) and then evaluated in `dtype`.  Returns a dict of arrays."""
    f = lambda a: np.asarray(a, dtype=np.float32).astype(dtype)
    N, D, alpha, rnd1, rnd2, u_sel = f(N), f(D), f(alpha), f(rnd1), f(rnd2), f(u_sel)
    F0 = np.broadcast_to(f(F0), N.shape)
    kd = np.broadcast_to(f(kd), N.shape)
    gv = G.vertex(N, D, alpha, rnd1, rnd2, F0, dtype=dtype)       # the coat lobe's draw: visible normals on the disc point of rnd1, rnd2
    X, Z, o = gv["X"], gv["Z"], gv["o"]
    ps = lobe_probability(F0, kd, o[:, 2])
    coat = u_sel < ps
    r = np.sqrt(rnd1)
    theta = (2.0 * np.pi * rnd2.astype(np.float64)).astype(np.float32).astype(np.float64)
    sn, cs = np.sin(theta).astype(dtype), np.cos(theta).astype(dtype)
    base = np.stack([r * cs, r * sn, np.sqrt(1 - rnd1)], 1)         # the base lobe's: diffuse_direction's cosine lobe
    w = np.where(coat[:, None], gv["w"], base)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = np.where(coat[:, None], gv["h"], G.unit(o + base))
    world = X * w[:, 0:1] + N * w[:, 2:3] + Z * w[:, 1:2]
    pb, g, spec, diff = evaluate(alpha, F0, kd, ps, o, h, w)
    pb_again, g_again, _, _ = evaluate_of(alpha, F0, kd, o, G.local(G.unit(world), X, Z, N))
    return dict(world=world, w=w, h=h, o=o, ps=ps, coat=coat, pb=pb, g=g, pb_again=pb_again, g_again=g_again, l2=gv["l2"], X=X, Z=Z)


def debug_columns(v):
    """vertex()'s result in the layout of pt_debug_coated: (n, 10)"""
    return np.concatenate([v["world"], v["ps"][:, None], v["coat"].astype(v["world"].dtype)[:, None], v["pb"][:, None], v["g"][:, 0:1], v["pb_again"][:, None],
                           v["g_again"][:, 0:1], v["o"][:, 2:3]], 1)


COLUMNS = ("direction", "ps", "p_b sampled", "g.x sampled", "p_b again", "g.x again", "o.z")
COLUMN_INDEX = (3, 5, 6, 7, 8, 9)      # where COLUMNS[1:] sit in the layout of pt_debug_coated


def column_errors(got, want):
    """Relative errors per item, (n, 7) in the order of COLUMNS: the direction as a vector, the others |got - want| / |want| (|got| itself
    where `want` is 0).  The lobe column is compared separately (it is a decision, not a value)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    out = np.zeros((len(want), 7))
    out[:, 0] = np.linalg.norm(got[:, :3] - want[:, :3], axis=1) / np.linalg.norm(want[:, :3], axis=1)
    for k, c in enumerate(COLUMN_INDEX):
        d = np.abs(got[:, c] - want[:, c])
        den = np.abs(want[:, c])
        out[:, k + 1] = np.where(den > 0, d / np.where(den > 0, den, 1.0), d)
    return out


COATED_EVENTS = ("coated_coat", "coated_base", "coated_end_wz", "coated_end_ng", "coated_light", "coated_emitter_wb", "coated_sky")


class CoatedModel(G.GlossyModel):
    """glossy_ref.GlossyModel with material type 5 shaded as the coated diffuse (coated = False: inert, as without the option).  ps_margin:
    a lobe choice whose |u_sel - ps| is below it is a near tie (the float32 restatement's error of ps)."""

    COATED_EVENTS = COATED_EVENTS

    def __init__(self, *a, coated=True, ps_margin=1e-5, **settings):
        settings.setdefault("events", S.BASE_EVENTS + G.EVENTS + COATED_EVENTS)
        super().__init__(*a, coated=coated, ps_margin=ps_margin, **settings)
