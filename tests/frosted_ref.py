"""Float64 numpy model of Scene.render_nee under option frosted (include/pt_api.h pins the vertex), on top of tests/coated_ref.py: the
CoatedModel with material type 6 shaded as a rough dielectric (GGX reflection and refraction through one visible-normal half vector) and
the `inside` flag it toggles.  It shares no code with the library.  vertex() is the frosted vertex itself, vectorised and in a chosen
precision: float64 is the reference, float32 the restatement of the pinned sequence that the tests measure their tolerances with."""
import numpy as np

import coated_ref as K
import glossy_ref as G
import nee_ref as R
import smooth_ref as S


def terms(F0, eta, o, h):
    """(c, F, disc, Fm, tir) at half vectors h: Schlick, type 2's discriminant, the mean; total internal reflection makes F and Fm 1"""
    t = o.dtype.type
    c = G.dot(o, h)
    F = G.schlick(F0, h, o)
    disc = 1 - ((1 - c * c) / eta) / eta
    Fm = ((F[:, 0] + F[:, 1]) + F[:, 2]) / t(3)
    tir = disc <= 0
    Fm = np.where(tir, t(1), Fm).astype(o.dtype)
    F = np.where(tir[:, None], t(1), F).astype(o.dtype)
    return c, F, disc, Fm, tir


def mirrored(w):
    return np.stack([w[:, 0], w[:, 1], -w[:, 2]], 1)


def reflect_terms(alpha, F0, eta, o, h, w):
    """(p_b, g) of reflected directions w with half vectors h"""
    c, F, disc, Fm, _ = terms(F0, eta, o, h)
    pb = Fm * G.ggx_pdf(alpha, o, h)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = F * (G.ggx_G1(alpha, w) / Fm)[:, None]
    return pb.astype(o.dtype), g.astype(o.dtype)


def refract_half(eta, o, w):
    """the half vector (h.z >= 0) that refracts o into w, and whether the pair is one: o.h > 0 > w.h"""
    h = G.unit(o + w * np.reshape(eta, (-1, 1)))
    h = np.where((h[:, 2] < 0)[:, None], -h, h)
    return h, (G.dot(o, h) > 0) & (G.dot(w, h) < 0)


def refract_density(alpha, F0, eta, o, w):
    """the density of refracted directions w (w.z < 0), which only the model needs: (1 - Fm) G1(o) D(h) (o.h) / o.z x
    eta^2 |w.h| / (o.h + eta w.h)^2; and the weight g(w) = (1 - F) G1(w mirrored) / (1 - Fm)"""
    h, ok = refract_half(eta, o, w)
    c, F, disc, Fm, tir = terms(F0, eta, o, h)
    wh = G.dot(w, h)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = (1 - Fm) * G.ggx_G1(alpha, o) * G.ggx_D(alpha, h) * c / o[:, 2] * eta * eta * np.abs(wh) / (c + eta * wh) ** 2
        g = (1 - F) * (G.ggx_G1(alpha, mirrored(w)) / (1 - Fm))[:, None]
    ok = ok & ~tir & (w[:, 2] < 0) & (o[:, 2] > 0)
    return np.where(ok, p, 0.0), np.where(ok[:, None], g, 0.0)


def evaluate_of(alpha, F0, eta, o, w):
    """(p, g) of given unit directions w in both hemispheres: above the surface the reflection lobe the way a light sample evaluates it
    (h = normalize(o + w) and the terms from scratch), below it the refraction lobe's density and weight"""
    up = w[:, 2] > 0
    wu = np.where(up[:, None], w, mirrored(w))
    pr, gr = reflect_terms(alpha, F0, eta, o, G.unit(o + wu), wu)
    pt, gt = refract_density(alpha, F0, eta, o, np.where(up[:, None], mirrored(w), w))
    return np.where(up, pr, pt), np.where(up[:, None], gr, gt)


def vertex(N, D, alpha, F0, eta, rnd1, rnd2, u_sel, dtype=np.float64):
    """The sampled vertex for n items: N, D (n, 3), alpha, eta, rnd1, rnd2, u_sel (n,), F0 (n, 3) or (3,), all first rounded to float32 (the
    values the device gets) and then evaluated in `dtype`.  Returns a dict of arrays."""
    f = lambda a: np.asarray(a, dtype=np.float32).astype(dtype)
    N, D, alpha, eta, rnd1, rnd2, u_sel = f(N), f(D), f(alpha), f(eta), f(rnd1), f(rnd2), f(u_sel)
    F0 = np.broadcast_to(f(F0), N.shape)
    gv = G.vertex(N, D, alpha, rnd1, rnd2, F0, dtype=dtype)       # the half vector: visible normals on the disc point of rnd1, rnd2
    X, Z, o, h = gv["X"], gv["Z"], gv["o"], gv["h"]
    c, F, disc, Fm, tir = terms(F0, eta, o, h)
    refl = u_sel < Fm
    with np.errstate(invalid="ignore"):
        wt = h * (c / eta - np.sqrt(np.where(disc > 0, disc, 0)))[:, None] - o / eta[:, None]
    w = np.where(refl[:, None], gv["w"], wt)
    world = X * w[:, 0:1] + N * w[:, 2:3] + Z * w[:, 1:2]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(refl[:, None], F * (G.ggx_G1(alpha, w) / Fm)[:, None], (1 - F) * (G.ggx_G1(alpha, mirrored(w)) / (1 - Fm))[:, None]).astype(dtype)
    pb = np.where(refl, Fm * G.ggx_pdf(alpha, o, h), 0).astype(dtype)
    wl = G.local(G.unit(world), X, Z, N)
    pb2, g2 = reflect_terms(alpha, F0, eta, o, G.unit(o + wl), wl)
    pb_again = np.where(refl, pb2, 0).astype(dtype)
    g_again = np.where(refl[:, None], g2, 0).astype(dtype)
    return dict(world=world, w=w, h=h, o=o, Fm=Fm, refl=refl, pb=pb, g=g, pb_again=pb_again, g_again=g_again, l2=gv["l2"], X=X, Z=Z, c=c, disc=disc,
                tir=tir)


def debug_columns(v):
    """vertex()'s result in the layout of pt_debug_frosted: (n, 10)"""
    return np.concatenate([v["world"], v["Fm"][:, None], v["refl"].astype(v["world"].dtype)[:, None], v["pb"][:, None], v["g"][:, 0:1], v["pb_again"][:, None],
                           v["g_again"][:, 0:1], v["o"][:, 2:3]], 1)


COLUMNS = ("direction", "Fm", "p_b sampled", "g.x sampled", "p_b again", "g.x again", "o.z")
COLUMN_INDEX = (3, 5, 6, 7, 8, 9)      # where COLUMNS[1:] sit in the layout of pt_debug_frosted
column_errors = K.column_errors        # (the same layout: direction, a scalar, the lobe flag, four values, o.z)


FROSTED_EVENTS = ("frosted_reflect", "frosted_refract", "frosted_tir", "frosted_inside", "frosted_end_wz", "frosted_end_ng", "frosted_light",
                  "frosted_emitter_wb", "frosted_sky", "frosted_through_emitter", "frosted_through_sky")


class FrostedModel(K.CoatedModel):
    """coated_ref.CoatedModel with material type 6 shaded as the rough dielectric (frosted = False: inert, as without the option) and the
    `inside` flag a refraction toggles.  fm_margin: a lobe choice whose |u_sel - Fm|, or a discriminant whose |disc|, is below it is a
    near tie (the float32 restatement's error of them)."""

    FROSTED_EVENTS = FROSTED_EVENTS

    def __init__(self, *a, frosted=True, fm_margin=1e-5, **settings):
        settings.setdefault("events", S.BASE_EVENTS + G.EVENTS + K.COATED_EVENTS + FROSTED_EVENTS)
        super().__init__(*a, frosted=frosted, fm_margin=fm_margin, **settings)
