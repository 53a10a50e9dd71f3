"""Float64 numpy model of Scene.render_nee with interiors bound to glass (include/pt_api.h pins the free flight, the absorption factor and
the scatter vertex): tests/medium_ref.py's MediumModel with the interior rule where `inside` is true (the rule itself is stated in tests/path_ref.py's
PathModel, behind the setting `interiors`).  Also
the float64 statements of the pieces that tests/test_interior_host.py checks against a brute-force integration and
tests/test_gpu_interior.py holds pt_debug_interior to.  MediumModel shades types 0 to 4, so a bound material of InteriorModel is of
type 2; InteriorFrostedModel adds the same rule to tests/frosted_ref.py's FrostedModel for a type-6 boundary."""
import numpy as np

import coated_ref as K
import frosted_ref as F
import glossy_ref as G
import lights_ref as L
import medium_ref as M
import nee_ref as R
import smooth_ref as S
from frosted_ref import reflect_terms, terms
from medium_ref import FLIGHT_MARGIN, STREAM, clip, direction, flight, hg, transmittance


def interior_of(d):
    """Scene.material_interior() -> the model's record in float64"""
    return dict(sigma_a=np.asarray(d["sigma_a"], dtype=np.float64), sigma_s=float(d["sigma_s"]), g=float(d["g"]))


def absorb(sigma_a, ell):
    """Beer-Lambert per channel over the length ell"""
    return np.exp(-np.asarray(sigma_a, dtype=np.float64) * ell)


def segment(it, t, u):
    """the interior rule on one segment whose hit is at t, u the free-flight number: (scatters, l, absorption factor)"""
    ell, sc = float(t), False
    if it["sigma_s"] > 0:
        d = flight(it["sigma_s"], u)
        if d < t:
            ell, sc = d, True
    return sc, ell, absorb(it["sigma_a"], ell)


INTERIOR_EVENTS = ("interior_scatter", "interior_absorbed", "interior_exit", "interior_then_light")


class InteriorModel(M.MediumModel):
    """medium_ref.MediumModel plus interiors = {material index: Scene.material_interior(index)}: the interior rule at the top of a segment
    that runs inside a dielectric.  MediumModel shades types 0 to 4, so a bound material is of type 2 here; with no binding, or an all-zero
    one, the model is MediumModel's sample for sample."""

    EVENTS = M.EVENTS + INTERIOR_EVENTS

    def __init__(self, verts, normals, mats, mat_of, cam, lights, medium, interiors, **settings):
        settings.setdefault("events", S.BASE_EVENTS + self.EVENTS)
        super().__init__(verts, normals, mats, mat_of, cam, lights, medium, interiors=interiors, **settings)


class InteriorFrostedModel(F.FrostedModel):
    """frosted_ref.FrostedModel (types 0 to 6, emitters and a sky, no analytic lights and no medium) plus interiors, for a type-6 boundary
    under option frosted.  A binding counts on a material of type 2 or 6 by its type alone, as the device table reads it (with `frosted`
    off a type-6 surface is inert, but a segment inside type-2 glass that ends on it still takes its interior)."""

    def __init__(self, *a, interiors=None, **settings):
        settings.setdefault("events", S.BASE_EVENTS + G.EVENTS + K.COATED_EVENTS + F.FROSTED_EVENTS + INTERIOR_EVENTS)
        super().__init__(*a, interiors=interiors, **settings)
