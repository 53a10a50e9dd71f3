"""The rough dielectric of option frosted on host-only contexts (the option and its refusals, pt_debug_frosted's argument checks,
scenes.cornell_box(frosted=True); include/pt_api.h) and the float64 model of the vertex (tests/frosted_ref.py) by quadrature: no device
needed."""

import os

import numpy as np
import pytest

import frosted_ref as F
import glossy_ref as G

# (the library is imported inside the tests, through conftest's `api` fixture: importing it while the modules are collected would load it
# before tests/test_distributed_gloo.py imports torch, and the library must bind to the HIP runtime torch loaded -- see bench.py)

NEW_SYMBOLS = ["pt_debug_frosted"]


def test_abi_has_the_new_symbol(api):
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTS and hasattr(api.LIB, name)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pt_api.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header


def host_scene(api, spec=None):
    from opencl_path_tracer_amd import scenes
    sc = api.Scene(16, 16, device=-1)
    spec = spec or scenes.cornell_box(8, 4, frosted=True)
    for m in spec.materials:
        sc.add_Material(*m)
    for verts, mati in spec.objects:
        sc.add_Triangles(api.triangles_from_vertices(verts, mati))
        sc.end_Obj()
    sc.upload_Triangles()
    sc.upload_Materials()
    return sc


def test_option_round_trips_and_refuses_2(api):
    sc = host_scene(api)
    sc.set_option("frosted", 1)
    sc.set_option("frosted", 0)
    for bad in (2, -1):
        with pytest.raises(api.PtError) as e:
            sc.set_option("frosted", bad)
        assert e.value.code == api.PT_EINVAL and "frosted" in str(e.value)
    # the options before it keep their contracts and their texts
    with pytest.raises(api.PtError) as e:
        sc.set_option("coated", 2)
    assert "coated must be 0 (material type 5 is inert)" in str(e.value)


def test_host_records_of_a_type_6_material_stay_as_added(api):
    """alpha = pt_material_roughness(shininess) goes into field shininess of the DEVICE copy only (a host-only context has none: what the
    device reads is checked by the float64 replay of tests/test_gpu_frosted.py, whose model takes alpha from the shininess and the index of
    refraction from n); the host records stay what was added, with type 2's n and F0."""
    from opencl_path_tracer_amd import scenes
    spec = scenes.cornell_box(8, 4, frosted=True)
    p = len(spec.materials) - 1
    sc = host_scene(api, spec)
    _, mats, _ = sc.debug_scene()
    want = api.Material(*spec.materials[p])
    glass = api.Material(*scenes.BUILTIN_MATERIALS[scenes.GLASS])
    assert int(mats["type"][p]) == 6 and mats[p].tobytes() == want[0].tobytes()
    assert mats["n"][p] == glass["n"][0] and mats["F0"][p].tobytes() == glass["F0"][0].tobytes()
    assert float(mats["shininess"][p]) == 30.0
    assert np.float32(api.material_roughness(30.0)) == np.float32(G.roughness(30.0)) == np.float32(0.25)


def test_refusals_come_before_the_device_check(api):
    sc = host_scene(api)
    sc.iterations = 4
    calls = (lambda: sc.render(1), lambda: sc.trace_rays(), lambda: sc.generate_rays(), lambda: sc.render_adaptive(2, 4, 0.1),
             lambda: sc.render_adaptive(2, 4, 0.1, path="render"))
    sc.set_option("frosted", 1)
    for call in calls:
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_EINVAL and "frosted" in str(e.value)
    # the NEE paths do not refuse: a host-only context has no device for them
    for call in (lambda: sc.render_nee(1, "mis"), lambda: sc.render_adaptive(2, 4, 0.1, path="nee", metric="half")):
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_ENODEVICE
    sc.set_option("frosted", 0)
    for call in calls:
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_ENODEVICE


def test_debug_frosted_argument_checks(api):
    sc = host_scene(api)
    with pytest.raises(api.PtError) as e:
        sc.debug_frosted(np.zeros((1, 12), dtype=np.float32))
    assert e.value.code == api.PT_ENODEVICE                    # host-only context: the device check comes first
    assert api.LIB.pt_debug_frosted(None, 1, None, None) == api.PT_EINVAL
    with pytest.raises(ValueError):
        sc.debug_frosted(np.zeros((1, 9), dtype=np.float32))   # 12 floats per item


def test_cornell_box_frosted_has_exactly_one_type_6_material(api):
    from opencl_path_tracer_amd import scenes
    plain, spec = scenes.cornell_box(8, 4), scenes.cornell_box(8, 4, frosted=True)
    types = [m[6] for m in spec.materials]
    assert types.count(6) == 1 and [m[6] for m in plain.materials].count(6) == 0
    p = types.index(6)
    assert spec.materials[:len(plain.materials)] == plain.materials and p == len(plain.materials)
    assert tuple(spec.materials[p][:5]) == tuple(scenes.BUILTIN_MATERIALS[scenes.GLASS][:5]) and spec.materials[p][5] == 30.0
    # the glass sphere, and only it, wears it
    assert (spec.objects[2][1] == p).all() and not (spec.objects[0][1] == p).any() and not (spec.objects[1][1] == p).any()
    for (v, _), (pv, _) in zip(spec.objects, plain.objects):
        assert np.array_equal(v, pv)
    with pytest.raises(ValueError):
        scenes.cornell_box(8, 4, coated=True, frosted=True)


# ---------------------------------------------------------------------------- the model alone, by quadrature
def sphere_half(n_mu, n_phi, lo=0.0, hi=1.0):
    """Gauss-Legendre in cos(theta) over [lo, hi] x the midpoint rule in phi (as test_gpu_coated.coated_quadrature): directions (n, 3) of the
    upper hemisphere, weights"""
    x, wt = np.polynomial.legendre.leggauss(n_mu)
    mu, wt = lo + (hi - lo) * 0.5 * (x + 1.0), (hi - lo) * 0.5 * wt
    phi = (np.arange(n_phi) + 0.5) * 2.0 * np.pi / n_phi
    s = np.sqrt(1.0 - mu * mu)
    w = np.stack([np.outer(s, np.cos(phi)), np.outer(s, np.sin(phi)), np.outer(mu, np.ones(n_phi))], -1).reshape(-1, 3)
    return w, np.outer(wt, np.full(n_phi, 2.0 * np.pi / n_phi)).reshape(-1)


def frosted_integrals(alpha, eta, oz, n_mu, n_phi, F0=0.04):
    """For o = (sqrt(1 - oz^2), 0, oz): (the integral of the model's density over the sphere of directions w -- the reflection lobe above,
    the refraction lobe below the surface --, the mass of the sampled directions that stay in their hemisphere, I(o) = the integral of
    g(w) p(w) over the sphere, the visible-normal density's own integral).  The second and fourth are integrals over the HALF vector h of
    the visible-normal density G1(o) D(h) (o.h) / o.z: each h reflects with probability Fm(h) and refracts with 1 - Fm(h), and the
    direction it gives stays or leaves.  The first and third run over w itself, so their agreement with the second is what checks the two
    Jacobians, 1 / (4 o.h) and eta^2 |w.h| / (o.h + eta w.h)^2.  cos(theta_h) is split at the lobe's width; the grid over w is simply fine."""
    a, e = np.array([alpha]), np.array([eta])
    o1 = np.array([[np.sqrt(1.0 - oz * oz), 0.0, oz]])
    cut = 1.0 / np.sqrt(1.0 + (8.0 * alpha) ** 2)              # tan(theta_h) = 8 alpha
    total = kept = 0.0
    for lo, hi in ((0.0, cut), (cut, 1.0)):
        h, wq = sphere_half(n_mu, n_phi, lo, hi)
        o = np.broadcast_to(o1, h.shape)
        F0v = np.full(h.shape, F0)
        c, Fr, disc, Fm, tir = F.terms(F0v, e, o, h)
        vis = G.ggx_G1(a, o) * G.ggx_D(a, h) * np.maximum(c, 0.0) / oz * wq
        wr = h * (2.0 * c)[:, None] - o
        wt = h * (c / eta - np.sqrt(np.maximum(disc, 0.0)))[:, None] - o / eta
        total += float(vis.sum())
        kept += float((vis * (Fm * (wr[:, 2] > 0) + (1.0 - Fm) * (wt[:, 2] < 0))).sum())
    # over w: the reflection lobe is centred on the mirror direction of o, the refraction lobe on the refracted one; the polar split
    # follows the lobe's elevation only loosely, so the grid is simply fine
    dens = energy = 0.0
    for sign in (1.0, -1.0):
        w, wq = sphere_half(n_mu, n_phi)
        w = w * np.array([1.0, 1.0, sign])
        o = np.broadcast_to(o1, w.shape)
        p, g = F.evaluate_of(a, np.full(w.shape, F0), e, o, w)
        dens += float((p * wq).sum())
        energy += float((np.where(p > 0, g[:, 0], 0.0) * p * wq).sum())
    return dens, kept, energy, total


QUAD_CASES = [(alpha, eta, oz) for alpha in (0.1, 0.5) for eta in (1.5, 1.0 / 1.5) for oz in (0.2, 0.5, 0.8, 1.0)]


def test_reflected_plus_refracted_density_integrates_to_the_kept_mass():
    """The model's reflected plus refracted density integrates over the sphere to 1 minus the mass of the sampled directions that leave
    their hemisphere, and I(o), the integral of g p, never exceeds 1 (no energy gain), for alpha in {0.1, 0.5} x eta in {1.5, 1 / 1.5} x
    o.z in {0.2, 0.5, 0.8, 1}.
    Convergence of the quadrature itself, measured on the CPU: between the 256 x 512 grid used here and a 384 x 768 one the density's
    integral moves by at most 1.63e-3 (CONV_DENSITY) and the kept mass by at most 1.32e-3 (CONV_KEPT) over these cases (the kept mass has indicator functions
    in its integrand, so it converges like the cell size); the residual |density - kept| is bounded by 4 x their sum, 1.24e-2 (the largest residual measured is 1.03e-3).  The visible-normal
    density integrates to 1 within 1e-3 (asserted): that is what says the grid resolves the lobe of alpha = 0.1."""
    worst = 0.0
    for alpha, eta, oz in QUAD_CASES:
        dens, kept, energy, total = frosted_integrals(alpha, eta, oz, 256, 512)
        assert abs(total - 1.0) < 1e-3, (alpha, eta, oz, total)
        assert kept <= total + 1e-12
        worst = max(worst, abs(dens - kept))
        assert abs(dens - kept) <= 4.0 * (CONV_DENSITY + CONV_KEPT), (alpha, eta, oz, dens, kept)
        assert energy <= 1.0 and energy <= kept + 4.0 * (CONV_DENSITY + CONV_KEPT), (alpha, eta, oz, energy)
    print("largest |density - kept mass| %.3g (bound %.3g)" % (worst, 4.0 * (CONV_DENSITY + CONV_KEPT)))


CONV_DENSITY = 1.7e-3      # measured on the CPU: 256 x 512 against 384 x 768, the largest change over QUAD_CASES (1.63e-3)
CONV_KEPT = 1.4e-3         # (1.32e-3)


def test_total_internal_reflection_cone_reflects_with_fm_1():
    """eta = 1 / 1.5: half vectors with 1 - (1 - c^2) / eta^2 <= 0, c = o.h below sqrt(1 - eta^2) = 0.745, reflect with Fm = 1 and
    F = (1, 1, 1), whatever u_sel in [0, 1) is; above the critical angle Fm is Schlick's mean, below 1."""
    rng = np.random.default_rng(11)
    n = 2048
    N = np.tile([0.0, 0.0, 1.0], (n, 1))
    oz = rng.uniform(0.05, 1.0, n)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    s = np.sqrt(1.0 - oz * oz)
    D = -np.stack([s * np.cos(phi), s * np.sin(phi), oz], 1)
    eta = np.float32(1.0) / np.float32(1.5)
    v = F.vertex(N, D, np.full(n, 0.5), np.full(3, 0.04), np.full(n, eta), rng.uniform(0, 1, n), rng.uniform(0, 1, n), np.full(n, 1.0 - 2.0 ** -24))
    ccrit = np.sqrt(1.0 - float(eta) ** 2)
    tir = v["c"] < ccrit - 1e-9
    assert tir.sum() > 200 and (~tir).sum() > 200
    assert (v["tir"][tir]).all() and (v["Fm"][tir] == 1.0).all() and v["refl"][tir].all()
    assert (v["g"][tir] == G.ggx_G1(np.full(int(tir.sum()), np.float64(np.float32(0.5))), v["w"][tir])[:, None]).all()      # F / Fm = 1
    above = v["c"] > ccrit + 1e-9
    assert (v["Fm"][above] < 1.0).all() and not v["refl"][above].any()      # u_sel just below 1: they refract
    assert (v["w"][above & ~v["refl"]][:, 2] < 0).mean() > 0.5      # (at alpha = 0.5 a share of the refractions leaves the lower hemisphere)
