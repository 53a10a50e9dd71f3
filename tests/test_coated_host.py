"""The coated diffuse of option coated on host-only contexts (the option and its refusals, pt_debug_coated's argument checks,
scenes.cornell_box(coated=True); include/pt_api.h) and the float64 model of the vertex (tests/coated_ref.py) by quadrature: no device
needed."""

import os

import numpy as np
import pytest

import coated_ref as K
import glossy_ref as G

# (the library is imported inside the tests, through conftest's `api` fixture: importing it while the modules are collected would load it
# before tests/test_distributed_gloo.py imports torch, and the library must bind to the HIP runtime torch loaded -- see bench.py)

NEW_SYMBOLS = ["pt_debug_coated"]


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
    spec = spec or scenes.cornell_box(8, 4, coated=True)
    for m in spec.materials:
        sc.add_Material(*m)
    for verts, mati in spec.objects:
        sc.add_Triangles(api.triangles_from_vertices(verts, mati))
        sc.end_Obj()
    sc.upload_Triangles()
    sc.upload_Materials()
    return sc


def test_option_parses_0_and_1_and_refuses_2(api):
    sc = host_scene(api)
    sc.set_option("coated", 1)
    sc.set_option("coated", 0)
    for bad in (2, -1):
        with pytest.raises(api.PtError) as e:
            sc.set_option("coated", bad)
        assert e.value.code == api.PT_EINVAL and "coated" in str(e.value)
    # option glossy keeps its contract and its text
    with pytest.raises(api.PtError) as e:
        sc.set_option("glossy", 2)
    assert "glossy must be 0 (material type 4 is inert) or 1 (pt_render_nee shades it as a rough metal)" in str(e.value)


def test_roughness_of_a_type_5_material_and_the_host_records(api):
    """alpha = pt_material_roughness(shininess) goes into field n of the DEVICE copy only (a host-only context has none: what the device
    reads is checked by the float64 replay of tests/test_gpu_coated.py, whose model takes alpha from the shininess); the host records
    stay what was added."""
    from opencl_path_tracer_amd import scenes
    spec = scenes.cornell_box(8, 4, coated=True)
    p = len(spec.materials) - 1
    sc = host_scene(api, spec)
    _, mats, _ = sc.debug_scene()
    want = api.Material(*spec.materials[p])
    assert int(mats["type"][p]) == 5 and mats[p].tobytes() == want[0].tobytes()
    assert np.float32(api.material_roughness(spec.materials[p][5])) == np.float32(G.roughness(300.0))
    assert np.allclose(want["F0"][0, :3], 0.04, rtol=1e-6)


def test_refusals_come_before_the_device_check(api):
    sc = host_scene(api)
    sc.iterations = 4
    calls = (lambda: sc.render(1), lambda: sc.trace_rays(), lambda: sc.generate_rays(), lambda: sc.render_adaptive(2, 4, 0.1),
             lambda: sc.render_adaptive(2, 4, 0.1, path="render"))
    sc.set_option("coated", 1)
    for call in calls:
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_EINVAL and "coated" in str(e.value)
    # the NEE paths do not refuse: a host-only context has no device for them
    for call in (lambda: sc.render_nee(1, "mis"), lambda: sc.render_adaptive(2, 4, 0.1, path="nee", metric="half")):
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_ENODEVICE
    sc.set_option("coated", 0)
    for call in calls:
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_ENODEVICE


def test_debug_coated_argument_checks(api):
    sc = host_scene(api)
    with pytest.raises(api.PtError) as e:
        sc.debug_coated(np.zeros((1, 12), dtype=np.float32))
    assert e.value.code == api.PT_ENODEVICE                    # host-only context: the device check comes first
    assert api.LIB.pt_debug_coated(None, 1, None, None) == api.PT_EINVAL
    with pytest.raises(ValueError):
        sc.debug_coated(np.zeros((1, 9), dtype=np.float32))    # 12 floats per item


def test_cornell_box_coated_has_exactly_one_type_5_material(api):
    from opencl_path_tracer_amd import scenes
    plain, spec = scenes.cornell_box(8, 4), scenes.cornell_box(8, 4, coated=True)
    types = [m[6] for m in spec.materials]
    assert types.count(5) == 1 and [m[6] for m in plain.materials].count(5) == 0
    p = types.index(5)
    assert spec.materials[:len(plain.materials)] == plain.materials and p == len(plain.materials)
    kd, ks, em, N, Kx, ns, _ = spec.materials[p]
    assert kd[0] > 3 * kd[1] and kd[0] > 3 * kd[2] and tuple(ks) == (0, 0, 0) and tuple(em) == (0, 0, 0)      # red
    assert tuple(N) == (1.5, 1.5, 1.5) and tuple(Kx) == (0, 0, 0) and 100.0 <= ns <= 1000.0
    # the second sphere, and only it, wears it; with glossy=True as well the first sphere is the rough metal
    assert (spec.objects[2][1] == p).all() and not (spec.objects[0][1] == p).any() and not (spec.objects[1][1] == p).any()
    both = scenes.cornell_box(8, 4, glossy=True, coated=True)
    assert sorted(m[6] for m in both.materials[len(plain.materials):]) == [4, 5]
    for (v, _), (pv, _) in zip(spec.objects, plain.objects):
        assert np.array_equal(v, pv)


# ---------------------------------------------------------------------------- the model alone, by quadrature
def hemisphere(n_mu, n_phi, lo=0.0, hi=1.0):
    """Gauss-Legendre in cos(theta) over [lo, hi] x the midpoint rule in phi (as test_gpu_glossy.quadrature): directions (n, 3), weights"""
    x, wt = np.polynomial.legendre.leggauss(n_mu)
    mu, wt = lo + (hi - lo) * 0.5 * (x + 1.0), (hi - lo) * 0.5 * wt
    phi = (np.arange(n_phi) + 0.5) * 2.0 * np.pi / n_phi
    s = np.sqrt(1.0 - mu * mu)
    w = np.stack([np.outer(s, np.cos(phi)), np.outer(s, np.sin(phi)), np.outer(mu, np.ones(n_phi))], -1).reshape(-1, 3)
    return w, np.outer(wt, np.full(n_phi, 2.0 * np.pi / n_phi)).reshape(-1)


def lobe_integrals(alpha, oz, F0=0.04, kd=1.0):
    """(integral of p_b over the upper hemisphere, ps, the coat lobe's mass above the surface, I(o) = integral of spec + diff) of
    coated_ref.evaluate for o = (sqrt(1 - oz^2), 0, oz).  The terms that carry D(h) are integrated over the HALF vector, w = 2 (o.h) h - o
    with dw = 4 (o.h) dh, cos(theta_h) split at the lobe's width so that the peak of alpha = 0.03 is resolved; the cosine lobe and diff over
    w itself.  The same grid integrates the visible-normal density to 1 (asserted), which is what says the quadrature resolves the lobe."""
    a = np.array([alpha])
    o = np.array([[np.sqrt(1.0 - oz * oz), 0.0, oz]])
    ps = float(K.lobe_probability(np.full((1, 3), F0), np.full((1, 3), kd), o[:, 2])[0])
    cut = 1.0 / np.sqrt(1.0 + (8.0 * alpha) ** 2)              # tan(theta_h) = 8 alpha
    up_mass = spec_int = total = 0.0
    for lo, hi in ((0.0, cut), (cut, 1.0)):
        h, wq = hemisphere(192, 384, lo, hi)
        oo = np.broadcast_to(o, h.shape)
        oh = G.dot(oo, h)
        w = h * (2.0 * oh)[:, None] - oo
        front = oh > 0
        h, w, oo, wq = h[front], w[front], oo[front], wq[front] * 4.0 * oh[front]
        F0v, kdv = np.full(h.shape, F0), np.full(h.shape, kd)
        pb, g, spec, diff = K.evaluate(a, F0v, kdv, np.full(len(h), ps), oo, h, w)
        coat = (pb - (1.0 - ps) * np.maximum(w[:, 2], 0.0) / np.pi) / ps      # the coat lobe's own density of w
        up = w[:, 2] > 0
        total += float((coat * wq).sum())
        up_mass += float((coat * wq)[up].sum())
        spec_int += float((spec[:, 0] * wq)[up].sum())
    assert abs(total - 1.0) < 2e-3, (alpha, oz, total)
    w, wq = hemisphere(96, 192)
    oo = np.broadcast_to(o, w.shape)
    F0v, kdv = np.full(w.shape, F0), np.full(w.shape, kd)
    pb, g, spec, diff = K.evaluate_of(a, F0v, kdv, oo, w)
    pg, _ = G.ggx_pdf_of(a, oo, w)
    base_int = float(((pb - ps * pg) * wq).sum())               # (1 - ps) x the cosine lobe
    pb_int = ps * up_mass + base_int
    return pb_int, ps, up_mass, spec_int + float((diff[:, 0] * wq).sum())


@pytest.mark.parametrize("alpha", [0.03, 0.1, 0.5, 1.0])
def test_mixture_density_and_energy_by_quadrature(alpha):
    """White kd, F0 = 0.04: the mixture integrates over the upper hemisphere to 1 - ps x (the share of the coat lobe's visible-normal
    reflections that fall below the surface) and never exceeds 1; I(o), the integral of spec + diff, is at most 1."""
    for oz in (0.05, 0.1, 0.2, 0.35, 0.5, 0.7, 0.85, 1.0):
        pb_int, ps, up_mass, energy = lobe_integrals(alpha, oz)
        assert 0.1 <= ps <= 0.9
        assert up_mass <= 1.0 + 2e-3
        assert abs(pb_int - (1.0 - ps * (1.0 - up_mass))) < 1e-9 + 2e-3 and pb_int <= 1.0 + 2e-3, (alpha, oz, pb_int)
        assert energy <= 1.0, (alpha, oz, energy)
    # the pointwise functions against the closed forms they are made of, at generic directions
    rng = np.random.default_rng(5)
    w = G.unit(np.abs(rng.normal(size=(64, 3))) + 1e-3)
    o = G.unit(np.abs(rng.normal(size=(64, 3))) + 1e-3)
    a = np.array([alpha])
    F0v, kdv = np.full((64, 3), 0.04), np.full((64, 3), 1.0)
    pb, g, spec, diff = K.evaluate_of(a, F0v, kdv, o, w)
    ps = K.lobe_probability(F0v, kdv, o[:, 2])
    pg, h = G.ggx_pdf_of(a, o, w)
    assert np.allclose(pb, ps * pg + (1.0 - ps) * w[:, 2] / np.pi, rtol=1e-12)
    assert np.allclose(spec[:, 0], K.schlick_c(F0v, G.dot(h, o))[:, 0] * G.ggx_D(a, h) * G.ggx_G1(a, o) * G.ggx_G1(a, w) / (4.0 * o[:, 2]), rtol=1e-12)
    assert np.allclose(g * pb[:, None], spec + diff, rtol=1e-12)
    # reciprocity: spec / w.z is symmetric in (o, w), and so is the attenuation of the base, diff / (kd w.z^2 / pi)
    pb2, g2, spec2, diff2 = K.evaluate_of(a, F0v, kdv, w, o)
    assert np.allclose(spec[:, 0] / w[:, 2], spec2[:, 0] / o[:, 2], rtol=1e-10)
    assert np.allclose(diff[:, 0] / w[:, 2] ** 2, diff2[:, 0] / o[:, 2] ** 2, rtol=1e-10)
