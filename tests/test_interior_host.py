"""Interiors of dielectrics (Scene.set_material_interior) on host-only contexts: the record, its checks, the life of a binding, the refusals
of the other render paths, SceneSpec.interiors, api.interior_from_tint (include/pt_api.h), and tests/interior_ref.py's InteriorModel against
a brute-force integration of Beer-Lambert, against MediumModel under a null binding and against the bounded fog it must agree with in
the mean (the premise of tests/test_gpu_interior.py's cross-check).  No device needed."""

import ctypes as C
import os

import numpy as np
import pytest

import interior_ref as IR
import medium_ref as M

NEW_SYMBOLS = ["pt_interior_defaults", "pt_set_material_interior", "pt_clear_material_interiors", "pt_get_material_interior", "pt_debug_interior"]


def host_scene(api, spec=None):
    from opencl_path_tracer_amd import scenes
    sc = api.Scene(16, 16, device=None)
    spec = spec or scenes.cornell_box(8, 4)
    for m in spec.materials:
        sc.add_Material(*m)
    for verts, mati in spec.objects:
        sc.add_Triangles(api.triangles_from_vertices(verts, mati))
        sc.end_Obj()
    sc.upload_Triangles()
    sc.upload_Materials()
    return sc


def f32(v):
    return tuple(float(np.float32(x)) for x in v)


def test_abi_has_the_new_symbols_and_the_record(api):
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTS and hasattr(api.LIB, name)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "pt_api.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header
    assert "typedef struct pt_interior {" in header
    with open(os.path.join(root, "include", "pt_scene.hpp")) as f:
        hpp = f.read()
    for name in ("set_material_interior", "clear_material_interiors", "material_interior", "debug_interior"):
        assert name + "(" in hpp
    assert C.sizeof(api.Interior) == 20
    assert [n for n, _ in api.Interior._fields_] == ["sigma_a", "sigma_s", "g"]
    p = api.Interior((C.c_float * 3)(1, 2, 3), 4.0, 0.5)
    api.LIB.pt_interior_defaults(C.byref(p))
    want = {"sigma_a": (0.0, 0.0, 0.0), "sigma_s": 0.0, "g": 0.0}
    assert p.as_dict() == want and api.interior_defaults() == want
    api.LIB.pt_interior_defaults(None)


def test_set_material_interior_checks_its_arguments(api):
    from opencl_path_tracer_amd import scenes
    sc = host_scene(api)
    G = scenes.GLASS
    assert sc.material_interior(G) is None
    good = dict(sigma_a=(0.1, 0.02, 0.3), sigma_s=0.25, g=0.6)
    sc.set_material_interior(G, **good)
    held = sc.material_interior(G)
    assert held == {"sigma_a": f32(good["sigma_a"]), "sigma_s": 0.25, "g": float(np.float32(0.6))}
    nan, inf = float("nan"), float("inf")
    bad = [(dict(sigma_a=(nan, 0, 0)), "sigma_a"), (dict(sigma_a=(0, -1e-3, 0)), "sigma_a"), (dict(sigma_a=(0, 0, inf)), "sigma_a"),
           (dict(sigma_s=nan), "sigma_s"), (dict(sigma_s=-0.5), "sigma_s"), (dict(sigma_s=inf), "sigma_s"),
           (dict(g=nan), "g"), (dict(g=0.995), "g"), (dict(g=-1.0), "g")]
    for change, field in bad:
        with pytest.raises(api.PtError) as e:
            sc.set_material_interior(G, **dict(good, **change))
        assert e.value.code == api.PT_EINVAL and "pt_set_material_interior" in str(e.value) and field in str(e.value), change
        assert sc.material_interior(G) == held, change              # a refused call leaves the held binding as it was
    for m in (-1, len(scenes.BUILTIN_MATERIALS)):                   # the material index, checked as pt_set_material_texture checks it
        with pytest.raises(api.PtError) as e:
            sc.set_material_interior(m, **good)
        assert e.value.code == api.PT_EINVAL and "pt_set_material_interior" in str(e.value) and "material" in str(e.value)
        with pytest.raises(api.PtError):
            sc.material_interior(m)
    p = api.Interior()
    assert api.LIB.pt_set_material_interior(None, G, C.byref(p)) == api.PT_EINVAL
    assert api.LIB.pt_set_material_interior(sc._h, G, None) == api.PT_EINVAL and "interior is NULL" in api.LIB.pt_last_error(sc._h).decode()
    assert api.LIB.pt_clear_material_interiors(None) == api.PT_EINVAL
    assert api.LIB.pt_get_material_interior(None, G, C.byref(p)) == api.PT_EINVAL and api.LIB.pt_get_material_interior(sc._h, G, None) == api.PT_EINVAL
    assert api.LIB.pt_debug_interior(None, None, 0, None) == api.PT_EINVAL
    assert sc.material_interior(G) == held
    # the edges of the ranges; a number for sigma_a; the defaults themselves
    sc.set_material_interior(G)
    assert sc.material_interior(G) == api.interior_defaults()
    sc.set_material_interior(G, sigma_a=0.5, sigma_s=0.0, g=-0.99)
    assert sc.material_interior(G) == {"sigma_a": (0.5, 0.5, 0.5), "sigma_s": 0.0, "g": float(np.float32(-0.99))}
    sc.set_material_interior(G, g=0.99)
    # any material added so far is accepted, as a texture is on a non-diffuse one (the device table ignores it unless the type is 2 or 6)
    sc.set_material_interior(scenes.WHITE_DIFFUSE, sigma_s=1.0)
    assert sc.material_interior(scenes.WHITE_DIFFUSE)["sigma_s"] == 1.0 and sc.material_interior(scenes.CHROMIUM) is None
    late = sc.add_Material(*scenes.BUILTIN_MATERIALS[G])            # added, not yet uploaded: "added so far" is enough
    sc.set_material_interior(late, sigma_a=(1, 2, 3))
    sc.upload_Triangles()                                            # uploads keep the bindings: they are not part of the scene
    sc.upload_Materials()
    assert sc.material_interior(late)["sigma_a"] == (1.0, 2.0, 3.0) and sc.material_interior(G)["g"] == float(np.float32(0.99))
    with pytest.raises(api.PtError) as e:                           # the debug kernel needs a device
        sc.debug_interior(np.zeros((1, 12), dtype=np.float32))
    assert e.value.code == api.PT_ENODEVICE
    sc.clear_material_interiors()
    assert all(sc.material_interior(m) is None for m in (G, scenes.WHITE_DIFFUSE, late))
    sc.clear_material_interiors()                                    # (clearing nothing is fine)


def test_refusals_come_before_the_device_check(api):
    from opencl_path_tracer_amd import scenes
    sc = host_scene(api)
    sc.iterations = 4
    calls = (lambda: sc.render(1), lambda: sc.trace_rays(), lambda: sc.generate_rays(), lambda: sc.render_adaptive(2, 4, 0.1),
             lambda: sc.render_adaptive(2, 4, 0.1, path="render"))
    nee_calls = (lambda: sc.render_nee(1, "mis"), lambda: sc.render_nee(1, "light"), lambda: sc.render_nee(1, "bsdf"),
                 lambda: sc.render_adaptive(2, 4, 0.1, path="nee", metric="half", strategy="mis"),
                 lambda: sc.render_adaptive(2, 4, 0.1, path="nee", metric="half", strategy="bsdf"))

    def codes(cs):
        out = []
        for call in cs:
            with pytest.raises(api.PtError) as e:
                call()
            out.append((e.value.code, str(e.value)))
        return out
    before = codes(calls)
    assert all(c == api.PT_ENODEVICE for c, _ in before)
    sc.set_material_interior(scenes.GLASS)                           # an all-zero binding is live
    for (code, text), name in zip(codes(calls), ("pt_render", "pt_trace_rays", "pt_generate_rays", "pt_render_adaptive", "pt_render_adaptive")):
        assert code == api.PT_EINVAL and "pt_clear_material_interiors" in text and name in text
    assert all(c == api.PT_ENODEVICE for c, _ in codes(nee_calls))       # every NEE strategy renders interiors; the guides keep the clear view
    assert all(c == api.PT_ENODEVICE for c, _ in codes((lambda: sc.render_aovs(1, 4),)))
    sc.clear_material_interiors()
    assert codes(calls) == before
    sc.set_material_interior(scenes.GLASS, sigma_a=(1, 0, 0))
    sc.set_medium(0.01)                                              # both kinds at once: the medium's refusal comes first, as before
    assert codes(calls)[0][0] == api.PT_EINVAL and "pt_clear_medium" in codes(calls)[0][1]
    sc.clear_medium()
    assert "pt_clear_material_interiors" in codes(calls)[0][1]


def test_interior_from_tint_and_the_scene_spec(api):
    from opencl_path_tracer_amd import scenes
    sa = api.interior_from_tint((0.5, 1.0, 0.25), 4.0)
    assert np.allclose(sa, (np.log(2.0) / 4.0, 0.0, np.log(4.0) / 4.0), rtol=1e-15, atol=0.0) and sa[1] == 0.0 and not np.signbit(sa[1])
    assert np.allclose(np.exp(-np.asarray(sa) * 4.0), (0.5, 1.0, 0.25), rtol=1e-15)
    for color, distance in (((0.0, 1, 1), 1.0), ((1.5, 1, 1), 1.0), ((0.5, 0.5, 0.5), 0.0), ((0.5, 0.5, float("nan")), 1.0)):
        with pytest.raises(ValueError):
            api.interior_from_tint(color, distance)
    # SceneSpec.interiors through Scene.load, on a context that already holds materials: the index is the spec's own
    spec = scenes.cornell_box(8, 4, tint=(0.9, 0.5, 0.2), wax=3.0)
    assert list(spec.interiors) == [scenes.GLASS]
    want = dict(sigma_a=f32(api.interior_from_tint((0.9, 0.5, 0.2), 400.0)), sigma_s=float(np.float32(3.0 / 400.0)), g=float(np.float32(0.8)))
    sc = api.Scene(16, 16, device=None)
    extra = sc.add_Material(*scenes.BUILTIN_MATERIALS[0])
    sc.load(spec)
    assert sc.material_interior(extra + 1 + scenes.GLASS) == want and sc.material_interior(scenes.GLASS) is None
    frosted = scenes.cornell_box(8, 4, frosted=True, tint=(0.5, 0.5, 0.5))
    (m, kw), = frosted.interiors.items()
    assert frosted.materials[m][6] == 6 and kw["sigma_s"] == 0.0 and kw["g"] == 0.0
    assert not scenes.cornell_box(8, 4).interiors
    with pytest.raises(ValueError):
        scenes.cornell_box(8, 4, coated=True, wax=1.0)
    with pytest.raises(ValueError):
        scenes.cornell_box(8, 4, tint=(0.0, 0.5, 0.5))


# ---------------------------------------------------------------------------- the model
def test_segment_rule_against_a_brute_force_slab_integration():
    """Beer-Lambert through a slab of thickness t, brute force in float64: the radiance that arrives unscattered is the product over
    200,000 thin layers of (1 - sigma dx) per channel, for absorption; with scattering, the share of free-flight numbers on a regular
    grid of u that reach t is the scattering transmittance, and the mean absorption factor over all of them is the closed form of
    integrating exp(-sigma_a l) over the free-flight density plus the survivors' share."""
    it = IR.interior_of(dict(sigma_a=(0.7, 0.05, 0.0), sigma_s=0.0, g=0.0))
    t, n = 2.6, 200000
    sc, ell, f = IR.segment(it, t, 0.3)
    assert not sc and ell == t
    layers = (1.0 - it["sigma_a"] * (t / n)) ** n
    assert np.allclose(f, layers, rtol=2e-5, atol=0.0) and f[2] == 1.0
    it = IR.interior_of(dict(sigma_a=(0.7, 0.05, 0.0), sigma_s=0.9, g=0.3))
    u = (np.arange(n) + 0.5) / n
    out = [IR.segment(it, t, x) for x in u[::40]]
    share = np.mean([not s for s, _, _ in out])
    assert abs(share - np.exp(-0.9 * t)) < 2.0 / len(out)
    # mean factor: int_0^t sigma_s exp(-sigma_s l) exp(-sigma_a l) dl + exp(-sigma_s t) exp(-sigma_a t)
    st = it["sigma_a"] + it["sigma_s"]
    closed = it["sigma_s"] / st * (1.0 - np.exp(-st * t)) + np.exp(-st * t)
    mean = np.mean([f for _, _, f in out], axis=0)
    assert np.allclose(mean, closed, rtol=1e-3, atol=0.0)
    assert all(ell == (M.flight(0.9, x) if s else t) for (s, ell, _), x in zip(out, u[::40]))


def box_spec(n, lo=(-1.0, -1.0, 4.0), hi=(1.0, 1.0, 6.0), emission=(3.0, 2.0, 1.0)):
    """a type-2 box of index n (F0 its Fresnel value) in front of the eye, and a large emitter quad behind and above it"""
    from opencl_path_tracer_amd import scenes
    F0 = ((n - 1.0) / (n + 1.0)) ** 2
    mats = [((0, 0, 0), (0, 0, 0), (0, 0, 0), (n, n, n), (0, 0, 0), 0.0, 2),
            ((0, 0, 0), (0, 0, 0), emission, (0, 0, 0), (0, 0, 0), 0.0, 3)]
    x0, y0, z0 = lo
    x1, y1, z1 = hi
    c = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    faces = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (3, 7, 6, 2), (0, 4, 7, 3), (1, 2, 6, 5)]
    tris, mo = [], []
    for a, b, cc, d in faces:
        tris += [(c[a], c[b], c[cc]), (c[a], c[cc], c[d])]
        mo += [0, 0]
    tris += [((-30, -30, 20.0), (30, -30, 20.0), (30, 30, 20.0)), ((-30, -30, 20.0), (30, 30, 20.0), (-30, 30, 20.0))]
    mo += [1, 1]
    spec = scenes.SceneSpec(materials=mats, name="interior_box", shift=(-500.0, -500.0, 1299.0378))
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.asarray(mo, dtype=np.uint16)))
    assert abs(api_material_F0(mats[0]) - F0) < 1e-6
    return spec


def api_material_F0(m):
    from opencl_path_tracer_amd import api
    return float(api.Material(*m)["F0"][0][0])


def model_of(api, sc, spec, medium=None, interiors=None, cls=IR.InteriorModel):
    verts = np.concatenate([v for v, _ in spec.objects])
    mo = np.concatenate([m for _, m in spec.objects])
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    args = (verts, recs["N"], mats, mo, sc.camera[0], None, medium)
    if cls is IR.InteriorModel:
        return cls(*args, interiors)
    return cls(*args)


def test_a_null_binding_is_the_medium_model_sample_for_sample(api):
    spec = box_spec(1.5)
    sc = api.Scene(12, 8, device=None).load(spec)
    fog = dict(sigma_t=0.05, albedo=(0.9, 0.7, 0.5), g=0.4, lo=(-3.0, -3.0, 0.5), hi=(3.0, 3.0, 9.0))
    seeds = np.random.default_rng(5).integers(1, 2 ** 31 - 2, 12 * 8).astype(np.int32)
    null = dict(sigma_a=(0.0, 0.0, 0.0), sigma_s=0.0, g=0.0)
    for medium in (None, fog):
        a = model_of(api, sc, spec, medium, {0: null})
        b = model_of(api, sc, spec, medium, cls=M.MediumModel)
        c = model_of(api, sc, spec, medium, {})
        inside = 0
        for gid in range(12 * 8):
            for strategy in (0, 2):
                ra, rb, rc = (m.sample(gid, int(seeds[gid]), 6, strategy) for m in (a, b, c))
                assert np.array_equal(ra[0], rb[0]) and ra[1:] == rb[1:] and np.array_equal(rc[0], rb[0]) and rc[1:] == rb[1:]
                assert {k: v for k, v in a.last.items() if not k.startswith("interior")} == b.last
                assert all(a.last[k] == 0 for k in IR.InteriorModel.EVENTS if k.startswith("interior"))
                inside += int(ra[0].any())
        assert inside > 0


CROSS = dict(n=1.0005, sigma_a=0.15, sigma_s=0.6, g=0.5, W=16, H=12, bounces=12)


def test_premise_of_the_cross_check_against_the_fog(api):
    """A type-2 box with n = 1.0005 (F0 = 6.2e-8: reflections carry nothing, refraction bends a ray at 60 degrees of incidence by under
    0.05 degrees) with a grey interior against the same box without a boundary as bounded fog of sigma_t = sigma_a + sigma_s and
    albedo = sigma_s / sigma_t, under the emitter quad of box_spec, strategy bsdf, model against model on independent seeds.  The two are
    the same estimator in expectation (absorption as a factor per segment against an albedo per scatter vertex); the frame means must
    agree within five standard errors, the bending bias far below that."""
    n = CROSS["n"]
    glass, air = box_spec(n), box_spec(n)
    air.objects = [(air.objects[0][0][12:], air.objects[0][1][12:])]           # the emitter alone
    W, H = CROSS["W"], CROSS["H"]
    sg = api.Scene(W, H, device=None).load(glass)
    sa = api.Scene(W, H, device=None).load(air)
    sig_t = CROSS["sigma_a"] + CROSS["sigma_s"]
    interior = dict(sigma_a=(CROSS["sigma_a"],) * 3, sigma_s=CROSS["sigma_s"], g=CROSS["g"])
    fog = dict(sigma_t=sig_t, albedo=(CROSS["sigma_s"] / sig_t,) * 3, g=CROSS["g"], lo=(-1.0, -1.0, 4.0), hi=(1.0, 1.0, 6.0))
    mi = model_of(api, sg, glass, None, {0: interior})
    mf = model_of(api, sa, air, fog, {})
    rng = np.random.default_rng(11)
    lum = {}
    for name, model in (("interior", mi), ("fog", mf)):
        vals = []
        for rep in range(6):
            seeds = rng.integers(1, 2 ** 31 - 2, W * H)
            vals += [model.sample(g, int(seeds[g]), CROSS["bounces"], 0)[0].mean() for g in range(W * H)]
        lum[name] = np.asarray(vals)
    a, b = lum["interior"], lum["fog"]
    se = np.sqrt(a.var(ddof=1) / a.size + b.var(ddof=1) / b.size)
    print("interior %.5f  fog %.5f  difference %.5f  standard error %.5f" % (a.mean(), b.mean(), a.mean() - b.mean(), se))
    assert a.mean() > 0.1 and abs(a.mean() - b.mean()) < 5.0 * se


def test_a_null_binding_is_the_frosted_model_sample_for_sample(api):
    """InteriorFrostedModel restates FrostedModel.sample: without a binding, and with an all-zero one on the type-6 material, it is
    FrostedModel's sample for sample -- colours, LCG state, near-tie flag and events -- on test_gpu_frosted.py's replay scene (a type-6
    sphere and pane, types 0 to 5 around them), every pixel of a 16 x 12 frame, strategies bsdf and mis, 8 bounces."""
    import frosted_ref as F
    import test_gpu_frosted as TF
    spec = TF.replay_spec()
    W, H = 16, 12
    sc = api.Scene(W, H, device=None).load(spec)
    verts = np.concatenate([v for v, _ in spec.objects])
    mo = np.concatenate([m for _, m in spec.objects])
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    vn = np.concatenate([np.zeros(v.shape, dtype=np.float32) if n is None else n for (v, _), n in zip(spec.objects, spec.normals)])
    args = (verts, recs["N"], mats, mo, sc.camera[0], vn)
    table = sc.debug_light_table()
    null = dict(sigma_a=(0.0, 0.0, 0.0), sigma_s=0.0, g=0.0)
    base = F.FrostedModel(*args, table=table)
    models = [IR.InteriorFrostedModel(*args, table=table, interiors=b) for b in ({}, {TF.FROSTED: null})]
    seeds = np.random.default_rng(7).integers(1, 2 ** 31 - 2, W * H)
    inside = 0
    for gid in range(W * H):
        for strategy in (0, 2):
            want = base.sample(gid, int(seeds[gid]), 8, strategy)
            events = dict(base.last)
            inside += events["frosted_inside"]
            for m in models:
                got = m.sample(gid, int(seeds[gid]), 8, strategy)
                assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
                assert {k: v for k, v in m.last.items() if not k.startswith("interior")} == events
                assert all(m.last[k] == 0 for k in IR.INTERIOR_EVENTS)
    assert inside > 0
