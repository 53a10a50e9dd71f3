"""No GPU: the area lights of render_nee on a host-only context (pt_set_area_lights, pt_arealights.cpp; include/pt_api.h pins the set, the
table and the estimator): struct sizes and defines, every argument check in its order, the table against a numpy restatement, the helper
conversions, the refusals, SceneSpec.area_lights, and the cone density of the restated sampler (tests/arealights_ref.py) by quadrature."""

import ctypes as C

import numpy as np
import pytest

import arealights_ref as A


@pytest.fixture()
def sc(api):
    return api.Scene(8, 8, device=None)


def sphere(api, **kw):
    d = dict(center=(0.0, 5.0, 0.0), radius=1.0, radiance=(3.0, 2.0, 1.0))
    if "power" in kw:
        del d["radiance"]
    d.update(kw)
    return api.sphere_light(**d)


def test_struct_sizes_and_defines(api):
    assert C.sizeof(api.AreaLight) == 48 and C.sizeof(api.AreaLightsParams) == 4
    assert api.AREA_LIGHT_SAMPLE.itemsize == 24 and api.AREA_LIGHT_HIT.itemsize == 16
    assert (api.AREA_LIGHT_SPHERE, api.AREA_LIGHT_SUN, api.AREA_LIGHTS_MAX) == (0, 1, 64)
    assert api.area_lights_defaults() == {"select": 0.5}
    assert api.AREA_KEY not in (0, 0xffffffff, 0x5bd1e995)      # S, ~S and S ^ 0x5bd1e995 are taken
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(api.__file__))), "include", "pt_api.h")).read()
    assert "#define PT_AREA_KEY 0x%xu" % api.AREA_KEY in header
    for name, value in (("PT_AREA_LIGHT_SPHERE", 0), ("PT_AREA_LIGHT_SUN", 1), ("PT_AREA_LIGHTS_MAX", 64)):
        assert any(line.split()[:3] == ["#define", name, str(value)] for line in header.splitlines()), name


def test_argument_checks_and_their_order(api, sc):
    good = sphere(api)
    sc.set_area_lights([good])
    before = sc.debug_area_lights()

    def refused(lights, select=0.5, count=None, null=False):
        arr = (api.AreaLight * max(len(lights), 1))(*lights)
        p = api.AreaLightsParams(select)
        rc = api.LIB.pt_set_area_lights(sc._h, None if null else arr, len(lights) if count is None else count, C.byref(p))
        assert rc == api.PT_EINVAL
        after = sc.debug_area_lights()           # a failed call leaves the set unchanged
        assert np.array_equal(after["records"], before["records"]) and after["P_area"] == before["P_area"]
        return api.LIB.pt_last_error(sc._h).decode()

    bad_type = sphere(api)
    bad_type.type = 2
    nan = sphere(api, center=(np.nan, 0, 0))
    assert "count" in refused([good], count=-1)
    assert "count" in refused([good], count=65, null=True)              # the count before the pointer
    assert "NULL" in refused([good], null=True, select=7.0)             # the pointer before select
    assert "select" in refused([bad_type], select=1.5)                  # select before the lights
    assert "select" in refused([good], select=float("nan"))
    bad_both = sphere(api, center=(np.nan, 0, 0))
    bad_both.type = 5
    assert "type" in refused([bad_both])                                # the type before the fields
    assert "finite" in refused([nan])
    neg_and_small = sphere(api, radiance=(-1.0, 0, 0), radius=0.0)
    assert "radiance" in refused([neg_and_small])                       # radiance before weight and size
    assert "weight" in refused([sphere(api, weight=-1.0, radius=-1.0)])
    assert "size" in refused([sphere(api, radius=0.0)])
    sun = api.sun_light((0, -1, 0), 1.0, irradiance=1.0)
    sun.size = 1.6
    assert "size" in refused([sun])
    sun.size = 0.0
    assert "size" in refused([sun])
    zero = api.sun_light((0, 0, 0), 1.0, irradiance=1.0)
    assert "direction" in refused([zero])
    assert "light 1" in refused([good, zero])                           # the first bad light is named
    with pytest.raises(api.PtError):
        sc.set_area_lights([good] * 65)
    half = api.sun_light((0, -1, 0), 180.0, radiance=1.0)               # a = pi / 2 is allowed
    sc.set_area_lights([good] * 63 + [half])
    assert len(sc.debug_area_lights()["cdf"]) == 64
    sc.set_area_lights([])
    assert len(sc.debug_area_lights()["cdf"]) == 0


def test_table_against_numpy(api, sc):
    lights = [api.sun_light((1.0, -2.0, 0.5), 0.533, irradiance=(3.0, 2.5, 2.0)),
              sphere(api, radius=0.5, radiance=(10.0, 10.0, 10.0)),
              sphere(api, center=(1, 2, 3), radius=2.0, radiance=(0.0, 0.0, 0.0)),          # black: stays, never picked
              api.sun_light((0.0, -1.0, 0.0), 57.0, radiance=(0.1, 0.2, 0.3), weight=4.0),
              sphere(api, center=(-3, 2, 1), radius=0.25, power=(50.0, 40.0, 30.0))]
    sc.set_area_lights(lights, select=0.3)
    got = sc.debug_area_lights()
    want = A.table(lights)
    assert got["n_sphere"] == 3 and list(got["order"]) == [1, 2, 4, 0, 3]
    assert np.array_equal(got["order"], want["order"])
    assert np.array_equal(got["cdf"].view(np.uint32), want["cdf"].view(np.uint32))
    assert np.array_equal(got["P_light"], want["P_light"])
    assert np.array_equal(got["records"].view(np.uint32), want["records"].view(np.uint32))
    assert got["P_light"][1] == 0.0 and got["P_light"].sum() == 1.0
    assert got["P_area"] == 1.0                  # nothing else is pickable on a context without a scene
    auto = want["weights"]
    assert np.isclose(auto[0], 30.0 * 4 * np.pi ** 2 * 0.25) and np.isclose(auto[3], 7.5, rtol=1e-6) and auto[4] == 4.0
    sc.set_area_lights([sphere(api, radiance=(0, 0, 0))])
    assert sc.debug_area_lights()["P_area"] == 0.0
    sc.clear_area_lights()
    assert len(sc.debug_area_lights()["cdf"]) == 0 and sc.debug_area_lights()["P_area"] == 0.0


def test_p_area_counts_the_other_lights(api, cb_spec):
    sc = api.Scene(8, 8, device=None).load(cb_spec)        # the box's lamp is in the light table
    sc.set_area_lights([sphere(api)], select=0.3)
    assert sc.debug_area_lights()["P_area"] == np.ceil(np.float32(0.3).astype(np.float64) * 2 ** 24) / 2 ** 24
    sc.set_area_lights([sphere(api)], select=0.0)
    assert sc.debug_area_lights()["P_area"] == 0.0
    sc.set_area_lights([sphere(api)], select=1.0)
    assert sc.debug_area_lights()["P_area"] == 1.0


def test_helper_conversions(api):
    s = api.sphere_light((1, 2, 3), 2.0, power=(8.0, 4.0, 2.0))
    assert np.allclose(list(s.radiance), np.array([8.0, 4.0, 2.0]) / (4 * np.pi ** 2 * 4.0), rtol=1e-6)
    assert s.type == api.AREA_LIGHT_SPHERE and s.size == 2.0 and list(s.position) == [1, 2, 3]
    sun = api.sun_light((0, -1, 0), 0.533, irradiance=(3.0, 2.0, 1.0))
    a = np.radians(0.533 / 2)
    assert np.isclose(sun.size, a, rtol=1e-6) and sun.type == api.AREA_LIGHT_SUN
    assert np.allclose(list(sun.radiance), np.array([3.0, 2.0, 1.0]) / (2 * np.pi * (1 - np.cos(a))), rtol=1e-5)
    with pytest.raises(ValueError):
        api.sphere_light((0, 0, 0), 1.0)
    with pytest.raises(ValueError):
        api.sun_light((0, -1, 0), 1.0, irradiance=1.0, radiance=1.0)
    d = api.area_light_from(dict(kind="sun", direction=(0, -1, 0), angular_diameter_degrees=1.0, radiance=(1, 1, 1)))
    assert d.type == api.AREA_LIGHT_SUN
    with pytest.raises(KeyError):
        api.area_light_from(dict(kind="disc"))


def test_refusals_on_a_host_only_context(api, cb_spec):
    sc = api.Scene(8, 8, device=None).load(cb_spec)
    sc.set_area_lights([sphere(api)])
    for call in (lambda: sc.render(1), sc.generate_rays, sc.trace_rays,
                 lambda: sc.render_adaptive(2, 4, 0.1), lambda: sc.render_adaptive(2, 4, 0.1, path="render"),
                 lambda: sc.render_adaptive(2, 4, 0.1, path=api.PT_ADAPT_PATH_RENDER, metric="variance")):
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_EINVAL and "pt_clear_area_lights" in str(e.value)      # before the device check
    with pytest.raises(api.PtError) as e:          # render_nee is allowed, in every strategy: what stops it here is the missing device
        sc.render_nee(1, "bsdf")
    assert e.value.code == api.PT_ENODEVICE
    sc.set_area_lights([sphere(api, radiance=(0, 0, 0))])      # an all-black set refuses nothing
    with pytest.raises(api.PtError) as e:
        sc.render(1)
    assert e.value.code == api.PT_ENODEVICE
    sc.set_area_lights([sphere(api)])
    sc.upload_Triangles()                                       # uploads keep the set
    sc.upload_Materials()
    assert len(sc.debug_area_lights()["cdf"]) == 1


def test_scene_spec_area_lights(api):
    from opencl_path_tracer_amd import scenes
    spec = scenes.cornell_box(lamp="sphere")
    assert spec.ntris == scenes.cornell_box().ntris - 2 and not spec.lights
    sc = api.Scene(8, 8, device=None).load(spec)
    t = sc.debug_area_lights()
    assert t["n_sphere"] == 1 and t["P_area"] == 1.0
    R = scenes.LAMP_SPHERE_RADIUS
    quad = scenes.cornell_box().objects[0][0][:2].astype(np.float64)
    area = 0.5 * sum(np.linalg.norm(np.cross(q[1] - q[0], q[2] - q[0])) for q in quad)
    E = np.asarray(scenes.BUILTIN_MATERIALS[scenes.LAMP][2], dtype=np.float64)
    assert np.allclose(t["records"][0, 4:7] * 4 * np.pi ** 2 * R * R, np.pi * E * area, rtol=1e-6)      # the quad's power
    img, sun = scenes.sun_and_sky_light()
    assert np.array_equal(img, scenes.sun_and_sky())            # sun_and_sky keeps its output
    light = api.area_light_from(sun)
    assert np.isclose(light.size, np.radians(5.0)) and list(light.radiance) == [400.0, 360.0, 300.0]
    assert np.allclose(-np.asarray(list(light.direction)), (0.3, 0.8, 0.5))


@pytest.mark.parametrize("q", [2.0 * np.sin(0.00465 / 2) ** 2, 2.0 * np.sin(0.25) ** 2, 1.0])
def test_cone_density_integrates_to_one(q):
    """The restated sampler's own Jacobian: |dw/du1 x dw/du2| by central differences of cone_direction over a midpoint grid of (u1, u2) is
    the solid angle per unit of the square, so its integral is the cone's solid angle, and the density 1 / (2 pi q) must integrate to 1
    over it; it is also uniform: the Jacobian is 2 pi q everywhere.  Every direction is unit and inside the cone."""
    axis = np.array([0.3, -0.8, 0.52])
    axis /= np.linalg.norm(axis)
    n, h = 24, 1e-5
    mid = (np.arange(n) + 0.5) / n
    total, worst = 0.0, 0.0
    for a in mid:
        for b in mid:
            d1 = (A.cone_direction(axis, q, a + h, b, np.float64) - A.cone_direction(axis, q, a - h, b, np.float64)) / (2 * h)
            d2 = (A.cone_direction(axis, q, a, b + h, np.float64) - A.cone_direction(axis, q, a, b - h, np.float64)) / (2 * h)
            jac = np.linalg.norm(np.cross(d1, d2))
            worst = max(worst, abs(jac * A.cone_density(q) - 1.0))
            total += jac / (n * n)
    assert abs(total * A.cone_density(q) - 1.0) < 1e-5 and worst < 1e-4, (total, worst)
    for a, b in ((0.0, 0.0), (1 - 2.0 ** -24, 0.3), (0.5, 1 - 2.0 ** -24)):
        w = A.cone_direction(axis, q, a, b, np.float64)
        assert abs(np.linalg.norm(w) - 1.0) < 1e-12 and w @ axis >= 1.0 - q - 1e-15


def test_no_authored_item_is_near_its_other_outcome():
    """The authored items of the GPU test's debug_area_light_eval comparison, in the float64 restatement: every sphere decision (outside or
    inside, the discriminant's sign, t against t_max and the best so far) is at least 1e-4 relative from its other outcome, every sun-disc
    membership at least 1e-4 of the disc's own scale 1 - cos a from its rim, and float32 decides each item as float64 does."""
    import test_gpu_arealights as T
    from opencl_path_tracer_amd import api
    lights, samples, rays = T.eval_items(api)
    table = A.table(lights)
    s64, h64 = T.eval_reference(table, samples, rays, np.float64)
    s32, h32 = T.eval_reference(table, samples, rays, np.float32)
    scale = {0: 1.0 - np.cos(T.SUN_SMALL), 1: 1.0 - np.cos(T.SUN_WIDE)}
    for (j, t, mask, m1, m2), b in zip(h64, h32):
        assert all(min(m) > 1e-4 for m in m1)
        assert all(m > 1e-4 * scale[k] for k, m in enumerate(m2))
        assert (j, mask) == (b[0], b[2])
    assert [(a is None) for a in s64] == [(b is None) for b in s32]


@pytest.mark.parametrize("scene", ["box", "box_sky", "fog", "glossy"])
def test_near_tie_share_of_the_model_alone(api, scene):
    """The float64 model on each of the GPU test's replay scenes and its seeds, on a host-only context, strategy mis: the share of pixels
    with a near-tie -- the models' own decisions plus sphere-hit margins and sun-disc membership -- stays under the project's 10 % cap
    (test_gpu_env.py), and the seeds reach the new decisions."""
    import test_gpu_arealights as T
    if scene == "glossy":
        sc, spec = T.glossy_replay_scene(api, device=None)
        model = T.glossy_replay_model(api, sc, spec)
    else:
        sky = scene != "box"
        sc, spec, rgb = T.replay_scene(api, sky, device=None, fog=scene == "fog")
        model = T.replay_model(api, sc, spec, rgb, sky)
    seeds = T.TL.replay_seeds()
    want, _, ties = model.render(seeds, T.REPLAY["bounces"], T.REPLAY["spp"], api.NEE_STRATEGIES["mis"])
    seen = {k: int(v[~ties].sum()) for k, v in model.pixel_events.items() if v[~ties].sum()}
    print("%s: near-tie share %.2f %% (%d of %d); events in the kept pixels: %s" % (scene, 100.0 * ties.mean(), int(ties.sum()), ties.size, seen))
    assert ties.mean() < 0.10
    assert np.isfinite(want).all() and want[~ties].mean() > 0.0
    need = {"box": ("sphere_end", "sun_miss", "area_sample", "sphere_blocks"), "box_sky": ("sphere_end", "sun_miss", "area_sample"),
            "fog": ("scatter", "scatter_light", "sphere_end", "sphere_end_scatter", "area_sample"),
            "glossy": ("sphere_end_rough", "area_glossy", "area_ng_reject", "sphere_blocks")}[scene]
    for name in need:
        assert seen.get(name, 0) > 0, name
