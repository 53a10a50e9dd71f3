"""The analytic lights of Scene.set_lights on host-only contexts (the record, its checks, the selection table, P_ana and the refusals of
the other render paths; include/pt_api.h), the cone of tests/lights_ref.py and SceneSpec.lights: no device needed."""

import ctypes as C
import os

import numpy as np
import pytest

import lights_ref as L

# (the library is imported inside the tests, through conftest's `api` fixture: see tests/test_lens_host.py)

NEW_SYMBOLS = ["pt_lights_defaults", "pt_set_lights", "pt_clear_lights", "pt_debug_lights"]


def test_abi_has_the_new_symbols_and_the_record(api):
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTS and hasattr(api.LIB, name)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pt_api.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header
    for text in ("#define PT_LIGHT_POINT 0", "#define PT_LIGHT_DIRECTIONAL 1", "#define PT_LIGHTS_MAX 4096"):
        assert text in header
    assert (api.LIGHT_POINT, api.LIGHT_DIRECTIONAL, api.LIGHTS_MAX) == (0, 1, 4096)
    assert C.sizeof(api.Light) == 52 and C.sizeof(api.LightsParams) == 4
    assert [n for n, _ in api.Light._fields_] == ["type", "position", "direction", "intensity", "cos_inner", "cos_outer", "weight"]
    p = api.LightsParams(7.0)
    api.LIB.pt_lights_defaults(C.byref(p))
    assert p.select == 0.5 and api.lights_defaults() == {"select": 0.5}


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


def test_set_lights_checks_its_arguments(api):
    sc = host_scene(api)
    good = api.spot_light((1, 2, 3), (0, -1, 0), (5, 5, 5), 20, 30)
    sc.set_lights([good])
    nan, inf = float("nan"), float("inf")

    def changed(**kw):
        l = api.Light.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(l, k, (C.c_float * 3)(*v) if isinstance(v, tuple) else v)
        return l
    bad = [changed(type=2), changed(type=-1), changed(position=(nan, 0, 0)), changed(position=(0, inf, 0)), changed(direction=(0, nan, 0)),
           changed(intensity=(1, 1, inf)), changed(intensity=(1, -0.5, 1)), changed(cos_inner=nan), changed(cos_outer=nan), changed(weight=nan),
           changed(weight=inf), changed(weight=-1.0), changed(cos_inner=0.5, cos_outer=0.6), changed(cos_inner=1.5), changed(cos_outer=-1.5),
           changed(direction=(0, 0, 0)), changed(type=1, direction=(0, 0, 0), cos_inner=-1.0, cos_outer=-1.0)]
    for l in bad:
        with pytest.raises(api.PtError) as e:
            sc.set_lights([good, l])
        assert e.value.code == api.PT_EINVAL and "pt_set_lights" in str(e.value) and "light 1" in str(e.value)
    for select in (-0.1, 1.1, nan):
        with pytest.raises(api.PtError) as e:
            sc.set_lights([good], select=select)
        assert e.value.code == api.PT_EINVAL and "select" in str(e.value)
    arr = (api.Light * 1)(good)
    assert api.LIB.pt_set_lights(sc._h, arr, api.LIGHTS_MAX + 1, None) == api.PT_EINVAL
    assert api.LIB.pt_set_lights(sc._h, arr, -1, None) == api.PT_EINVAL
    assert api.LIB.pt_set_lights(sc._h, None, 1, None) == api.PT_EINVAL
    assert api.LIB.pt_set_lights(None, arr, 1, None) == api.PT_EINVAL and api.LIB.pt_clear_lights(None) == api.PT_EINVAL
    # a refused call leaves the set as it was
    assert len(sc.debug_lights()["cdf"]) == 1
    # a zero direction is fine where it is not read; the whole range of cosines; the largest set
    sc.set_lights([api.point_light((0, 0, 0), (1, 1, 1)), changed(cos_inner=1.0, cos_outer=-1.0, direction=(0, 0, 0)), changed(cos_inner=1.0, cos_outer=1.0)])
    sc.set_lights([good] * api.LIGHTS_MAX)
    assert len(sc.debug_lights()["cdf"]) == api.LIGHTS_MAX
    assert api.LIB.pt_set_lights(sc._h, arr, 1, None) == api.PT_OK          # params NULL: the defaults
    sc.set_lights([])
    assert len(sc.debug_lights()["cdf"]) == 0
    sc.clear_lights()


def test_debug_lights_records_and_selection_table(api):
    sc = host_scene(api)
    lights = [api.point_light((1, 2, 3), (3, 2, 1)),                                   # automatic weight 6
              api.spot_light((4, 5, 6), (0, -2, 0), (1, 1, 1), 20, 30, weight=2.5),
              api.point_light((0, 0, 0), (0, 0, 0)),                                   # black
              api.directional_light((3, 0, -4), (0.5, 0.25, 0.25)),                    # automatic weight 1
              api.point_light((9, 9, 9), (0, 0, 0))]                                   # black, last
    sc.set_lights(lights, select=0.3)
    d = sc.debug_lights()
    rec, cdf, pl = d["records"], d["cdf"], d["P_light"]
    assert rec.shape == (5, 16) and cdf.dtype == np.float32
    assert rec[:, 3].copy().view(np.int32).tolist() == [0, 0, 0, 1, 0]
    assert rec[0, :3].tolist() == [1, 2, 3] and rec[0, 4:8].tolist() == [0, 0, 0, -1] and rec[0, 8:12].tolist() == [3, 2, 1, -1]
    assert rec[1, 4:7].tolist() == [0, -1, 0]                                          # normalised
    assert rec[1, 7] == np.float32(np.cos(np.radians(20.0))) and rec[1, 11] == np.float32(np.cos(np.radians(30.0)))
    assert np.allclose(rec[3, 4:7], [0.6, 0, -0.8], rtol=0, atol=1e-7) and rec[3, 7] == -1 and rec[3, 11] == -1 and not rec[3, :3].any()
    assert np.array_equal(rec[:, 12], pl) and not rec[:, 13:].any()
    # the cdf ends at 1, P_light sums to 1 and obeys the counting rule; black lights are never picked
    want_cdf, want_pl = L.selection_table([6.0, 2.5, 0.0, 1.0, 0.0])
    assert cdf[-1] == 1.0 and np.array_equal(cdf, want_cdf)
    assert np.array_equal(pl, want_pl.astype(np.float32)) and float(pl.astype(np.float64).sum()) == 1.0
    assert pl[2] == 0.0 and pl[4] == 0.0 and (pl[[0, 1, 3]] > 0).all()
    up = np.ceil(cdf.astype(np.float64) * 2.0 ** 24)
    assert np.array_equal(pl.astype(np.float64) * 2.0 ** 24, np.diff(np.concatenate([[0.0], up])))
    parsed = L.parse_records(rec)
    assert [p["type"] for p in parsed] == [0, 0, 0, 1, 0] and parsed[1]["P_light"] == float(pl[1])


def test_P_ana(api):
    from opencl_path_tracer_amd import scenes
    lit, black = api.point_light((500, 900, 500), (9, 9, 9)), api.point_light((0, 0, 0), (0, 0, 0))
    counted = lambda s: float(np.ceil(float(np.float32(s)) * 2.0 ** 24) / 2.0 ** 24)
    box = host_scene(api)                                    # the box has its lamp
    for select in (0.5, 0.3, 1.0, 0.0, 1e-9):
        box.set_lights([lit, black], select=select)
        assert box.debug_lights()["P_ana"] == counted(select), select
    box.set_lights([black, black])
    assert box.debug_lights()["P_ana"] == 0.0 and not box.debug_lights()["P_light"].any()
    box.clear_lights()
    assert box.debug_lights()["P_ana"] == 0.0
    dark = host_scene(api, scenes.cornell_box(8, 4, lamp="point"))         # no emitter, no sky: forced to 1
    dark.set_lights([lit], select=0.25)
    assert dark.debug_lights()["P_ana"] == 1.0
    dark.set_lights([black])
    assert dark.debug_lights()["P_ana"] == 0.0
    dark.set_lights([lit], select=0.25)
    dark.set_environment(np.zeros((2, 4, 3), dtype=np.float32))          # a sky without a distribution is no sky
    assert dark.debug_lights()["P_ana"] == 1.0
    dark.set_environment(np.ones((2, 4, 3), dtype=np.float32))
    assert dark.debug_lights()["P_ana"] == 0.25
    dark.upload_Triangles()                                              # uploads keep the set
    dark.upload_Materials()
    assert dark.debug_lights()["P_ana"] == 0.25 and len(dark.debug_lights()["cdf"]) == 1


def test_cone_function():
    ci, co = np.cos(np.radians(20.0)), np.cos(np.radians(40.0))
    assert L.cone_factor(1.0, ci, co) == 1.0 and L.cone_factor(ci, ci, co) == 1.0
    assert L.cone_factor(co, ci, co) == 0.0 and L.cone_factor(-1.0, ci, co) == 0.0
    mid = 0.5 * (ci + co)
    assert abs(L.cone_factor(mid, ci, co) - 0.5) < 1e-15
    s = 0.25
    assert abs(L.cone_factor(co + s * (ci - co), ci, co) - s * s * (3 - 2 * s)) < 1e-15
    cs = np.linspace(co, ci, 101)
    f = np.array([L.cone_factor(c, ci, co) for c in cs])
    assert (np.diff(f) >= 0).all() and f[0] == 0.0 and f[-1] == 1.0
    for c in (-1.0, -0.3, 0.0, 1.0):                                     # -1, -1: an omnidirectional light
        assert L.cone_factor(c, -1.0, -1.0) == 1.0
    assert L.cone_factor(0.5, 0.5, 0.5) == 1.0 and L.cone_factor(0.4999, 0.5, 0.5) == 0.0      # a hard edge
    assert L.cone_factor(np.float32(mid), np.float32(ci), np.float32(co)).dtype == np.float32


def test_refusals_come_before_the_device_check(api):
    sc = host_scene(api)
    sc.iterations = 4
    calls = (lambda: sc.render(1), lambda: sc.trace_rays(), lambda: sc.generate_rays(), lambda: sc.render_adaptive(2, 4, 0.1),
             lambda: sc.render_adaptive(2, 4, 0.1, path="render"), lambda: sc.render_nee(1, "bsdf"),
             lambda: sc.render_adaptive(2, 4, 0.1, path="nee", metric="half", strategy="bsdf"))
    nee_calls = (lambda: sc.render_nee(1, "mis"), lambda: sc.render_nee(1, "light"),
                 lambda: sc.render_adaptive(2, 4, 0.1, path="nee", metric="half", strategy="mis"))

    def codes(cs):
        out = []
        for call in cs:
            with pytest.raises(api.PtError) as e:
                call()
            out.append((e.value.code, str(e.value)))
        return out
    before = codes(calls)
    assert all(c == api.PT_ENODEVICE for c, _ in before)
    sc.set_lights([api.point_light((500, 900, 500), (9, 9, 9))])
    for code, text in codes(calls):
        assert code == api.PT_EINVAL and "pt_clear_lights" in text
    assert all(c == api.PT_ENODEVICE for c, _ in codes(nee_calls))       # the NEE paths do not refuse; neither do the guides
    assert all(c == api.PT_ENODEVICE for c, _ in codes((lambda: sc.render_aovs(1, 4),)))
    sc.set_lights([api.point_light((0, 0, 0), (0, 0, 0))])               # only black lights: nothing to drop
    assert codes(calls) == before
    sc.set_lights([api.point_light((500, 900, 500), (9, 9, 9))])
    sc.clear_lights()
    assert codes(calls) == before


def test_scene_spec_lights_round_trip_through_load(api):
    from opencl_path_tracer_amd import scenes
    quad = scenes.cornell_box(8, 4)
    assert quad.lights == [] and quad.objects[0][0].shape[0] == 12       # the default keeps the lamp quad
    E = np.asarray(scenes.BUILTIN_MATERIALS[scenes.LAMP][2], dtype=np.float64)
    for lamp, power in (("point", lambda I: 4 * np.pi * I), ("spot", lambda I: 2 * np.pi * I * (1 - 0.5 + 0.25))):
        spec = scenes.cornell_box(8, 4, lamp=lamp)
        assert spec.objects[0][0].shape[0] == 10 and not (spec.objects[0][1] == scenes.LAMP).any()
        sc = api.Scene(16, 16, device=None).load(spec)
        d = sc.debug_lights()
        assert len(d["cdf"]) == 1 and d["P_ana"] == 1.0 and d["P_light"][0] == 1.0
        rec = L.parse_records(d["records"])[0]
        assert rec["type"] == L.POINT and rec["position"].tolist() == [500.0, scenes.LAMP_LIGHT_Y, 500.0]
        assert np.allclose(power(rec["intensity"]), np.pi * E * 400.0 * 400.0, rtol=1e-6)      # the quad's total power
        assert (rec["cos_outer"] == -1.0) == (lamp == "point")
    with pytest.raises(ValueError):
        scenes.cornell_box(8, 4, lamp="sun")
    spec = scenes.cornell_box(8, 4)
    spec.lights = [dict(kind="directional", direction=(0, -1, 0), irradiance=(1, 2, 3)), dict(kind="point", position=(1, 1, 1), intensity=(2, 2, 2), weight=4)]
    spec.lights_select = 0.75
    d = api.Scene(16, 16, device=None).load(spec).debug_lights()
    assert [r["type"] for r in L.parse_records(d["records"])] == [L.DIRECTIONAL, L.POINT] and d["P_ana"] == 0.75
    assert np.array_equal(d["cdf"], np.array([0.6, 1.0], dtype=np.float32))
