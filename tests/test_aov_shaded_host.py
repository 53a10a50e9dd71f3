"""Host side of the shaded guide buffers (pt_aov_defaults, pt_render_aovs_ex; include/pt_api.h): the defaults, the argument checks,
which come before the device check, and the Python keyword.  No GPU: every context here is host-only."""
import ctypes as C

import pytest


def _scene(api):
    from opencl_path_tracer_amd import scenes
    return api.Scene(16, 16, device=-1).load(scenes.cornell_box(segments=8, rings=4))


def _ex(api, sc, params):
    return api.LIB.pt_render_aovs_ex(sc._h, api._ptr(sc.camera), None if params is None else C.byref(params))


def test_defaults(api):
    p = api.AovParams(-7, -7, -7)
    api.LIB.pt_aov_defaults(C.byref(p))
    assert (p.subpixels, p.specular_depth, p.shading) == (1, 4, api.PT_AOV_GEOMETRIC)
    assert api.aov_defaults() == {"subpixels": 1, "specular_depth": 4, "shading": 0}
    assert (api.PT_AOV_GEOMETRIC, api.PT_AOV_SHADED) == (0, 1)
    api.LIB.pt_aov_defaults(None)                                # tolerated, like the other defaults


def test_python_defaults_are_the_c_defaults(api):
    import inspect
    sig = inspect.signature(api.Scene.render_aovs).parameters
    d = api.aov_defaults()
    assert sig["subpixels"].default == d["subpixels"] and sig["specular_depth"].default == d["specular_depth"]
    assert api.AOV_SHADING[sig["shading"].default] == d["shading"]


@pytest.mark.parametrize("bad", [None, (0, 4, 0), (9, 4, 1), (-1, 4, 1), (1, -1, 0), (1, 17, 1), (1, 4, 2), (1, 4, -1), (0, 4, 1)])
def test_bad_arguments_are_einval_before_the_device(api, bad):
    sc = _scene(api)
    rc = _ex(api, sc, None if bad is None else api.AovParams(*bad))
    assert rc == api.PT_EINVAL, (bad, rc)
    assert b"pt_render_aovs_ex" in api.LIB.pt_last_error(sc._h)
    assert api.LIB.pt_render_aovs_ex(None, api._ptr(sc.camera), C.byref(api.AovParams(1, 4, 1))) == api.PT_EINVAL
    sc.close()


@pytest.mark.parametrize("good", [(1, 4, 0), (1, 4, 1), (8, 16, 1), (1, 0, 1), (8, 0, 0)])
def test_good_arguments_reach_the_device_check(api, good):
    sc = _scene(api)
    assert _ex(api, sc, api.AovParams(*good)) == api.PT_ENODEVICE, good
    sc.close()


def test_python_keyword(api):
    sc = _scene(api)
    for shading in ("geometric", "shaded"):
        with pytest.raises(api.PtError) as e:
            sc.render_aovs(1, 4, shading=shading)
        assert e.value.code == api.PT_ENODEVICE
    with pytest.raises(api.PtError) as e:
        sc.render_aovs(9, 4, shading="shaded")
    assert e.value.code == api.PT_EINVAL
    for bad in ("smooth", "", "SHADED", None, 1):
        with pytest.raises(ValueError):
            sc.render_aovs(1, 4, shading=bad)
    sc.close()


def test_authoring_calls_work_on_a_host_only_context_as_before(api):
    """the staleness rule of the shaded guides adds nothing a host-only context could trip over"""
    import numpy as np
    sc = _scene(api)
    sc.set_vertex_normals(np.ones((1, 3, 3), dtype=np.float32))
    sc.clear_vertex_normals()
    sc.compute_vertex_normals(30.0)
    sc.set_vertex_uvs(np.zeros((1, 3, 2), dtype=np.float32))
    sc.clear_vertex_uvs()
    t = sc.add_texture(np.ones((1, 1, 3), dtype=np.float32))
    sc.set_material_texture(0, t)
    sc.clear_textures()
    sc.close()
