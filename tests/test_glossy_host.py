"""The rough metal of option glossy on host-only contexts (pt_material_roughness, the option and its refusals, scenes.cornell_box(glossy=True);
include/pt_api.h): no device needed."""

import os

import numpy as np
import pytest

from opencl_path_tracer_amd import api, scenes

NEW_SYMBOLS = ["pt_material_roughness", "pt_debug_glossy"]


def test_abi_has_the_new_symbols():
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTS and hasattr(api.LIB, name)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pt_api.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header


@pytest.mark.parametrize("shininess", [0.0, 6.0, 50.0, 2220.0, 1e9, -1.0, float("nan"), float("inf")])
def test_material_roughness_is_the_double_formula(shininess):
    """0 sits on the upper clamp (sqrt(2 / 2) = 1), 2220 just above the lower one (sqrt(2 / 2222) = 0.0300015..), 1e9 far below it; 6 gives
    0.5 exactly, 50 an inexact root; negative and non-finite values give 1."""
    s = float(np.float32(shininess))
    if not np.isfinite(s) or s < 0:
        want = np.float32(1.0)
    else:
        want = np.float32(min(1.0, max(0.03, np.sqrt(2.0 / (s + 2.0)))))
    got = np.float32(api.material_roughness(shininess))
    assert got.view(np.uint32) == want.view(np.uint32), (shininess, got, want)
    assert np.float32(0.03) <= got <= np.float32(1.0)


def test_roughness_covers_both_clamps():
    assert api.material_roughness(0.0) == 1.0
    assert api.material_roughness(6.0) == 0.5
    assert np.float32(api.material_roughness(1e9)) == np.float32(0.03)
    assert np.float32(0.03) < np.float32(api.material_roughness(2220.0)) < np.float32(0.030003)


def host_scene(spec=None):
    sc = api.Scene(16, 16, device=-1)
    spec = spec or scenes.cornell_box(8, 4, glossy=True)
    for m in spec.materials:
        sc.add_Material(*m)
    for verts, mati in spec.objects:
        sc.add_Triangles(api.triangles_from_vertices(verts, mati))
        sc.end_Obj()
    sc.upload_Triangles()
    sc.upload_Materials()
    return sc


def test_option_is_accepted_on_a_host_only_context():
    sc = host_scene()
    sc.set_option("glossy", 1)
    sc.set_option("glossy", 0)
    for bad in (2, -1):
        with pytest.raises(api.PtError) as e:
            sc.set_option("glossy", bad)
        assert e.value.code == api.PT_EINVAL and "glossy" in str(e.value)


def test_refusals_come_before_the_device_check():
    sc = host_scene()
    sc.iterations = 4
    calls = (lambda: sc.render(1), lambda: sc.trace_rays(), lambda: sc.generate_rays(), lambda: sc.render_adaptive(2, 4, 0.1),
             lambda: sc.render_adaptive(2, 4, 0.1, path="render"))
    sc.set_option("glossy", 1)
    for call in calls:
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_EINVAL and "glossy" in str(e.value)
    # the NEE paths do not refuse: a host-only context has no device for them
    for call in (lambda: sc.render_nee(1, "mis"), lambda: sc.render_adaptive(2, 4, 0.1, path="nee", metric="half")):
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_ENODEVICE
    with pytest.raises(api.PtError) as e:
        sc.debug_glossy(np.zeros((1, 9), dtype=np.float32))
    assert e.value.code == api.PT_ENODEVICE
    sc.set_option("glossy", 0)
    for call in calls:
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_ENODEVICE


def test_cornell_box_glossy_has_exactly_one_type_4_material():
    plain, spec = scenes.cornell_box(8, 4), scenes.cornell_box(8, 4, glossy=True)
    types = [m[6] for m in spec.materials]
    assert types.count(4) == 1 and [m[6] for m in plain.materials].count(4) == 0
    g = types.index(4)
    assert spec.materials[:len(plain.materials)] == plain.materials and g == len(plain.materials)
    assert spec.materials[g][5] == 50.0 and spec.materials[g][:5] == tuple(plain.materials[scenes.CHROMIUM][:5])
    # the chromium sphere, and only it, wears the copy
    assert (spec.objects[1][1] == g).all() and not (spec.objects[0][1] == g).any() and not (spec.objects[2][1] == g).any()
    assert (plain.objects[1][1] == scenes.CHROMIUM).all()
    for (v, _), (pv, _) in zip(spec.objects, plain.objects):
        assert np.array_equal(v, pv)
