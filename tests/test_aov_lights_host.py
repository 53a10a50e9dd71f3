"""No GPU: the lit guide buffers (option aov_lights; include/pt_api.h pins them) on a host-only context -- the option's values, the
guide calls' refusals in their order, the area-light calls as before -- and the margins of the authored GPU scenes
(tests/aov_lights_scenes.py) in the float64 restatement of the rule (tests/aov_lights_ref.py): no per-pixel decision of any of them
lies within 1e-3 relative of its other outcome, so that no bit-for-bit comparison of tests/test_gpu_aov_lights.py can hinge on a
rounding."""
import ctypes as C

import numpy as np
import pytest

import aov_lights_ref as AL
import aov_lights_scenes as SC
import denoise_ref as DR

MARGIN = 1e-3


def test_option_values(api, cb_spec):
    sc = api.Scene(16, 12, device=None).load(cb_spec)
    for v in (0, 1, 0):
        sc.set_option("aov_lights", v)
    for v in (-1, 2, 7):
        assert api.LIB.pt_set_option(sc._h, b"aov_lights", v) == api.PT_EINVAL
        assert b"aov_lights" in api.LIB.pt_last_error(sc._h)
    assert sc.stat("aov_lights") == 0            # no guide launch yet


@pytest.mark.parametrize("option", [0, 1])
def test_guide_calls_refuse_in_the_same_order(api, cb_spec, option):
    """the argument checks first, then PT_ENODEVICE, with the option on or off and with a set held"""
    sc = api.Scene(16, 12, device=None).load(cb_spec)
    sc.set_option("aov_lights", option)
    sc.set_area_lights([api.sphere_light((500.0, 800.0, 0.0), 50.0, radiance=(5.0, 5.0, 5.0))])
    cam = api._ptr(sc.camera)
    for sub, depth in ((0, 4), (9, 4), (1, -1), (1, 17)):
        assert api.LIB.pt_render_aovs(sc._h, cam, sub, depth) == api.PT_EINVAL
        p = api.AovParams(sub, depth, api.PT_AOV_SHADED)
        assert api.LIB.pt_render_aovs_ex(sc._h, cam, C.byref(p)) == api.PT_EINVAL
    assert api.LIB.pt_render_aovs_ex(sc._h, cam, None) == api.PT_EINVAL
    assert api.LIB.pt_render_aovs_ex(sc._h, cam, C.byref(api.AovParams(1, 4, 2))) == api.PT_EINVAL      # shading stays 0 or 1
    assert api.LIB.pt_render_aovs(sc._h, cam, 1, 4) == api.PT_ENODEVICE
    for shading in (api.PT_AOV_GEOMETRIC, api.PT_AOV_SHADED):
        assert api.LIB.pt_render_aovs_ex(sc._h, cam, C.byref(api.AovParams(2, 4, shading))) == api.PT_ENODEVICE
    assert sc.stat("aov_lights") == 0
    with pytest.raises(api.PtError) as e:        # no guides: the consumers refuse as before
        sc.denoise()
    assert e.value.code in (api.PT_EINVAL, api.PT_ENODEVICE)


def test_area_light_calls_behave_as_before(api, cb_spec):
    sc = api.Scene(16, 12, device=None).load(cb_spec)
    lights = [api.sphere_light((500.0, 800.0, 0.0), 50.0, radiance=(5.0, 4.0, 3.0)), api.sun_light((0.0, -1.0, 0.0), 2.0, radiance=1.0)]
    tables = []
    for option in (0, 1):
        sc.set_option("aov_lights", option)
        sc.set_area_lights(lights, select=0.25)
        tables.append(sc.debug_area_lights())
        sc.clear_area_lights()
        assert len(sc.debug_area_lights()["records"]) == 0
        assert api.LIB.pt_set_area_lights(sc._h, None, 1, None) == api.PT_EINVAL
    for k in tables[0]:
        assert np.array_equal(tables[0][k], tables[1][k]), k
    assert tables[0]["n_sphere"] == 1 and len(tables[0]["records"]) == 2


def _margins(api, spec, W, H, offsets, depth, smooth):
    lit = SC.model_of(api, spec, W, H, SC.host_area(api, spec))
    alb, nd, near, margin, light, _ = AL.replay(lit, np.arange(W * H), offsets, depth, smooth, False)
    return AL.closest_margin(margin), near, light, nd


@pytest.mark.parametrize("name", sorted(SC.primary_scenes()))
def test_primary_scenes_decide_with_a_margin(api, name):
    spec, W, H = SC.primary_scenes()[name]
    cm, near, light, nd = _margins(api, spec, W, H, [(0.5, 0.5)], 4, False)
    print("%s: smallest relative margin %.3g; %d pixels on a light" % (name, float(cm.min()), int((light >= 0).sum())))
    assert cm.min() >= MARGIN and not near.any()
    seen = set(int(j) for j in light if j >= 0)
    want = {"front": {0}, "nothing": {0}, "hidden": set(), "two": {0, 1}, "inside": {1}, "sixtyfour": set(range(64)), "suns": {0, 1}}[name]
    assert seen == want
    if name == "nothing":
        assert (nd[:, 3] > 0).sum() == (light == 0).sum() > 0          # the only hits are the sphere's
    if name == "two":                                                    # (the nearer sphere is record 1: it hides part of record 0)
        assert (light == 1).sum() > 4 and (light == 0).sum() > 4


@pytest.mark.parametrize("sub", [1, 2])
@pytest.mark.parametrize("smooth", [False, True])
def test_chain_scene_decides_with_a_margin(api, sub, smooth):
    spec = SC.chain_spec()
    cm, near, light, nd = _margins(api, spec, SC.CHAIN["W"], SC.CHAIN["H"], DR.subpixel_offsets(sub), SC.CHAIN["depth"], smooth)
    print("chain, subpixels %d, smooth %s: smallest relative margin %.3g" % (sub, smooth, float(cm.min())))
    assert cm.min() >= MARGIN and not near.any()
    assert all((light == j).any() for j in range(4))                    # through the glass, in the mirror, in front of it, the sun in it


def test_ref_by_hand(api):
    """one ray of the rule by hand: a unit sphere at distance 5 on the axis, a wall behind it at 10"""
    spec = SC._spec("hand", SC.wall_at(10.0), [0, 0], [SC.sphere((0.0, 0.0, 5.0), 1.0, (2.0, 3.0, 4.0)), SC.sun((0.0, 0.0, 1.0), 10.0, (1.0, 1.0, 1.0))])
    lit = SC.model_of(api, spec, 2, 2, SC.host_area(api, spec))
    lit.begin()
    ti, t, _ = lit.intersect(np.zeros(3), np.array([0.0, 0.0, 1.0]))
    assert ti == lit.slot and abs(t - 4.0) < 1e-12 and lit.end == ("sphere", 0, True)
    assert np.allclose(lit.n[lit.slot], (0.0, 0.0, -1.0)) and np.allclose(lit.mats[len(lit.model.mats)]["kd"], (2.0, 3.0, 4.0))
    assert abs(lit.margin["t_tri"] - 0.6) < 1e-12 and abs(lit.margin["disc"] - 1.0 / 25.0) < 1e-12
    lit.begin()
    ti, t, _ = lit.intersect(np.array([0.0, 0.0, 11.0]), np.array([0.0, 0.0, 1.0]))      # past the wall: only the sun
    assert ti == lit.slot and lit.end == ("sun", 1, True) and lit.margin["sun"] > 0.99
    c = AL.trace_chain(lit, 0, 0.5, 0.5, 4, False, False)                # pixel 0 looks down and left of the sphere: the wall
    assert c["light"] == -1 and c["mat"] == 0 and abs(c["t"] - 10.0 * np.linalg.norm(SC.pixel_direction(0, 0, 2, 2) / SC.pixel_direction(0, 0, 2, 2)[2])) < 1e-5
