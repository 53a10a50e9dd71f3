"""-m gpu: point, spot and directional lights in Scene.render_nee and Scene.render_adaptive(path="nee") (pt_set_lights, the lights
instances of k_nee in pt_nee.hip; include/pt_api.h pins the set, the selection and the estimator).

  1 without a pickable light render_nee computes the bits it computed before; 2 strategies light and mis against tests/lights_ref.py
  (float64, brute force, same LCG and hashes) on a scene of 13 triangles, with and without a sky; 3 closed forms on a diffuse floor:
  a directional light, a point light, an occluder's shadow and a spot's cone; 4 the same mean in light and mis next to a real emitter,
  with pt_render's rnds and rays; 5 determinism, the flat preview, adaptive tiles, tiled ranks, and the variance / guide / denoise /
  temporal passes on a light-lit frame."""

import numpy as np
import pytest

import lights_ref as L
import nee_ref as R

pytestmark = pytest.mark.gpu

CB_BOUNCES = 8
EYE_AT_ORIGIN = (-500.0, -500.0, 1299.0378)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def state(sc):
    rays = sc.read_rays()
    return sc.read_colors().copy(), sc.read_rnds().copy(), rays["P"][:, :3].copy(), rays["D"][:, :3].copy()


def same_state(a, b):
    return same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2]) and same_bits(a[3], b[3])


def box_light(api):
    return api.point_light((200.0, 800.0, 100.0), (4e6, 3e6, 2e6))


# ---------------------------------------------------------------------------- 1: no change without lights
def test_no_lights_no_change(api, cb_spec):
    W, H = 48, 40
    black = [api.point_light((500.0, 900.0, 500.0), (0, 0, 0)), api.directional_light((0, -1, 0), (0, 0, 0))]
    for strategy in ("bsdf", "light", "mis"):
        fresh = api.Scene(W, H).load(cb_spec)
        fresh.iterations = CB_BOUNCES
        fresh.render_nee(3, strategy)
        want = state(fresh)
        cleared = api.Scene(W, H).load(cb_spec)
        cleared.set_lights([box_light(api)])
        cleared.clear_lights()
        dark = api.Scene(W, H).load(cb_spec)
        dark.set_lights(black)
        for sc in (cleared, dark):
            sc.iterations = CB_BOUNCES
            sc.render_nee(3, strategy)
            assert same_state(state(sc), want), strategy
        if strategy == "bsdf":
            continue
        lit = api.Scene(W, H).load(cb_spec)              # and a real light does change the frame
        lit.set_lights([box_light(api)])
        lit.iterations = CB_BOUNCES
        lit.render_nee(3, strategy)
        assert not same_bits(lit.read_colors(), want[0])
        assert np.array_equal(lit.read_rnds(), want[1])


FAMILY_CASES = {       # cornell_box arguments, options, lens: what the frame would launch without lights, and the flags a lights launch reads
    "plain": (dict(), {}, False),
    "smooth_textures": (dict(smooth=True, textured=True), {"smooth_normals": 1, "textures": 1}, False),
    "glossy": (dict(smooth=True, glossy=True), {"smooth_normals": 1, "glossy": 1}, False),                  # flags bit 0
    "coated": (dict(glossy=True, coated=True), {"glossy": 1, "coated": 1}, False),                         # bits 0 and 1
    "coated_alone": (dict(glossy=True, coated=True), {"coated": 1}, False),                                # bit 1: type 4 inert
    "lens": (dict(glossy=True, coated=True), {"glossy": 1}, True),                                         # bits 0 and 2: type 5 inert
    "frosted": (dict(smooth=True, frosted=True), {"smooth_normals": 1, "frosted": 1}, False),              # bit 3
    "frosted_lens": (dict(glossy=True, frosted=True), {"glossy": 1, "frosted": 1}, True),                  # bits 0, 2 and 3
    "frosted_off": (dict(frosted=True), {}, False),                                                        # bit 3 clear: type 6 inert
}


@pytest.mark.parametrize("case", sorted(FAMILY_CASES))
def test_a_set_that_is_never_picked_keeps_every_familys_bits(api, case):
    """select = 0 next to the box's lamp: P_ana = 0, so the lights instances run (a pickable light is held) but never take the analytic
    branch, and every 1 - P_ana is exactly 1.  The frame must be, bit for bit, the one the family it replaces renders: what the lights
    family reads at run time -- options glossy, coated and frosted (flags bits 0, 1, 3: metal_live, coat_live, frost_live), the lens (bit 2),
    the vertex normals and the texture view -- is what those families read or have compiled in."""
    from opencl_path_tracer_amd import scenes
    W, H = 48, 40
    box, options, lens = FAMILY_CASES[case]
    spec = scenes.cornell_box(**box)
    frames = []
    for lights in (False, True):
        sc = api.Scene(W, H).load(spec)
        for k, v in options.items():
            sc.set_option(k, v)
        if lens:
            sc.set_lens(25.0, 1600.0)
        if lights:
            sc.set_lights([box_light(api)], select=0.0)
            assert sc.debug_lights()["P_ana"] == 0.0 and sc.debug_lights()["P_light"][0] == 1.0
            with pytest.raises(api.PtError) as e:          # the set is held: the lights family is what launches
                sc.render_nee(1, "bsdf")
            assert e.value.code == api.PT_EINVAL and "pt_clear_lights" in str(e.value)
        sc.iterations = CB_BOUNCES
        sc.render_nee(3, "mis")
        frames.append(state(sc))
    assert same_state(frames[0], frames[1]), case
    assert np.isfinite(frames[0][0]).all() and frames[0][0][:, :3].mean() > 0.0


# ---------------------------------------------------------------------------- 2: replay against the float64 model
def replay_spec():
    """tests/test_gpu_env.py's replay scene: a box with an open top: glossy floor, three walls, an occluder, a mirror and one emitting
    triangle (13 triangles)."""
    from opencl_path_tracer_amd import scenes
    mats = [
        ((0.6, 0.6, 0.6), (0.2, 0.2, 0.2), (0, 0, 0), (0, 0, 0), (0, 0, 0), 20.0, 0),      # 0 white, glossy lobe
        ((0.6, 0.1, 0.1), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),             # 1 red
        ((0.1, 0.6, 0.1), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),             # 2 green
        ((0, 0, 0), (0, 0, 0), (12.0, 4.0, 2.0), (0, 0, 0), (0, 0, 0), 0.0, 3),            # 3 small hot emitter
        scenes.BUILTIN_MATERIALS[scenes.CHROMIUM],                                           # 4 mirror
    ]

    def quad(a, b, c, d):
        return [(a, b, c), (a, c, d)]
    x0, x1, y0, y1, z0, z1 = -5.0, 5.0, -3.0, 5.0, -1.0, 12.0
    tris, mo = [], []
    for q, m in ((quad((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)), 0),      # floor
                 (quad((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)), 0),      # back
                 (quad((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)), 1),      # left
                 (quad((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)), 2),      # right
                 (quad((-1.0, 0.5, 5.0), (1.0, 0.5, 5.0), (1.0, 0.5, 7.0), (-1.0, 0.5, 7.0)), 0),   # occluder
                 (quad((4.95, -2.0, 8.0), (4.95, 1.0, 8.0), (4.95, 1.0, 11.0), (4.95, -2.0, 11.0)), 4)):   # mirror
        tris += q
        mo += [m] * len(q)
    tris.append(((-4.9, 2.0, 9.0), (-4.9, 3.0, 9.0), (-4.9, 2.0, 10.5)))       # the emitter, on the left wall
    mo.append(3)
    spec = scenes.SceneSpec(materials=mats, name="lights_replay", shift=EYE_AT_ORIGIN)
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.asarray(mo, dtype=np.uint16)))
    return spec


def replay_map():
    h, w = 8, 16
    rgb = np.zeros((h, w, 3), dtype=np.float32)
    rgb[...] = (0.05 + 0.3 * (np.arange(h)[:, None] / h) + 0.1 * (np.arange(w)[None, :] / w))[..., None] * np.array([0.8, 0.9, 1.0])
    rgb[1, 5] = (60.0, 50.0, 40.0)
    return rgb


REPLAY = dict(W=48, H=32, spp=2, bounces=4, scale=1.25, yaw_degrees=25.0, select=0.5)


def replay_lights(api):
    """an omnidirectional point light over the occluder, a spot whose cone edge crosses the floor, and a directional light that comes in
    through the open top"""
    return [api.point_light((0.5, 3.0, 6.0), (30.0, 28.0, 24.0)),
            api.spot_light((-2.0, 4.0, 8.0), (0.2, -1.0, 0.1), (90.0, 80.0, 60.0), 15.0, 30.0),
            api.directional_light((0.3, -1.0, 0.2), (1.5, 1.4, 1.2))]


def replay_scene(api, sky, device=0):
    W, H = REPLAY["W"], REPLAY["H"]
    spec, rgb = replay_spec(), replay_map()
    sc = api.Scene(W, H, device=device).load(spec)
    if sky:
        sc.set_environment(rgb, scale=REPLAY["scale"], yaw_degrees=REPLAY["yaw_degrees"], select=REPLAY["select"])
    sc.set_lights(replay_lights(api), select=REPLAY["select"])
    return sc, spec, rgb


def replay_model(api, sc, spec, rgb, sky):
    verts, mo = spec.objects[0]
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    env = dict(rgb=rgb, tables=sc.debug_environment(), scale=REPLAY["scale"], yaw_degrees=REPLAY["yaw_degrees"]) if sky else None
    return L.LightsModel(verts, recs["N"], mats, mo, sc.camera[0], sc.debug_lights(), env=env, table=sc.debug_light_table())


def replay_seeds():
    return np.random.default_rng(17).integers(1, 2 ** 31 - 2, REPLAY["W"] * REPLAY["H"]).astype(np.int32)


@pytest.mark.parametrize("sky", [True, False])
@pytest.mark.parametrize("strategy", ["light", "mis"])
def test_matches_float64_model(api, strategy, sky):
    """The model alone, on these seeds, flags 0.33 % (sky) / 0.26 % (no sky) of the pixels as near-ties in both strategies (measured on a
    host-only context before the first GPU run): far below the 10 % cap.  The tolerance and the cap are test_gpu_env.py's."""
    spp, bounces = REPLAY["spp"], REPLAY["bounces"]
    sc, spec, rgb = replay_scene(api, sky)
    seeds = replay_seeds()
    sc.upload_seeds(seeds)
    sc.iterations = bounces
    sc.render_nee(spp, strategy)
    model = replay_model(api, sc, spec, rgb, sky)
    assert len(model.lights) == 1 and model.pa == 0.5 and model.pe == (0.5 if sky else 0.0) and len(model.set) == 3
    want, want_seeds, ties = model.render(seeds, bounces, spp, api.NEE_STRATEGIES[strategy])
    got = sc.read_colors()[:, :3].astype(np.float64)
    keep = ~ties
    print("near-tie pixels: %d of %d" % (int(ties.sum()), ties.size))
    assert keep.mean() > 0.9, "too many near-tie pixels: %d" % int(ties.sum())
    assert np.array_equal(sc.read_rnds()[keep], want_seeds[keep])
    scale = float(want[keep].max())
    err = np.abs(got[keep] - want[keep])
    worst = float((err / (np.abs(want[keep]) + 1e-6 * scale)).max())
    print("worst relative error %g" % worst)
    bad = err > 2e-3 * np.abs(want[keep]) + 1e-6 * scale
    assert not bad.any(), "%d of %d pixel channels differ; worst %g" % (int(bad.sum()), bad.size, worst)
    assert float(want[keep].mean()) > 0.0


GLOSSY_SPHERES = [((-2.6, -1.6, 7.0), 1.4, 0), ((0.3, -1.5, 9.6), 1.5, 5), ((2.7, -1.7, 6.2), 1.3, 6), ((1.6, 1.7, 8.2), 1.0, 8)]


def glossy_replay_spec():
    """tests/test_gpu_glossy.py's replay scene: a closed box with a type-4 floor (shininess 30), a lamp quad, a small emitter, an occluder,
    a mirror, and four 8 x 4 spheres with their analytic vertex normals: white, mirror, glass and rough gold"""
    from opencl_path_tracer_amd import scenes
    chromium = scenes.BUILTIN_MATERIALS[scenes.CHROMIUM]
    mats = [
        ((0.6, 0.6, 0.6), (0.2, 0.2, 0.2), (0, 0, 0), (0, 0, 0), (0, 0, 0), 20.0, 0),      # 0 white, glossy lobe
        ((0.6, 0.1, 0.1), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),             # 1 red
        ((0.1, 0.6, 0.1), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),             # 2 green
        ((0, 0, 0), (0, 0, 0), (6.0, 5.0, 4.0), (0, 0, 0), (0, 0, 0), 0.0, 3),             # 3 lamp
        ((0, 0, 0), (0, 0, 0), (12.0, 4.0, 2.0), (0, 0, 0), (0, 0, 0), 0.0, 3),            # 4 small hot emitter
        chromium,                                                                            # 5 mirror
        scenes.BUILTIN_MATERIALS[scenes.GLASS],                                              # 6 glass
        tuple(chromium[:5]) + (30.0, 4),                                                     # 7 rough metal, alpha 0.25
        tuple(scenes.BUILTIN_MATERIALS[scenes.GOLD][:5]) + (198.0, 4),                     # 8 rough gold, alpha 0.1
    ]

    def quad(a, b, c, d):
        return [(a, b, c), (a, c, d)]
    x0, x1, y0, y1, z0, z1 = -5.0, 5.0, -3.0, 5.0, -1.0, 12.0
    tris, mo = [], []
    for q, m in ((quad((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)), 7),      # floor
                 (quad((x0, y1, z0), (x0, y1, z1), (x1, y1, z1), (x1, y1, z0)), 0),      # ceiling
                 (quad((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)), 0),      # back
                 (quad((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)), 1),      # left
                 (quad((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)), 2),      # right
                 (quad((-1.5, 4.9, 6.0), (1.5, 4.9, 6.0), (1.5, 4.9, 9.0), (-1.5, 4.9, 9.0)), 3),   # lamp
                 (quad((-1.0, 0.5, 5.0), (1.0, 0.5, 5.0), (1.0, 0.5, 7.0), (-1.0, 0.5, 7.0)), 0),   # occluder
                 (quad((4.95, -2.0, 8.0), (4.95, 1.0, 8.0), (4.95, 1.0, 11.0), (4.95, -2.0, 11.0)), 5)):   # mirror
        tris += q
        mo += [m] * len(q)
    tris.append(((-4.9, 2.0, 9.0), (-4.9, 3.0, 9.0), (-4.9, 2.0, 10.5)))       # small emitter on the left wall
    mo.append(4)
    spec = scenes.SceneSpec(materials=mats, name="lights_glossy_replay", shift=EYE_AT_ORIGIN)
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.asarray(mo, dtype=np.uint16)))
    spec.normals = [None]
    for c, r, m in GLOSSY_SPHERES:
        v = scenes.uv_sphere(c, r, 8, 4)
        spec.objects.append((v, np.full(len(v), m, dtype=np.uint16)))
        spec.normals.append(scenes.uv_sphere_normals(c, r, 8, 4))
    return spec


def glossy_replay_lights(api):
    """inside the closed box: a point light beside the occluder, a spot onto the floor between the spheres, and a weak directional
    light that only reaches what the ceiling does not shade (nothing: it tests the uncut shadow ray)"""
    return [api.point_light((-0.5, 3.0, 4.0), (30.0, 28.0, 24.0)),
            api.spot_light((1.0, 4.0, 8.0), (-0.1, -1.0, -0.1), (90.0, 80.0, 60.0), 20.0, 40.0),
            api.directional_light((0.3, -1.0, 0.2), (1.5, 1.4, 1.2))]


def glossy_replay_scene(api, device=0):
    spec = glossy_replay_spec()
    sc = api.Scene(REPLAY["W"], REPLAY["H"], device=device).load(spec)
    sc.set_option("smooth_normals", 1)
    sc.set_option("glossy", 1)
    sc.set_lights(glossy_replay_lights(api), select=REPLAY["select"])
    return sc, spec


def glossy_replay_model(api, sc, spec):
    verts = np.concatenate([v for v, _ in spec.objects])
    mo = np.concatenate([m for _, m in spec.objects])
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    vn = np.concatenate([np.zeros(v.shape, dtype=np.float32) if n is None else n for (v, _), n in zip(spec.objects, spec.normals)])
    return L.LightsModel(verts, recs["N"], mats, mo, sc.camera[0], sc.debug_lights(), vnormals=vn, table=sc.debug_light_table())


def test_matches_float64_model_under_smooth_normals_and_glossy(api):
    """Options smooth_normals + glossy on tests/test_gpu_glossy.py's replay scene (a type-4 floor, spheres with vertex normals) with the
    three lights inside the box, strategy mis.  The model alone, on these seeds, flags 1.3 % of the pixels as near-ties (measured
    on a host-only context before the first GPU run; cap 10 %); in the kept pixels it takes 911 delta samples, 211 of them weighted at
    a rough vertex and 19 more refused by the geometric side under a shading normal, next to 1,860 glossy vertices, 555 light samples
    at one, 22 emitter hits after one with W_b < 1 and 44 specular fall-backs to Ng."""
    spp, bounces = REPLAY["spp"], REPLAY["bounces"]
    sc, spec = glossy_replay_scene(api)
    seeds = replay_seeds()
    sc.upload_seeds(seeds)
    sc.iterations = bounces
    sc.render_nee(spp, "mis")
    model = glossy_replay_model(api, sc, spec)
    assert model.pa == 0.5 and len(model.set) == 3 and len(model.lights) == 3
    want, want_seeds, ties = model.render(seeds, bounces, spp, 2)
    got = sc.read_colors()[:, :3].astype(np.float64)
    keep = ~ties
    print("near ties: %.2f %%; events in the kept pixels: %s" % (100.0 * ties.mean(), {k: int(v[keep].sum()) for k, v in model.pixel_events.items()}))
    assert keep.mean() > 0.9, "too many near-tie pixels: %d" % int(ties.sum())
    # what only this run reaches: a delta sample weighted at a rough vertex, one refused by the geometric side under a shading normal
    for name in ("delta", "delta_glossy", "delta_ng_reject", "glossy_vertex", "glossy_light", "glossy_emitter_wb", "spec_fallback"):
        assert int(model.pixel_events[name][keep].sum()) > 0, name
    assert np.array_equal(sc.read_rnds()[keep], want_seeds[keep])
    scale = float(want[keep].max())
    err = np.abs(got[keep] - want[keep])
    worst = float((err / (np.abs(want[keep]) + 1e-6 * scale)).max())
    print("worst relative error %g" % worst)
    bad = err > 2e-3 * np.abs(want[keep]) + 1e-6 * scale
    assert not bad.any(), "%d of %d pixel channels differ; worst %g" % (int(bad.sum()), bad.size, worst)
    off, _ = glossy_replay_scene(api)                  # and the material matters: with the option off the frame differs
    off.set_option("glossy", 0)
    off.upload_seeds(seeds)
    off.iterations = bounces
    off.render_nee(spp, "mis")
    assert not same_bits(off.read_colors()[:, :3], sc.read_colors()[:, :3])


# ---------------------------------------------------------------------------- 3: closed forms
FLOOR_Y, KD = -10.0, 0.5
CF_W, CF_H = 48, 36
# The relative tolerance of the closed forms: what evaluating the whole chain -- camera ray, hit point on the floor's triangles, light
# sample, kd cos (I cone / d) cos / pi -- in float32 instead of float64 changes, over every pixel the cases below compare, times 4
# (measure_float32_error() below, run on a host-only context; per case, because the directional cases involve no hit point and are exact
# to a few roundings, while the point lights inherit the float32 hit point on triangles 20,000 units wide; profiles/lights/README.md)
CF_FLOAT32_ERROR = {"down": 7.2e-8, "tilted": 6.8e-8, "point": 5.8e-5, "occluder": 5.8e-5, "spot": 7.7e-6}
CF_RTOL = {k: 4 * v for k, v in CF_FLOAT32_ERROR.items()}
# s^2 (3 - 2 s) has no relative precision at s = 0, so pixels whose cone cosine is within CONE_EDGE_BAND of cos_outer -- on either side
# of the edge -- are compared absolutely, against the value the cone factor 1 would give: CF_EDGE_ATOL is four times the same float32
# measurement over the pixels of the band
CONE_EDGE_BAND = 2e-2
CF_EDGE_FLOAT32_ERROR = 8.2e-7      # (28 pixels in the band)
CF_EDGE_ATOL = 4 * CF_EDGE_FLOAT32_ERROR


def floor_tris():
    big = 1e4
    return [((-big, FLOOR_Y, -big), (big, FLOOR_Y, big), (big, FLOOR_Y, -big)), ((-big, FLOOR_Y, -big), (-big, FLOOR_Y, big), (big, FLOOR_Y, big))]


def floor_spec(occluder=False):
    """test_gpu_env.py's floor_spec(kd): an (effectively) infinite diffuse floor 10 below a level camera, no emitter; occluder: a quad of
    the same material 4 above the floor"""
    from opencl_path_tracer_amd import scenes
    mats = [((KD, KD, KD), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0)]
    tris = floor_tris()
    if occluder:
        a, b, c, d = (-4.0, -6.0, 34.0), (4.0, -6.0, 34.0), (4.0, -6.0, 46.0), (-4.0, -6.0, 46.0)
        tris += [(a, b, c), (a, c, d)]
    spec = scenes.SceneSpec(materials=mats, fov=60.0, shift=EYE_AT_ORIGIN, name="floor")
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.zeros(len(tris), dtype=np.uint16)))
    return spec


def closed_form_cases(api):
    th = np.radians(35.0)
    return [("down", False, api.directional_light((0, -1, 0), (3.0, 2.0, 1.0))),
            ("tilted", False, api.directional_light((np.sin(th), -np.cos(th), 0.0), (3.0, 2.0, 1.0))),
            ("point", False, api.point_light((0.5, -4.0, 40.0), (400.0, 300.0, 200.0))),
            ("occluder", True, api.point_light((0.0, -2.0, 40.0), (400.0, 300.0, 200.0))),
            ("spot", False, api.spot_light((-1.0, 2.0, 40.0), (0.1, -1.0, -0.05), (900.0, 700.0, 500.0), 20.0, 35.0))]


def camera_ray(cam, gid, r1, r2, f):
    X, Y = int(cam["XM"]), int(cam["YM"])
    x, y = f(gid % X) + f(r1), f(gid // X) + f(r2)
    pp = cam["lookat"][:3].astype(f) + cam["right"][:3].astype(f) * ((f(2) * x) / f(X) - f(1)) + cam["up"][:3].astype(f) * ((f(2) * y) / f(Y) - f(1))
    eye = cam["eye"][:3].astype(f)
    d = pp - eye
    return eye, d / np.sqrt((d * d).sum(dtype=f))


def floor_hit(P, D, f):
    """the hit of (P, D) on the floor's two triangles (Moeller-Trumbore in precision f), or None"""
    for tri in floor_tris():
        v = np.asarray(tri, dtype=f)
        e1, e2 = v[1] - v[0], v[2] - v[0]
        pv = np.cross(D, e2)
        det = (e1 * pv).sum(dtype=f)
        if det == 0:
            continue
        s = P - v[0]
        u = (s * pv).sum(dtype=f) / det
        q = np.cross(s, e1)
        w = (D * q).sum(dtype=f) / det
        t = (e2 * q).sum(dtype=f) / det
        if u >= 0 and w >= 0 and u + w <= 1 and t > 0:
            return P + D * t
    return None


def closed_form_expect(api, sc, spec, seeds, f=np.float64):
    """per pixel: the formula's value in precision f (0: a miss, a shadow, or outside the cone), the same with the cone factor 1 (float64),
    whether the pixel is compared (its first hit is surely the floor, its shadow ray surely free or surely blocked), whether it is lit
    (in float64), and whether its cone cosine lies in the band around cos_outer (compared with the absolute tolerance)"""
    verts, mo = spec.objects[0]
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    cam = sc.camera[0]
    model = R.Model(verts, recs["N"], mats, mo, cam)
    light = L.parse_records(sc.debug_lights()["records"])[0]
    open_light = dict(light, cos_inner=-1.0, cos_outer=-1.0)
    spot = light["type"] == L.POINT and light["cos_outer"] > -1.0
    n = len(seeds)
    want, full = np.zeros((n, 3), dtype=f), np.zeros((n, 3))
    sure, lit, edge = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    N = np.array([0.0, 1.0, 0.0])
    for i in range(n):
        s, r1 = R.lcg(int(seeds[i]))
        s, r2 = R.lcg(s)
        P, D = model.camera_ray(i, r1, r2)
        ti, t, tie = model.intersect(P, D)
        if tie or ti >= 2:
            continue                        # (the occluder's own pixels are not compared)
        sure[i] = True
        if ti < 0:
            continue
        hp = P + D * t
        w, cut, _ = L.light_sample(open_light, hp + N * 0.001)
        hi, _, st = model.intersect(hp + N * 0.001, w, cut)
        if st:
            sure[i] = False
            continue
        if hi >= 0:
            continue                        # in the shadow: exactly 0
        if spot:
            edge[i] = abs(float(-w @ light["axis"]) - light["cos_outer"]) < CONE_EDGE_BAND
        Pf, Df = camera_ray(cam, i, r1, r2, f)
        want[i] = L.floor_radiance(KD, light, floor_hit(Pf, Df, f), N, f)
        full[i] = L.floor_radiance(KD, open_light, hp, N)
        lit[i] = L.light_sample(light, hp + N * 0.001) is not None
    return want, full, sure, lit, edge


def measure_float32_error(api, device=None):
    """per case, over the compared pixels (no GPU: a host-only context): the worst |float32 chain - float64 chain| / float64 chain off
    the cone's outer edge, and inside the band around it the worst |float32 chain - float64 chain| / (the value with the cone factor 1)"""
    worst = {}
    seeds = np.random.default_rng(41).integers(1, 2 ** 31 - 2, CF_W * CF_H).astype(np.int32)
    for name, occluder, light in closed_form_cases(api):
        spec = floor_spec(occluder)
        sc = api.Scene(CF_W, CF_H, device=device).load(spec)
        sc.set_lights([light])
        w64, full, sure, lit, edge = closed_form_expect(api, sc, spec, seeds, np.float64)
        w32 = closed_form_expect(api, sc, spec, seeds, np.float32)[0].astype(np.float64)
        sel = sure & lit & ~edge
        worst[name] = float((np.abs(w32[sel] - w64[sel]) / w64[sel]).max())
        band = sure & edge
        if band.any():
            worst[name + "_edge"] = (float((np.abs(w32[band] - w64[band]) / full[band]).max()), int(band.sum()))
    return worst


@pytest.mark.parametrize("case", ["down", "tilted", "point", "occluder", "spot"])
def test_closed_forms_on_a_floor(api, case):
    """iterations = 2, strategy light, one sample, no emitter and no sky (P_ana = 1): a floor pixel is exactly its one light sample,
    kd cos (I cone / d) (cos / pi) at that sample's own hit point -- kd E / pi under a directional light straight down, kd E cos^2 / pi under a
    tilted one, kd I cos^2 / (pi r^2) under a point light, 0 in an occluder's shadow and outside a spot's cos_outer.  Every floor pixel
    is compared: relatively off the spot's outer edge, absolutely (against the value with the cone factor 1) in the band around it."""
    name, occluder, light = [c for c in closed_form_cases(api) if c[0] == case][0]
    spec = floor_spec(occluder)
    sc = api.Scene(CF_W, CF_H).load(spec)
    sc.set_lights([light])
    assert sc.debug_lights()["P_ana"] == 1.0
    seeds = np.random.default_rng(41).integers(1, 2 ** 31 - 2, CF_W * CF_H).astype(np.int32)
    sc.upload_seeds(seeds)
    sc.iterations = 2
    sc.render_nee(1, "light")
    got = sc.read_colors()[:, :3].astype(np.float64)
    want, full, sure, lit, edge = closed_form_expect(api, sc, spec, seeds)
    assert sure.mean() > 0.8
    dark = sure & ~lit & ~edge
    assert not got[dark].any(), "%d dark pixels are lit" % int(got[dark].any(axis=1).sum())
    sel = sure & lit & ~edge
    assert sel.sum() > 50
    rel = np.abs(got[sel] - want[sel]) / want[sel]
    print("%s: %d lit, %d dark pixels compared; worst relative error %.3g (tolerance %.3g)" % (case, int(sel.sum()), int(dark.sum()), rel.max(), CF_RTOL[case]))
    assert rel.max() <= CF_RTOL[case]
    E = np.array([3.0, 2.0, 1.0])
    if case == "down":          # every floor pixel, whatever the jitter
        assert np.allclose(want[sel], KD * E / np.pi, rtol=1e-12)
        assert (got[sel] == got[sel][0]).all()
    elif case == "tilted":
        assert np.allclose(want[sel], KD * E * np.cos(np.radians(35.0)) ** 2 / np.pi, rtol=1e-6)      # (the stored direction is float32)
    elif case == "occluder":    # some floor pixels are in the shadow
        rows = np.arange(CF_W * CF_H) // CF_W
        assert (dark & (rows < CF_H // 2 - 1)).sum() > 5
    elif case == "spot":        # all three regimes of the cone are on the floor, and both sides of its outer edge
        rows = np.arange(CF_W * CF_H) // CF_W
        assert (dark & (rows < CF_H // 2 - 1)).sum() > 5
        cone = want[sel, 0] / full[sel, 0]
        assert (cone > 1 - 1e-9).sum() > 5 and ((cone > 1e-3) & (cone < 0.999)).sum() > 20
        band = sure & edge
        assert (band & lit).sum() > 3 and (band & ~lit).sum() > 3
        err = np.abs(got[band] - want[band]) / full[band]
        print("spot: %d pixels in the band around cos_outer; worst error / uncut value %.3g (tolerance %.3g)" % (int(band.sum()), err.max(), CF_EDGE_ATOL))
        assert err.max() <= CF_EDGE_ATOL


# ---------------------------------------------------------------------------- 4: the same expectation next to a real emitter
def test_light_and_mis_agree_and_keep_renders_stream(api, oracle, cb_spec):
    """The Cornell box with its lamp plus a point light, 16 x 16: the triangle pdfs carry 1 - P_ana.  Batch means of light and mis agree
    within batch-to-batch standard errors (bsdf cannot find a delta light and is refused); rnds are pt_render's, rays the oracle's
    frame's (pt_render's parity target), as tests/test_gpu_env.py checks them."""
    W = H = 16
    batches, spp = 32, 64
    sc = api.Scene(W, H).load(cb_spec)
    sc.set_lights([box_light(api)], select=0.5)
    assert sc.debug_lights()["P_ana"] == 0.5
    sc.iterations = CB_BOUNCES
    rng = np.random.default_rng(11)
    per = {"light": [], "mis": []}
    for b in range(batches):
        for s in per:
            sc.upload_seeds(rng.integers(1, 2 ** 31 - 2, W * H).astype(np.int32))
            sc.current_sample = 0
            sc.render_nee(spp, s)
            per[s].append(sc.read_colors()[:, :3].reshape(H // 8, 8, W // 8, 8, 3).mean(axis=(1, 3)))
    m = {s: np.mean(v, axis=0) for s, v in per.items()}
    se = {s: np.std(v, axis=0, ddof=1) / np.sqrt(batches) for s, v in per.items()}
    z = np.abs(m["light"] - m["mis"]) / np.sqrt(se["light"] ** 2 + se["mis"] ** 2)
    print("light against mis: max |z| %.2f" % z.max())
    assert z.max() < 5.0
    plain = api.Scene(W, H).load(cb_spec)
    plain.iterations = CB_BOUNCES
    plain.render(3)
    fr = oracle.OracleFrame(W, H)
    fr.render(oracle.load_scene(cb_spec), oracle.make_camera(cb_spec.fov, cb_spec.yaw, cb_spec.pitch, cb_spec.shift, W, H), CB_BOUNCES, 0, 3, nthreads=16)
    assert np.array_equal(plain.read_rnds(), fr.rnds())
    for s in per:
        lit = api.Scene(W, H).load(cb_spec)
        lit.set_lights([box_light(api)])
        lit.iterations = CB_BOUNCES
        lit.render_nee(2, s)
        lit.render_nee(1, s)
        got = state(lit)
        assert np.array_equal(got[1], plain.read_rnds()), s
        assert same_bits(got[2], fr.rays()["P"][:, :3]) and same_bits(got[3], fr.rays()["D"][:, :3]), s
        assert not same_bits(got[0], plain.read_colors())


# ---------------------------------------------------------------------------- 5: other paths
def test_runs_repeat_and_the_flat_preview_is_unchanged(api, cb_spec):
    W, H = 48, 40
    runs = []
    for _ in range(2):
        sc = api.Scene(W, H).load(cb_spec)
        sc.set_lights([box_light(api), api.spot_light((800.0, 900.0, -200.0), (0, -1, 0), (5e6, 5e6, 5e6), 10, 25)], select=0.4)
        sc.iterations = CB_BOUNCES
        sc.render_nee(2, "mis")
        sc.render_nee(1, "mis")
        runs.append(state(sc))
    assert same_state(runs[0], runs[1])
    for strategy in ("light", "mis"):
        plain = api.Scene(W, H).load(cb_spec)
        plain.iterations = 1
        plain.render_nee(2, strategy)
        lit = api.Scene(W, H).load(cb_spec)
        lit.set_lights([box_light(api)])
        lit.iterations = 1
        lit.render_nee(2, strategy)
        assert same_state(state(lit), state(plain)), strategy


@pytest.mark.parametrize("sky", [False, True])
def test_adaptive_nee_tiles_hold_render_nee_bits(api, sky):
    """k_nee_tiles_lights / k_nee_env_tiles_lights against k_nee_lights / k_nee_env_lights at 36 x 20: ragged tiles on the right and at
    the bottom"""
    from opencl_path_tracer_amd import scenes
    W, H = 36, 20
    spec = scenes.cornell_box()

    def scene():
        c = api.Scene(W, H).load(spec)
        if sky:
            c.set_environment(scenes.sun_and_sky())
        c.set_lights([box_light(api)], select=0.4)
        c.iterations = CB_BOUNCES
        return c
    sc = scene()
    sc.render_adaptive(4, 16, 0.0, metric="half", path="nee", strategy="mis")
    thr = float(np.median(sc.tile_state()[1]))
    assert np.isfinite(thr) and thr > 0.0
    sc.current_sample = 0
    sc.seed_default()
    sc.render_adaptive(4, 16, thr, metric="half", path="nee", strategy="mis")
    counts = sc.sample_counts().reshape(-1)
    cols, rnds = sc.read_colors(), sc.read_rnds()
    seen = sorted(set(int(c) for c in np.unique(counts)))
    assert set(seen) <= {4, 8, 16} and len(seen) >= 2, seen
    for k in seen:
        fresh = scene()
        fresh.render_nee(k, "mis")
        sel = counts == k
        assert same_bits(cols[sel, :3], fresh.read_colors()[sel, :3]) and np.array_equal(rnds[sel], fresh.read_rnds()[sel]), k


def test_tiled_ranks_assemble_the_single_context_frame(api, cb_spec):
    W, H, world = 48, 36, 2
    lights = [box_light(api), api.directional_light((0.2, -1.0, 0.1), (0.5, 0.5, 0.5))]
    one = api.Scene(W, H).load(cb_spec)
    one.set_lights(lights)
    one.iterations = CB_BOUNCES
    one.render_nee(3, "mis")
    whole = state(one)
    seen = np.zeros(W * H, dtype=bool)
    for r in range(world):
        sc = api.Scene(W, H, rank=r, world=world, rows_per_block=8).load(cb_spec)
        sc.set_lights(lights)
        sc.iterations = CB_BOUNCES
        sc.render_nee(3, "mis")
        ids = sc.local_pixel_ids()
        assert same_state(state(sc), tuple(a[ids] for a in whole)), r
        seen[ids] = True
    assert seen.all()


def test_light_lit_frame_composes_with_variance_guides_denoise_and_temporal(api):
    from opencl_path_tracer_amd import scenes
    W, H = 48, 40
    sc = api.Scene(W, H).load(scenes.cornell_box(lamp="point"))
    assert sc.debug_lights()["P_ana"] == 1.0
    sc.set_option("moments", 1)
    sc.iterations = CB_BOUNCES
    sc.render_nee(8, "mis")
    cols = sc.read_colors()
    assert np.isfinite(cols).all() and cols[:, :3].mean() > 0.0
    var = sc.read_variance()
    assert np.isfinite(var).all() and (var >= 0).all()
    sc.render_aovs(1, 4)
    for dn in (sc.denoise(iterations=2), sc.denoise_variance(iterations=2)):
        assert np.isfinite(dn).all()
    assert np.isfinite(sc.temporal_accumulate()).all()
    assert np.isfinite(sc.denoise_temporal(iterations=2)).all()
    assert same_bits(sc.read_colors(), cols)
