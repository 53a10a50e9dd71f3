"""-m gpu: sphere lights and suns with an angular size in Scene.render_nee and Scene.render_adaptive(path="nee") (pt_set_area_lights, the
area-light instances of k_nee in pt_nee_arealights.hip; include/pt_api.h pins the set, the selection and the estimator).

  1 without a pickable area light render_nee and the adaptive NEE tiles compute the bits they computed before; 2 a sphere no ray can reach,
  with select = 0, renders the frame of the family that family 12 replaces, bit for bit; 3 all sixteen instances of family 12, the four node
  modes bit for bit; 4 the device's sample and hit functions against
  float64 on authored items; 6 closed forms on a diffuse floor under a sun and under a sphere, and an umbra that is exactly dark; 7 the
  camera sees a sphere light as L; 8 the three estimators agree on the mean of cornell_box(lamp="sphere"); 9 adaptive tiles, tiled ranks and
  repeated runs hold render_nee's bits, and the frame composes with variance, guides, denoise, temporal and despeckle.
  5 frames against the float64 model (tests/arealights_ref.AreaLightsModel) in the three strategies with and without a sky, with bounded
  fog, and under smooth_normals + glossy, and 7b a sphere seen in the box's mirror."""

import numpy as np
import pytest

import arealights_ref as A
import nee_instances as I
import nee_ref as R
import test_gpu_interior as TG
import test_gpu_nee_instances as TI

pytestmark = pytest.mark.gpu

CB_BOUNCES = 4
EYE_AT_ORIGIN = (-500.0, -500.0, 1299.0378)
# far below and behind the box: the box is open only towards +z, and the rare path that leaks through a seam of its walls would have to leave
# within 7e-4 rad of one direction to meet it (a sphere 4,000 behind the back wall was met by one such path in 2,560)
FAR_SPHERE = dict(center=(500.0, -1e5, -1e5), radius=100.0, radiance=(5.0, 5.0, 5.0))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def state(sc):
    rays = sc.read_rays()
    return sc.read_colors().copy(), sc.read_rnds().copy(), rays["P"][:, :3].copy(), rays["D"][:, :3].copy()


def same_state(a, b):
    return same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2]) and same_bits(a[3], b[3])


def lum(c):
    return c[:, :3].astype(np.float64) @ np.array([0.2126, 0.7152, 0.0722])


# ---------------------------------------------------------------------------- 1: no change without area lights
@pytest.mark.parametrize("adaptive", [False, True])
def test_no_area_lights_no_change(api, cb_spec, adaptive):
    W, H = 48, 40

    def frame(prepare):
        sc = api.Scene(W, H).load(cb_spec)
        prepare(sc)
        sc.iterations = CB_BOUNCES
        if adaptive:
            sc.render_adaptive(2, 4, 0.05, metric="half", path="nee", strategy="mis")
        else:
            sc.render_nee(3, "mis")
        return state(sc), sc.stat("nee_family")

    want, family = frame(lambda sc: None)

    def cleared(sc):
        sc.set_area_lights([api.sphere_light(**FAR_SPHERE)])
        sc.clear_area_lights()
    black = [api.sphere_light((500.0, 900.0, 0.0), 50.0, radiance=(0, 0, 0)), api.sun_light((0, -1, 0), 1.0, radiance=(0, 0, 0))]
    for prepare in (cleared, lambda sc: sc.set_area_lights(black)):
        got, fam = frame(prepare)
        assert same_state(got, want) and fam == family != 12
    lit, fam = frame(lambda sc: sc.set_area_lights([api.sphere_light((500.0, 800.0, 0.0), 50.0, radiance=(50.0, 50.0, 50.0))]))
    assert fam == 12 and not same_bits(lit[0], want[0])


# ---------------------------------------------------------------------------- 2: a set no ray can reach
UNREACHED_CASES = {     # cornell_box arguments, options, and what else is set: the family the frame launches without the area set
    "plain": (dict(), {}, None, 0),
    "smooth": (dict(smooth=True), {"smooth_normals": 1}, None, 1),
    "smooth_textures": (dict(smooth=True, textured=True), {"smooth_normals": 1, "textures": 1}, None, 2),
    "glossy": (dict(smooth=True, glossy=True), {"smooth_normals": 1, "glossy": 1}, None, 3),
    "coated": (dict(glossy=True, coated=True), {"glossy": 1, "coated": 1}, None, 4),
    "lens": (dict(glossy=True, coated=True), {"glossy": 1}, "lens", 5),
    "frosted": (dict(smooth=True, frosted=True), {"smooth_normals": 1, "frosted": 1}, None, 6),
    "lights": (dict(frosted=True), {}, "lights", 7),
    "fog": (dict(fog=1e-3), {}, None, 8),
    "fog_lights": (dict(fog=1e-3, lamp="spot"), {"glossy": 1}, None, 8),
    "grid": (dict(fog=2e-3), {}, "grid", 9),
    "interior": (dict(tint=(0.9, 0.6, 0.3), wax=2.0), {}, None, 10),
    "interior_fog": (dict(tint=(0.9, 0.6, 0.3), fog=1e-3, frosted=True), {"frosted": 1}, None, 10),
    "light_tree": (dict(), {"light_tree": 1}, None, 11),
    "light_tree_sky": (dict(wax=1.0), {"light_tree": 1}, "sky", 11),
}


@pytest.mark.parametrize("case", sorted(UNREACHED_CASES))
def test_an_unreachable_set_keeps_every_familys_bits(api, case):
    """A sphere far below and behind the box with select = 0: P_area = 0, every 1 - P_area is exactly 1, no segment meets the sphere, so the
    frame is, bit for bit, the one the family it replaces renders, while nee_family reads 12: what family 12 reads at run time (every flag up
    to the light tree's) is what those families read or have compiled in."""
    from opencl_path_tracer_amd import scenes
    W, H = 40, 32
    box, options, extra, family = UNREACHED_CASES[case]
    spec = scenes.cornell_box(**box)
    frames = []
    for area in (False, True):
        sc = api.Scene(W, H).load(spec)
        for k, v in options.items():
            sc.set_option(k, v)
        if extra == "lens":
            sc.set_lens(25.0, 1600.0)
        if extra == "lights":
            sc.set_lights([api.point_light((200.0, 800.0, 100.0), (4e6, 3e6, 2e6))], select=0.4)
        if extra == "grid":
            sc.set_medium_density(scenes.smoke_plume(8))
        if extra == "sky":
            sc.set_environment(scenes.sun_and_sky())
        if area:
            sc.set_area_lights([api.sphere_light(**FAR_SPHERE)], select=0.0)
            assert sc.debug_area_lights()["P_area"] == 0.0
        sc.iterations = CB_BOUNCES
        sc.render_nee(2, "mis")
        frames.append(state(sc))
        assert sc.stat("nee_family") == (12 if area else family), case
    assert same_state(frames[0], frames[1]), case
    assert np.isfinite(frames[0][0]).all() and frames[0][0][:, :3].mean() > 0.0


# ---------------------------------------------------------------------------- 3: the sixteen instances
def instance_lights(api):
    return [api.sphere_light((300.0, 700.0, 200.0), 80.0, radiance=(30.0, 25.0, 20.0)), api.sphere_light((800.0, 500.0, 400.0), 40.0, radiance=(5.0, 9.0, 12.0)),
            api.sun_light((0.2, -1.0, 0.3), 4.0, irradiance=2.0)]


@pytest.mark.parametrize("form", range(4), ids=I.FORMS)
def test_node_modes_render_the_same_bits(api, form):
    """tests/test_gpu_nee_instances.py's equalities for the sixteen new instances: its scenes with every feature, the fog, a waxy interior
    and the light tree live, and two sphere lights and a sun inside: small scene, mode 0 = 1 = 3 = 3 with the stack overflowing; mesh, mode
    1 = 2 = 3; each launch is identified by node_mode, nee_family, nee_form and nee_block, and the lights change the frame."""
    for scene, first in (("small", "lds"), ("mesh", "treelet")):
        frames, thr = {}, None
        for placement in list(I.PLACEMENTS[scene]) + ["dark"]:
            sc, mode = I.build(api, scene, "medium", first if placement == "dark" else placement, sky=bool(form & 1))
            TG.bind(sc, I.scene_spec(scene, True, True), **TG.WAX)
            sc.set_option("light_tree", 1)
            if placement != "dark":
                sc.set_area_lights(instance_lights(api), select=0.4)
            if form & 2 and thr is None:
                sc.iterations = TI.TL.CB_BOUNCES
                thr = TI.threshold_of(sc)
            frames[placement] = TI.render(sc, form, thr)
            got = tuple(int(sc.stat(k)) for k in ("node_mode", "nee_family", "nee_form", "nee_block"))
            assert got == (mode, 11 if placement == "dark" else 12, form, TG.block_of(form, mode)), (scene, placement, got)
            sc.close()
        want, dark = frames[first], frames.pop("dark")
        assert np.isfinite(want[0]).all() and want[0][:, :3].mean() > 0.0
        assert not same_bits(want[0], dark[0])
        for placement, got in frames.items():
            assert TI.same_frames(got, want), (I.FORMS[form], scene, placement)


# ---------------------------------------------------------------------------- 4: the device's sample and hit functions
SUN_SMALL, SUN_WIDE = 0.00465, 0.5
U_LAST = 1.0 - 2.0 ** -24


def eval_items(api):
    """the set (two spheres in line along +z, two to pass at 1.01 R and 0.99 R, one around an origin; two suns) and the authored items"""
    lights = [api.sphere_light((0.0, 0.0, 10.0), 1.0, radiance=1.0), api.sphere_light((0.0, 0.0, 20.0), 2.0, radiance=1.0),
              api.sphere_light((30.0, 1.01, 10.0), 1.0, radiance=1.0), api.sphere_light((60.0, 0.99, 10.0), 1.0, radiance=1.0),
              api.sphere_light((0.0, 100.0, 0.0), 5.0, radiance=1.0),
              api.sun_light((0.0, -1.0, 0.0), np.degrees(2 * SUN_SMALL), radiance=1.0), api.sun_light((-0.3, -0.8, -0.5), np.degrees(2 * SUN_WIDE), radiance=1.0)]
    us = [(0.0, 0.0), (U_LAST, U_LAST), (0.5, 0.25), (U_LAST, 0.0), (0.3, U_LAST)]
    samples = []
    for u in us:
        samples += [((0.0, 0.0, 10.0 - (1 + 1e-3)), 0, u),          # d = R (1 + 1e-3)
                    ((0.0, 0.0, 10.0 - 1e4), 0, u),                 # R / d = 1e-4
                    ((0.2, 100.5, -0.1), 4, u),                     # inside: rejected
                    ((3.0, -2.0, 1.0), 1, u), ((1.0, 2.0, 3.0), 5, u), ((1.0, 2.0, 3.0), 6, u)]
    z = (0.0, 0.0, 1.0)
    rays = [((0.0, 0.0, 0.0), z, np.inf),                           # two in line: the nearer one
            ((0.0, 0.0, 12.0), z, np.inf),                          # from between them: the farther one
            ((0.0, 0.0, 10.5), z, np.inf),                          # from inside the nearer one: it is transparent
            ((30.0, 0.0, 0.0), z, np.inf), ((60.0, 0.0, 0.0), z, np.inf),       # passes at 1.01 R (a miss) and at 0.99 R (a hit)
            ((0.0, 0.0, 0.0), z, 9.0 * (1 - 1e-3)), ((0.0, 0.0, 0.0), z, 9.0 * (1 + 1e-3)),      # t_max just short of the sphere and just past it
            ((0.0, 100.0, 0.0), (0.0, 1.0, 0.0), np.inf)]           # from a sphere's centre along the small sun's axis
    for a, axis in ((SUN_SMALL, np.array([0.0, 1.0, 0.0])), (SUN_WIDE, np.array([0.3, 0.8, 0.5]) / np.linalg.norm([0.3, 0.8, 0.5]))):
        side = np.cross(axis, [1.0, 0.0, 0.0])
        side /= np.linalg.norm(side)
        for f in (0.98, 1.02):                                      # both sides of the rim
            d = axis * np.cos(a * f) + side * np.sin(a * f)
            rays.append(((5.0, -50.0, 5.0), tuple(d), np.inf))
    return lights, samples, rays


def eval_reference(table, samples, rays, f):
    rec, ns = table["records"].astype(np.float64), int((table["records"][:, 8] == 0).sum())
    spheres = [(rec[j, :3], rec[j, 3]) for j in range(ns)]
    suns = [(rec[j, :3], rec[j, 3]) for j in range(ns, len(rec))]
    s_out, h_out = [], []
    for o, j, (u1, u2) in samples:
        o32 = np.asarray(o, dtype=np.float32).astype(f)
        r = A.sphere_sample(rec[j, :3], rec[j, 3], o32, u1, u2, f) if j < ns else A.sun_sample(rec[j, :3], rec[j, 8], u1, u2, f)
        s_out.append(r)
    for o, d, tmax in rays:
        o32, d32 = np.asarray(o, dtype=np.float32).astype(f), np.asarray(d, dtype=np.float32).astype(f)
        j, t, m1 = A.sphere_hit(spheres, o32, d32, np.float32(tmax), f)
        mask, m2 = A.sun_mask(suns, d32, f)
        h_out.append((j, t, mask, m1, m2))
    return s_out, h_out


def eval_errors(got_s, got_h, want_s, want_h):
    """per quantity, the worst error of (w, p_omega, t_s) tuples / (sphere, t, ...) tuples against the float64 ones: w absolute (unit
    vectors), p_omega, t_s and the hit's t relative"""
    worst = dict(w=0.0, p_omega=0.0, t_s=0.0, t=0.0)
    for g, w in zip(got_s, want_s):
        if w is None:
            continue
        worst["w"] = max(worst["w"], float(np.abs(np.asarray(g[0], np.float64) - w[0]).max()))
        worst["p_omega"] = max(worst["p_omega"], abs(float(g[1]) - w[1]) / w[1])
        if np.isfinite(w[2]):
            worst["t_s"] = max(worst["t_s"], abs(float(g[2]) - w[2]) / w[2])
    for g, w in zip(got_h, want_h):
        if w[0] >= 0:
            worst["t"] = max(worst["t"], abs(float(g[1]) - w[1]) / w[1])
    return worst


def eval_spread(api):
    """per quantity, the worst |float32 - float64| of the restatement over the items: no GPU"""
    lights, samples, rays = eval_items(api)
    table = A.table(lights)
    s64, h64 = eval_reference(table, samples, rays, np.float64)
    s32, h32 = eval_reference(table, samples, rays, np.float32)
    for a, b in zip(s64, s32):
        assert (a is None) == (b is None)
    for a, b in zip(h64, h32):
        assert a[0] == b[0] and a[2] == b[2]
    return eval_errors(s32, h32, s64, h64)


# the rounding spread of the float32 restatement against float64 over the items (eval_spread, measured on the CPU), and the tolerance: 4 x
# for fma contraction and the device's divide and sqrt paths (profiles/arealights/README.md).  EVAL_RTOL is the issue's one tolerance, from
# the worst spread of all: the cut t_s of the sphere seen at R / d = 1e-4 and at the rim, where b - sqrt(b^2 - (d^2 - R^2)) cancels in
# float32.  Each quantity is also held to 4 x its own spread, which is what makes the test bite for w and p_omega
EVAL_SPREADS = dict(w=1.01e-4, p_omega=4.6e-7, t_s=1.13e-3, t=9.5e-7)
EVAL_FLOAT32_SPREAD = max(EVAL_SPREADS.values())
EVAL_RTOL = 4 * EVAL_FLOAT32_SPREAD


def test_debug_area_light_eval_against_float64(api):
    lights, samples, rays = eval_items(api)
    sc = api.Scene(8, 8)
    sc.set_area_lights(lights)
    table = sc.debug_area_lights()
    assert table["n_sphere"] == 5 and np.array_equal(table["order"], np.arange(7))
    spread = eval_spread(api)
    print("float32 spreads over the items %s (pinned %s)" % (spread, EVAL_SPREADS))
    assert all(spread[k] <= EVAL_SPREADS[k] for k in spread)
    want_s, want_h = eval_reference(A.table(lights), samples, rays, np.float64)
    got_s, got_h = sc.debug_area_light_eval(origins=[s[0] for s in samples], lights=[s[1] for s in samples], u=[s[2] for s in samples],
                                            rays=[tuple(r[0]) + tuple(r[1]) + (r[2],) for r in rays])
    for g, w in zip(got_s, want_s):
        assert bool(g["accept"]) == (w is not None)
        if w is None:
            assert g["p_omega"] == 0.0 and np.isinf(g["t_s"])
        elif not np.isfinite(w[2]):
            assert np.isinf(g["t_s"])
    assert sum(w is None for w in want_s) == 5
    for g, (j, t, mask, m1, m2) in zip(got_h, want_h):
        # no decision within 1e-4 relative of its other outcome (a sun's rim: of 1 - cos a, the disc's own scale)
        assert all(min(m) > 1e-4 for m in m1) and min(m2) > 1e-4 * (1.0 - np.cos(SUN_SMALL))
        assert int(g["sphere"]) == j and int(g["suns"][0]) == mask and int(g["suns"][1]) == 0
    assert [h[0] for h in want_h[:8]] == [0, 1, 1, -1, 3, -1, 0, -1]
    assert [h[2] for h in want_h[7:]] == [1, 1, 0, 2, 0]
    errors = eval_errors([(g["w"], g["p_omega"], g["t_s"]) for g in got_s], [(int(g["sphere"]), g["t"]) for g in got_h], want_s, want_h)
    print("device against float64: worst errors %s" % errors)
    assert max(errors.values()) <= EVAL_RTOL
    for k, e in errors.items():
        assert e <= 4 * EVAL_SPREADS[k], (k, e)


# ---------------------------------------------------------------------------- 5: frames against the float64 model
import test_gpu_lights as TL          # noqa: E402

REPLAY = dict(TL.REPLAY, area_select=0.5)


def replay_area_lights(api):
    """a sphere light above the occluder, one half under its edge, and a sun through the open top"""
    return [api.sphere_light((0.0, 2.5, 6.0), 0.6, radiance=(20.0, 18.0, 15.0)), api.sphere_light((1.0, -0.3, 6.0), 0.7, radiance=(6.0, 8.0, 10.0)),
            api.sun_light((0.3, -1.0, 0.2), 40.0, irradiance=(1.5, 1.4, 1.2))]


MIRROR_SPHERE = dict(center=(4.0, -0.5, 10.5), radius=0.5, radiance=(7.0, 5.0, 3.0))     # its image in the mirror at x = 4.95 is in view


FOG = dict(sigma_t=0.08, albedo=(0.9, 0.7, 0.5), g=0.6, bounds=((-4.5, -2.5, 0.5), (4.5, 4.5, 11.5)))      # test_gpu_medium.py's: both spheres are inside


def replay_scene(api, sky, lights=None, device=0, fog=False):
    spec, rgb = TL.replay_spec(), TL.replay_map()
    sc = api.Scene(REPLAY["W"], REPLAY["H"], device=device).load(spec)
    if fog:
        sc.set_medium(**FOG)
    if sky:
        sc.set_environment(rgb, scale=REPLAY["scale"], yaw_degrees=REPLAY["yaw_degrees"], select=REPLAY["select"])
    sc.set_area_lights(replay_area_lights(api) if lights is None else lights, select=REPLAY["area_select"])
    return sc, spec, rgb


def replay_model(api, sc, spec, rgb, sky):
    verts, mo = spec.objects[0]
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    env = dict(rgb=rgb, tables=sc.debug_environment(), scale=REPLAY["scale"], yaw_degrees=REPLAY["yaw_degrees"]) if sky else None
    return A.AreaLightsModel(verts, recs["N"], mats, mo, sc.camera[0], sc.debug_lights(), sc.debug_area_lights(), medium=sc.medium(), env=env,
                             table=sc.debug_light_table())


def glossy_replay_scene(api, device=0):
    """test_gpu_lights.py's glossy replay scene (a closed box with a type-4 floor and spheres with vertex normals) under smooth_normals +
    glossy, lit by its lamp and emitter and by the replay's area set in place of the delta lights (the sun stays outside the ceiling)"""
    spec = TL.glossy_replay_spec()
    sc = api.Scene(REPLAY["W"], REPLAY["H"], device=device).load(spec)
    sc.set_option("smooth_normals", 1)
    sc.set_option("glossy", 1)
    sc.set_area_lights(replay_area_lights(api), select=REPLAY["area_select"])
    return sc, spec


def glossy_replay_model(api, sc, spec):
    verts = np.concatenate([v for v, _ in spec.objects])
    mo = np.concatenate([m for _, m in spec.objects])
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    vn = np.concatenate([np.zeros(v.shape, dtype=np.float32) if n is None else n for (v, _), n in zip(spec.objects, spec.normals)])
    return A.AreaLightsModel(verts, recs["N"], mats, mo, sc.camera[0], sc.debug_lights(), sc.debug_area_lights(), vnormals=vn, table=sc.debug_light_table())


def compare_with_model(sc, want, want_seeds, ties, sel=None):
    got = sc.read_colors()[:, :3].astype(np.float64)
    keep = ~ties if sel is None else (~ties & sel)
    print("near-tie pixels: %d of %d" % (int(ties.sum()), ties.size))
    assert (~ties).mean() > 0.9, "too many near-tie pixels: %d" % int(ties.sum())
    assert np.array_equal(sc.read_rnds()[keep], want_seeds[keep])
    scale = float(want[~ties].max())
    err = np.abs(got[keep] - want[keep])
    worst = float((err / (np.abs(want[keep]) + 1e-6 * scale)).max())
    print("worst relative error %g" % worst)
    bad = err > 2e-3 * np.abs(want[keep]) + 1e-6 * scale
    assert not bad.any(), "%d of %d pixel channels differ; worst %g" % (int(bad.sum()), bad.size, worst)
    return got


@pytest.mark.parametrize("sky", [True, False])
@pytest.mark.parametrize("strategy", ["bsdf", "light", "mis"])
def test_matches_float64_model(api, strategy, sky):
    """test_gpu_lights.py's replay box with two sphere lights and a sun, against tests/arealights_ref.AreaLightsModel: rnds equal and
    colours within 2e-3 |want| + 1e-6 scale on the kept pixels, at least 90 % kept.  The model alone, on these seeds, flags 0.98 % (no sky) / 1.04 %
    (sky) of the pixels as near-ties under mis (measured on a host-only context before the first GPU run, tests/test_arealights_host.py):
    far below the 10 % cap."""
    spp, bounces = REPLAY["spp"], REPLAY["bounces"]
    sc, spec, rgb = replay_scene(api, sky)
    seeds = TL.replay_seeds()
    sc.upload_seeds(seeds)
    sc.iterations = bounces
    sc.render_nee(spp, strategy)
    assert sc.stat("nee_family") == 12
    model = replay_model(api, sc, spec, rgb, sky)
    assert model.par == 0.5 and len(model.spheres) == 2 and len(model.suns) == 1 and model.pa == 0.0
    want, want_seeds, ties = model.render(seeds, bounces, spp, api.NEE_STRATEGIES[strategy])
    compare_with_model(sc, want, want_seeds, ties)
    assert float(want[~ties].mean()) > 0.0


@pytest.mark.parametrize("strategy", ["bsdf", "light", "mis"])
def test_matches_float64_model_in_bounded_fog(api, strategy):
    """The same replay, under the sky, in test_gpu_medium.py's bounded fog, which holds both spheres: the free flight is drawn against the
    segment cut at a sphere, a segment that scatters first does not end on it, a scatter vertex samples the set without a cosine, and every
    sample carries its transmittance up to t_s.  The model alone flags 1.11 % of the pixels as near-ties under mis (host-only, before
    the first GPU run); the events below are what only this run reaches."""
    spp, bounces = REPLAY["spp"], REPLAY["bounces"]
    sc, spec, rgb = replay_scene(api, True, fog=True)
    seeds = TL.replay_seeds()
    sc.upload_seeds(seeds)
    sc.iterations = bounces
    sc.render_nee(spp, strategy)
    assert sc.stat("nee_family") == 12
    model = replay_model(api, sc, spec, rgb, True)
    assert model.medium is not None and model.par == 0.5
    want, want_seeds, ties = model.render(seeds, bounces, spp, api.NEE_STRATEGIES[strategy])
    keep = ~ties
    print("events in the kept pixels: %s" % {k: int(v[keep].sum()) for k, v in model.pixel_events.items() if v[keep].sum()})
    for name in ("scatter", "sphere_end", "sphere_end_scatter") + (() if strategy == "bsdf" else ("scatter_light", "area_sample")):
        assert int(model.pixel_events[name][keep].sum()) > 0, name
    compare_with_model(sc, want, want_seeds, ties)


def test_matches_float64_model_under_smooth_normals_and_glossy(api):
    """Options smooth_normals + glossy on the glossy replay scene, strategy mis: W_b of a sphere met after a rough vertex comes from the
    GGX p_b, an area sample at a rough vertex is weighted with it, and one on the wrong geometric side of a shading normal is refused.
    The model alone flags 1.76 % of the pixels as near-ties (host-only, before the first GPU run)."""
    spp, bounces = REPLAY["spp"], REPLAY["bounces"]
    sc, spec = glossy_replay_scene(api)
    seeds = TL.replay_seeds()
    sc.upload_seeds(seeds)
    sc.iterations = bounces
    sc.render_nee(spp, "mis")
    assert sc.stat("nee_family") == 12
    model = glossy_replay_model(api, sc, spec)
    assert model.par == 0.5 and len(model.lights) == 3 and len(model.spheres) == 2
    want, want_seeds, ties = model.render(seeds, bounces, spp, 2)
    keep = ~ties
    print("events in the kept pixels: %s" % {k: int(v[keep].sum()) for k, v in model.pixel_events.items() if v[keep].sum()})
    for name in ("sphere_end_rough", "area_glossy", "area_ng_reject", "glossy_vertex", "sphere_blocks"):
        assert int(model.pixel_events[name][keep].sum()) > 0, name
    compare_with_model(sc, want, want_seeds, ties)


def test_a_sphere_seen_in_the_mirror(api):
    """iterations = 2, strategy bsdf, no sky: a pixel whose camera ray meets the box's mirror and, reflected, the sphere shows
    L (fL + fB) fS = 2 L F, F the mirror's Fresnel factor as the model computes it"""
    sc, spec, rgb = replay_scene(api, False, lights=[api.sphere_light(**MIRROR_SPHERE)])
    seeds = TL.replay_seeds()
    sc.upload_seeds(seeds)
    sc.iterations = 2
    sc.render_nee(1, "bsdf")
    model = replay_model(api, sc, spec, rgb, False)
    want, want_seeds, ties = model.render(seeds, 2, 1, 0)
    mirror = np.zeros(len(seeds), dtype=bool)
    for i in range(len(seeds)):
        s_, r1 = R.lcg(int(seeds[i]))
        s_, r2 = R.lcg(s_)
        ti = model.intersect(*model.camera_ray(i, r1, r2))[0]
        mirror[i] = ti >= 0 and int(model._mat(ti)["type"]) == 1
    seen = mirror & ~ties & (want.sum(axis=1) > 0)
    print("%d mirror pixels, %d of them show the sphere" % (int(mirror.sum()), int(seen.sum())))
    assert seen.sum() >= 3
    Lr = np.array(MIRROR_SPHERE["radiance"])
    assert (want[seen] > 0.5 * Lr).all() and (want[seen] < 2.0 * Lr).all()          # 2 L F with F of chromium between 0.25 and 1
    compare_with_model(sc, want, want_seeds, ties, sel=seen)


# ---------------------------------------------------------------------------- 6: closed forms on a diffuse floor
FLOOR_Y, KD = -10.0, 0.5
CF_W, CF_H = 48, 36
CF_RTOL = 4 * 7.2e-8             # test_gpu_lights.py's CF_RTOL["down"]: four times the float32 rounding of the directional chain


def floor_spec(extra=()):
    from opencl_path_tracer_amd import scenes
    big = 1e4
    mats = [((KD, KD, KD), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0), ((0, 0, 0), (0, 0, 0), (30.0, 30.0, 30.0), (0, 0, 0), (0, 0, 0), 0.0, 3)]
    tris = [((-big, FLOOR_Y, -big), (big, FLOOR_Y, big), (big, FLOOR_Y, -big)), ((-big, FLOOR_Y, -big), (-big, FLOOR_Y, big), (big, FLOOR_Y, big))]
    mo = [0, 0]
    for t, m in extra:
        tris.append(t)
        mo.append(m)
    spec = scenes.SceneSpec(materials=mats, fov=60.0, shift=EYE_AT_ORIGIN, name="floor")
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.asarray(mo, dtype=np.uint16)))
    return spec


def floor_rows():
    return np.arange(CF_W * CF_H) // CF_W


def test_a_small_sun_at_the_zenith_is_the_directional_light(api):
    """iterations = 2, strategy light, one sample, P_area = 1: a floor pixel is exactly its one light sample, kd cos L (cos / pi) / p_omega =
    2 kd L q cos^2 with cos = 1 - u1 q of the pixel's own u1 = pt_nee_rand(S, 0, 1) (N is the sun's axis, so N.w is the cone's cosine): each
    pixel is held to that value within CF_RTOL of test_gpu_lights.py.  The integrand is flat: over the disc of a = 0.00465 it moves by
    1 - cos^2 a = 2.2e-5, its mean is 2 kd L (1 - cos^3 a) / 3 -- checked on the expectation in float64 -- and the frame is the
    directional light's kd E / pi to O(a^2)."""
    E = np.array([3.0, 2.0, 1.0])
    a = SUN_SMALL
    sc = api.Scene(CF_W, CF_H).load(floor_spec())
    sun = api.sun_light((0.0, -1.0, 0.0), np.degrees(2 * a), irradiance=E)
    sc.set_area_lights([sun])
    table = sc.debug_area_lights()
    assert table["P_area"] == 1.0
    seeds = np.random.default_rng(41).integers(1, 2 ** 31 - 2, CF_W * CF_H).astype(np.int32)
    sc.upload_seeds(seeds)
    sc.iterations = 2
    sc.render_nee(1, "light")
    got = sc.read_colors()[:, :3].astype(np.float64)
    floor = got.any(axis=1)
    assert floor[floor_rows() < CF_H // 2 - 1].all() and floor.sum() > CF_W * CF_H // 3
    L = table["records"][0, 4:7].astype(np.float64)
    q = float(table["records"][0, 8])
    u1 = ((np.asarray(R.nee_rand(seeds, 0, 1)).astype(np.int64) >> 8).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float64)
    c = 1.0 - u1 * q
    want = 2.0 * KD * q * (c * c)[:, None] * L[None, :]
    rel = np.abs(got[floor] - want[floor]) / want[floor]
    print("sun: %d floor pixels, worst relative error against 2 kd L q cos^2: %.3g (tolerance %.3g)" % (int(floor.sum()), rel.max(), CF_RTOL))
    assert rel.max() <= CF_RTOL
    mean = 2.0 * KD * L * (1.0 - np.cos(a) ** 3) / 3.0                 # the closed form is the expectation over u1: int_0^1 2 q (1 - u q)^2 du
    uu = (np.arange(4096) + 0.5) / 4096
    assert np.allclose(2.0 * KD * q * ((1.0 - uu * q) ** 2).mean() * L, mean, rtol=1e-6)      # (q is a float32 of 1 - cos a)
    assert np.abs(want[floor] / mean - 1.0).max() <= 1.0 - np.cos(a) ** 2
    flat = api.Scene(CF_W, CF_H).load(floor_spec())
    flat.set_lights([api.directional_light((0.0, -1.0, 0.0), E)])
    flat.upload_seeds(seeds)
    flat.iterations = 2
    flat.render_nee(1, "light")
    ref = flat.read_colors()[:, :3].astype(np.float64)
    assert np.array_equal(ref.any(axis=1), floor)
    assert np.abs(got[floor] / ref[floor] - 1.0).max() <= 2 * a * a


def test_under_a_sphere_light_the_floor_shows_the_closed_form(api):
    """Straight under a sphere light (sin t_m = R / d) a floor point shows 2 kd L (1 - cos^3 t_m) / 3.  A 48 x 36 frame has no column of
    pixels straight under a lamp, so the lamp is so large and far (R = 4e5 at height 1e6) that every floor pixel compared, at most 130 from
    its foot, is straight under it to (130 / 1e6)^2 = 1.7e-8 of the value, far inside the 5 standard errors of option moments that the mean
    over those pixels is held to, and those are below 1 % of the value.  Measured: 672 pixels at 64 spp: mean 0.153359 against
    0.153418, 5 sigma = 1.86e-4 (0.12 % of the value)."""
    R_, h, Lr = 4e5, 1e6, 2.0
    sc = api.Scene(CF_W, CF_H).load(floor_spec())
    sc.set_option("moments", 1)
    sc.set_area_lights([api.sphere_light((0.0, FLOOR_Y + h, 60.0), R_, radiance=Lr)])
    sc.iterations = 2
    spp = 64
    sc.render_nee(spp, "light")
    got = sc.read_colors()[:, 0].astype(np.float64)
    var = sc.read_variance().astype(np.float64).reshape(-1)
    sel = (floor_rows() < CF_H // 2 - 4) & (got > 0)
    assert sel.sum() > 300
    cm = np.sqrt(1.0 - (R_ / h) ** 2)
    want = 2.0 * KD * Lr * (1.0 - cm ** 3) / 3.0
    mean, se = got[sel].mean(), np.sqrt(var[sel].sum()) / sel.sum()
    print("sphere: %d pixels, %d spp: mean %.6g, closed form %.6g, 5 sigma = %.3g (%.2f %% of the value)" % (int(sel.sum()), spp, mean, want, 5 * se, 500 * se / want))
    assert 5 * se < 0.01 * want
    assert abs(mean - want) <= 5 * se


def test_the_umbra_of_a_sphere_light_is_dark(api):
    """A black sphere light between a small lamp quad and the floor is opaque to the quad's light samples.  An all-black set launches
    nothing, so a second, lit sphere sits under the floor, where no ray meets it, and select = 0 keeps every light sample on the quad: in
    strategy light the pixels in the blocker's umbra read exactly 0, and pixels outside its shadow keep their bits."""
    lamp = [(((-0.5, 20.0, 39.5), (0.5, 20.0, 39.5), (0.5, 20.0, 40.5)), 1), (((-0.5, 20.0, 39.5), (0.5, 20.0, 40.5), (-0.5, 20.0, 40.5)), 1)]
    frames = []
    for blocker in (False, True):
        sc = api.Scene(CF_W, CF_H).load(floor_spec(lamp))
        if blocker:
            sc.set_area_lights([api.sphere_light((0.0, 5.0, 40.0), 6.0, radiance=0.0), api.sphere_light((0.0, -500.0, 40.0), 10.0, radiance=5.0)], select=0.0)
            assert sc.debug_area_lights()["P_light"][0] == 0.0
        sc.iterations = 2
        sc.render_nee(2, "light")
        assert sc.stat("nee_family") == (12 if blocker else 0)
        frames.append(sc.read_colors()[:, :3].astype(np.float64))
    lit, shadowed = frames
    # the umbra on the floor: the shadow of a 6-unit sphere 15 above it, lit from 30 above by a 1-unit lamp, has radius > 8 around (0, 40)
    sc = api.Scene(CF_W, CF_H).load(floor_spec())
    cam = sc.camera[0]
    X, Y = int(cam["XM"]), int(cam["YM"])
    gid = np.arange(CF_W * CF_H)
    x, y = (gid % X) + 0.5, (gid // X) + 0.5
    pp = cam["lookat"][:3] + np.outer(2 * x / X - 1, cam["right"][:3]) + np.outer(2 * y / Y - 1, cam["up"][:3])
    d = pp - cam["eye"][:3]
    t = (FLOOR_Y - cam["eye"][1]) / np.where(d[:, 1] < 0, d[:, 1], np.nan)
    hit = cam["eye"][:3] + d * t[:, None]
    rho = np.hypot(hit[:, 0], hit[:, 2] - 40.0)
    # (the shadow's outer edge is at 13.8; a pixel's footprint on the floor is up to 9 long at these distances, and the samples jitter in it)
    umbra, outside = rho < 6.0, (rho > 25.0) & (rho < 60.0)
    assert umbra.sum() >= 4 and outside.sum() > 30
    assert lit[umbra].min() > 1e-3 and not shadowed[umbra].any()
    assert same_bits(lit[outside], shadowed[outside]) and lit[outside].any(axis=1).all()


# ---------------------------------------------------------------------------- 7: the camera sees the light
@pytest.mark.parametrize("iterations", [1, 8])
def test_the_camera_sees_a_sphere_light(api, iterations):
    L = (7.0, 5.0, 3.0)
    sc = api.Scene(CF_W, CF_H).load(floor_spec())
    cam = sc.camera[0]
    ahead = cam["lookat"][:3] - cam["eye"][:3]
    centre = cam["eye"][:3] + ahead / np.linalg.norm(ahead) * 50.0
    sc.set_area_lights([api.sphere_light(tuple(centre), 5.0, radiance=L)])
    sc.iterations = iterations
    for strategy in ("bsdf", "mis"):
        sc.current_sample = 0
        sc.seed_default()
        sc.render_nee(3, strategy)
        got = sc.read_colors().reshape(CF_H, CF_W, 4)
        for px in ((CF_H // 2, CF_W // 2), (CF_H // 2 - 1, CF_W // 2 - 1)):       # the four pixels around the frame's centre look at the sphere
            assert tuple(got[px][:3]) == tuple(np.float32(L)), (strategy, px)


# ---------------------------------------------------------------------------- 8: three estimators, one mean
def test_three_estimators_one_mean(api):
    from opencl_path_tracer_amd import scenes
    W, H, spp = 24, 16, 96
    spec = scenes.cornell_box(lamp="sphere")
    means, ses, var = {}, {}, {}
    for strategy in ("bsdf", "light", "mis"):
        sc = api.Scene(W, H).load(spec)
        sc.set_option("moments", 1)
        sc.iterations = CB_BOUNCES
        sc.render_nee(spp, strategy)
        assert sc.stat("nee_family") == 12
        y = lum(sc.read_colors())
        v = sc.read_variance().astype(np.float64).reshape(-1)
        assert np.isfinite(y).all() and np.isfinite(v).all()
        means[strategy], ses[strategy], var[strategy] = y.mean(), np.sqrt(v.sum()) / v.size, v.mean()
    print("frame means %s, standard errors %s, mean per-pixel variance %s" % (means, ses, var))
    for a, b in (("bsdf", "light"), ("bsdf", "mis"), ("light", "mis")):
        assert abs(means[a] - means[b]) <= 5 * np.hypot(ses[a], ses[b]), (a, b)
    assert means["mis"] > 0.0


# ---------------------------------------------------------------------------- 9: composition
def sphere_box(api, W, H, **kw):
    from opencl_path_tracer_amd import scenes
    sc = api.Scene(W, H, **kw).load(scenes.cornell_box())
    sc.set_area_lights([api.sphere_light((300.0, 700.0, 200.0), 80.0, radiance=(30.0, 25.0, 20.0)), api.sun_light((0.2, -1.0, 0.3), 4.0, irradiance=2.0)],
                       select=0.4)
    sc.iterations = CB_BOUNCES
    return sc


def test_runs_repeat_and_tiled_ranks_assemble_the_frame(api):
    W, H, world = 48, 32, 2
    one = sphere_box(api, W, H)
    one.render_nee(3, "mis")
    whole = state(one)
    again = sphere_box(api, W, H)
    again.render_nee(3, "mis")
    assert same_state(state(again), whole)
    seen = np.zeros(W * H, dtype=bool)
    for r in range(world):
        sc = sphere_box(api, W, H, rank=r, world=world, rows_per_block=8)
        sc.render_nee(3, "mis")
        ids = sc.local_pixel_ids()
        assert same_state(state(sc), tuple(a[ids] for a in whole)), r
        seen[ids] = True
    assert seen.all()


def test_adaptive_nee_tiles_hold_render_nee_bits(api):
    W, H = 36, 20
    sc = sphere_box(api, W, H)
    sc.render_adaptive(4, 16, 0.0, metric="half", path="nee", strategy="mis")
    thr = float(np.median(sc.tile_state()[1]))
    sc.current_sample = 0
    sc.seed_default()
    sc.render_adaptive(4, 16, thr, metric="half", path="nee", strategy="mis")
    assert sc.stat("nee_family") == 12 and int(sc.stat("nee_form")) & 2
    counts = sc.sample_counts().reshape(-1)
    cols, rnds = sc.read_colors(), sc.read_rnds()
    seen = sorted(set(int(c) for c in np.unique(counts)))
    assert set(seen) <= {4, 8, 16} and len(seen) >= 2, seen
    for k in seen:
        fresh = sphere_box(api, W, H)
        fresh.render_nee(k, "mis")
        sel = counts == k
        assert same_bits(cols[sel, :3], fresh.read_colors()[sel, :3]) and np.array_equal(rnds[sel], fresh.read_rnds()[sel]), k


def test_an_area_lit_frame_composes_with_variance_guides_denoise_temporal_and_despeckle(api):
    """The stages run on a frame lit by an area set and leave it as it was; the guides keep the view without the lights (the known limit
    include/pt_api.h records): they equal, bit for bit, those of the same scene with no set."""
    from opencl_path_tracer_amd import scenes
    W, H = 48, 40
    sc = sphere_box(api, W, H)
    sc.set_option("moments", 1)
    sc.render_nee(8, "mis")
    assert sc.stat("nee_family") == 12
    cols = sc.read_colors()
    assert np.isfinite(cols).all() and cols[:, :3].mean() > 0.0
    var = sc.read_variance()
    assert np.isfinite(var).all() and (var >= 0).all()
    bare = api.Scene(W, H).load(scenes.cornell_box())
    for shading in ("geometric", "shaded"):
        sc.render_aovs(1, 4, shading=shading)
        bare.render_aovs(1, 4, shading=shading)
        for a, b in zip(sc.read_aovs(), bare.read_aovs()):
            assert same_bits(a, b), shading
    for dn in (sc.denoise(iterations=2), sc.denoise_variance(iterations=2)):
        assert np.isfinite(dn).all()
    assert np.isfinite(sc.temporal_accumulate()).all()
    assert np.isfinite(sc.denoise_temporal(iterations=2)).all()
    rgbv, flags = sc.despeckle()
    assert np.isfinite(rgbv).all()
    assert np.isfinite(sc.denoise_despeckled(iterations=2)).all()
    assert same_bits(sc.read_colors(), cols)
