"""-m gpu: the lit guide buffers (option aov_lights: pt_render_aovs and pt_render_aovs_ex see the sphere lights and the suns of the area
set; include/pt_api.h pins them, the kernels are k_aovs<.., AovLights> in pt_denoise.hip).

  1 primary rays, device against device, bit for bit: the camera ray of every pixel and the unlit guides' depth through
    pt_debug_area_light_eval (the function the kernel calls) give the sphere, its distance and the suns' mask the lit guides must show;
    everywhere else the lit guides are the unlit guides;
  2 chains (a sphere light in a mirror, through a glass slab, a sun in a mirror, a sphere in front of a mirror) against the float64 replay
    of tests/aov_lights_ref.py, geometric and shaded, subpixels 1 and 2;
  3 option off, no set, a black set, a cleared set: the guides of a context that never heard of the option, bit for bit; stat aov_lights;
  4 staleness: pt_set_area_lights / pt_clear_area_lights make lit guides stale and leave unlit ones alone; the option invalidates nothing;
  5 consumers: both filters and the temporal pass against their models fed the lit guides; a lamp's interior pixel keeps its history under
    a moving camera with the option on and loses it with the option off;
  6 a tiled rank renders its rows.
The scenes are tests/aov_lights_scenes.py's; tests/test_aov_lights_host.py shows on the CPU that none of their decisions is near."""
import numpy as np
import pytest

import aov_lights_ref as AL
import aov_lights_scenes as SC
import denoise_ref as DR
import temporal_ref as T
import test_gpu_aov_shaded as TS
import variance_ref as V

pytestmark = pytest.mark.gpu

F32 = np.float32
same_bits, guides = TS.same_bits, TS.guides


def lit_scene(api, spec, W, H, option=1, **kw):
    sc = api.Scene(W, H, **kw).load(spec)
    sc.set_option("aov_lights", option)
    return sc


def sphere_normal(P, D, t, C):
    """normalize3(madd(D, t, P) - C) in float32 with the device's fma placement, then pt_render_aovs's sum over one sub-pixel and its
    normalisation (test_gpu_aov_shaded.normalised)"""
    h = np.stack([DR._fma32(D[:, k], t, P[:, k]) for k in range(3)], axis=1).astype(F32) - C.astype(F32)
    l2 = DR._fma32(h[:, 2], h[:, 2], DR._fma32(h[:, 1], h[:, 1], (h[:, 0] * h[:, 0]).astype(F32)))
    n = (h * (F32(1.0) / np.sqrt(l2.astype(F32)))[:, None]).astype(F32)
    return TS.normalised(n)


# ---------------------------------------------------------------------------- 1: primary rays, device against device
@pytest.mark.parametrize("name", sorted(SC.primary_scenes()))
def test_primary_rays_bit_for_bit(api, oracle, name):
    spec, W, H = SC.primary_scenes()[name]
    sc = lit_scene(api, spec, W, H, option=0)
    ualb, und = guides(sc, 1, 4, "geometric")
    assert sc.stat("aov_lights") == 0
    sc.set_option("aov_lights", 1)
    alb, nd = guides(sc, 1, 4, "geometric")
    assert sc.stat("aov_lights") == 1
    salb, snd = guides(sc, 1, 4, "shaded")                              # nothing to shade with: the same bits
    assert sc.stat("aov_lights") == 1 and same_bits(salb, alb) and same_bits(snd, nd)
    area = sc.debug_area_lights()
    rec, ns = area["records"], area["n_sphere"]
    rays = TS.pixel_rays(api, oracle, spec, W, H, F32(0.5), F32(0.5))
    items = np.zeros((W * H, 7), dtype=F32)
    items[:, :3], items[:, 3:6] = rays["P"][:, :3], rays["D"][:, :3]
    items[:, 6] = np.where(und[:, 3] < 0, F32(np.inf), und[:, 3])
    _, hits = sc.debug_area_light_eval(rays=items)
    on = hits["sphere"] >= 0
    j = hits["sphere"][on]
    assert same_bits(nd[on, 3], hits["t"][on])                          # the depth is the device's own t_s
    assert np.array_equal(alb[on, 3], (-2 - j).astype(F32))
    assert same_bits(alb[on, :3], rec[j, 4:7])                          # tint 1: L_j itself
    want = sphere_normal(items[on, :3], items[on, 3:6], hits["t"][on], rec[j, :3])
    if on.any():
        ulp = np.abs(nd[on, :3].astype(np.float64) - want) / np.spacing(np.maximum(np.abs(want), F32(1e-30)))
        print("%s: %d sphere pixels, normal at most %.2f ulp from the float32 formula" % (name, int(on.sum()), float(ulp.max())))
        assert ulp.max() <= 2.0
    mask = hits["suns"][:, 0].astype(np.uint64) | (hits["suns"][:, 1].astype(np.uint64) << np.uint64(32))
    sun = ~on & (und[:, 3] < 0) & (mask != 0)                           # a primary miss under a sun's disc
    for p in np.nonzero(sun)[0]:
        total, first = np.zeros(3, dtype=F32), None
        for s in range(len(rec) - ns):
            if int(mask[p]) >> s & 1:
                total = (total + rec[ns + s, 4:7]).astype(F32)
                first = s if first is None else first
        assert same_bits(alb[p, :3], total) and alb[p, 3] == F32(-2 - (ns + first))
        assert np.all(nd[p, :3] == 0) and nd[p, 3] == -1.0             # still a miss: no normal, no depth
    rest = ~on & ~sun
    assert same_bits(alb[rest], ualb[rest]) and same_bits(nd[rest], und[rest])
    seen = set(int(v) for v in j)
    if name == "suns":
        bits = np.array([bin(int(m)).count("1") for m in mask[sun]])
        assert ns == 0 and not on.any() and (bits == 2).any() and (bits == 1).any()      # two overlapping suns add
        assert not (mask[sun] >> np.uint64(2)).any()                    # the sun behind the camera is not seen
        assert (und[:, 3] > 0).any() and same_bits(nd[:, 3], und[:, 3])
    else:
        want_seen = {"front": {0}, "nothing": {0}, "hidden": set(), "two": {0, 1}, "inside": {1}, "sixtyfour": set(range(64))}[name]
        assert seen == want_seen and not sun.any()
    if name == "nothing":
        assert (und[:, 3] < 0).all() and (nd[:, 3] > 0).sum() == on.sum() > 0            # a primary miss became a hit
    if name == "hidden":
        assert same_bits(alb, ualb) and same_bits(nd, und)
    if name == "front":                                                  # without the feature the lamp's pixels carry the wall's depth
        assert np.all(nd[on, 3] < und[on, 3]) and np.all(ualb[on, 3] == 0)
    sc.close()


# ---------------------------------------------------------------------------- 2: chains against the float64 replay
@pytest.fixture(scope="module")
def chain_model(api):
    spec = SC.chain_spec()
    return spec, SC.model_of(api, spec, SC.CHAIN["W"], SC.CHAIN["H"], SC.host_area(api, spec))


@pytest.mark.parametrize("sub", [1, 2])
@pytest.mark.parametrize("shading", ["geometric", "shaded"])
def test_chains_match_float64_replay(api, chain_model, shading, sub):
    """Tolerance: |gpu - model| <= 2e-3 |model| + 1e-6 max|model| per column group, what tests/test_gpu_aov_shaded.py uses for its float64
    replay; pixels the model flags as near a decision of the triangle chain would be left out (there are none: the host test)."""
    spec, lit = chain_model
    W, H, depth = SC.CHAIN["W"], SC.CHAIN["H"], SC.CHAIN["depth"]
    sc = lit_scene(api, spec, W, H)
    sc.set_option("smooth_normals", 1)                                   # (read by the shaded run only)
    alb, nd = guides(sc, sub, depth, shading)
    assert sc.stat("aov_lights") == 1
    walb, wnd, near, margin, light, ends = AL.replay(lit, np.arange(W * H), DR.subpixel_offsets(sub), depth, shading == "shaded", False)
    keep = ~near
    assert near.mean() <= 0.02 and AL.closest_margin(margin).min() >= 1e-3
    assert all((light[keep] == k).any() for k in range(4))              # through the glass, in the mirror, in front of it, the sun in it
    assert np.array_equal(alb[keep, 3], walb[keep, 3].astype(F32))
    for what, got, want in (("albedo", alb[keep, :3], walb[keep, :3]), ("normal", nd[keep, :3], wnd[keep, :3]), ("depth", nd[keep, 3:], wnd[keep, 3:])):
        err = np.abs(got.astype(np.float64) - want)
        tol = 2e-3 * np.abs(want) + 1e-6 * float(np.abs(want).max())
        print("%s, subpixels %d, %s: worst |gpu - model| / tolerance = %.3g" % (shading, sub, what, float((err / tol).max())))
        assert np.all(err <= tol), "%s: %d values differ; worst %g of the tolerance" % (what, int((err > tol).sum()), float((err / tol).max()))
    if shading == "shaded":                                              # the bent vertex normals matter here: the geometric guides differ
        galb, gnd = guides(sc, sub, depth, "geometric")
        assert not same_bits(galb, alb) and not same_bits(gnd, nd)
    rec = sc.debug_area_lights()["records"]
    if sub == 1:
        F0 = np.asarray(api.Material(*spec.materials[2])["F0"][0][:3], dtype=np.float64)
        mirrored = np.nonzero(light == 1)[0]                             # sphere 1 is out of the camera's view: seen in the mirror only
        assert np.allclose(alb[mirrored, :3], F0 * rec[1, 4:7], rtol=2e-3)      # tint F0 x L
        glass = np.nonzero(light == 0)[0]
        assert np.allclose(alb[glass, :3], rec[0, 4:7], rtol=2e-3)      # tint 1 ...
        zs = np.array([nd[p, 3] * SC.pixel_direction(p % W, p // W, W, H)[2] for p in glass])
        assert np.allclose(zs, 5.0, rtol=1e-4)                           # ... and the depth is the slab's front face (z = 5)
        front = np.nonzero((light == 2) & (wnd[:, 3] < 5.5))[0]          # in front of the mirror (z = 6): the chain ends at d = 0, tint 1
        assert len(front) and same_bits(alb[front, :3], np.tile(rec[2, 4:7], (len(front), 1))) and np.all(nd[front, 3] < 5.5)
        sunny = np.nonzero(light == 3)[0]
        assert np.all(nd[sunny, :3] == 0) and np.all(nd[sunny, 3] > 0)   # the sun in the mirror: normal 0, the mirror's depth
    else:
        rim = (ends > 0) & (ends < sub * sub)
        assert rim.any()                                                 # pixels only some of whose chains end on a light: means over sub-pixels
    sc.close()


# ---------------------------------------------------------------------------- 3: the same bits when off
def test_off_states_render_the_parents_bits(api):
    spec, W, H = SC.primary_scenes()["front"]
    lights, bare = list(spec.area_lights), SC._spec("front", SC.wall_at(10.0), [0, 0], [])
    black = [api.sphere_light((0.42, 0.41, 6.0), 1.3, radiance=(0, 0, 0)), api.sun_light((0, 0, -1), 30.0, radiance=(0, 0, 0))]
    plain = api.Scene(W, H).load(bare)
    want = {sh: guides(plain, 2, 4, sh) for sh in ("geometric", "shaded")}
    assert plain.stat("aov_lights") == 0
    plain.close()

    def held_off(sc):
        sc.set_area_lights(lights)

    def on_no_set(sc):
        sc.set_option("aov_lights", 1)

    def on_black(sc):
        sc.set_option("aov_lights", 1)
        sc.set_area_lights(black)

    def on_cleared(sc):
        sc.set_option("aov_lights", 1)
        sc.set_area_lights(lights)
        got = guides(sc, 2, 4, "geometric")
        assert sc.stat("aov_lights") == 1 and not same_bits(got[0], want["geometric"][0])
        sc.clear_area_lights()

    for prepare in (held_off, on_no_set, on_black, on_cleared):
        sc = api.Scene(W, H).load(bare)
        prepare(sc)
        for sh in ("geometric", "shaded"):
            got = guides(sc, 2, 4, sh)
            assert sc.stat("aov_lights") == 0, prepare.__name__
            assert same_bits(got[0], want[sh][0]) and same_bits(got[1], want[sh][1]), (prepare.__name__, sh)
        sc.close()
    sc = lit_scene(api, spec, W, H)
    for sh in ("geometric", "shaded"):
        got = guides(sc, 2, 4, sh)
        assert sc.stat("aov_lights") == 1 and not same_bits(got[1], want[sh][1])
    p = api.AovParams(2, 4, api.PT_AOV_GEOMETRIC)                        # GEOMETRIC through _ex is lit too
    import ctypes as C
    sc._ck(api.LIB.pt_render_aovs_ex(sc._h, api._ptr(sc.camera), C.byref(p)))
    ex = sc.read_aovs()
    lit = guides(sc, 2, 4, "geometric")
    assert same_bits(ex[0], lit[0]) and same_bits(ex[1], lit[1])
    sc.set_option("aov_lights", 0)
    got = guides(sc, 2, 4, "geometric")
    assert sc.stat("aov_lights") == 0 and same_bits(got[0], want["geometric"][0]) and same_bits(got[1], want["geometric"][1])
    sc.close()


# ---------------------------------------------------------------------------- 4: staleness
def framed(api, spec, W, H, option):
    sc = lit_scene(api, spec, W, H, option)
    sc.set_option("moments", 1)
    sc.iterations = 3
    return sc


def new_frame(sc, spp=2):
    sc.current_sample = 0
    sc.render_nee(spp, "mis")


def test_area_light_calls_make_lit_guides_stale(api):
    spec, W, H = SC.primary_scenes()["front"]
    lights = list(spec.area_lights)
    sc = framed(api, spec, W, H, 1)
    consumers = [("denoise", sc.denoise), ("denoise_variance", sc.denoise_variance), ("temporal_accumulate", sc.temporal_accumulate)]
    for call in (lambda: sc.set_area_lights(lights), sc.clear_area_lights):
        sc.set_area_lights(lights)
        new_frame(sc)
        sc.render_aovs(1, 4)
        assert sc.stat("aov_lights") == 1
        for _, run in consumers:
            run()
        call()
        for name, run in consumers:
            with pytest.raises(api.PtError) as e:
                run()
            assert e.value.code == api.PT_EINVAL, name
        sc.set_area_lights(lights)
        new_frame(sc)
        sc.render_aovs(1, 4)                                             # rendering them again restores PT_OK
        for _, run in consumers:
            run()
        _, n = sc.read_temporal()
        assert np.all(n == sc.sample_counts().reshape(-1))               # ... and the first guides after stale ones dropped the history
    sc.close()
    # unlit guides survive the same calls, and the option invalidates nothing
    sc = framed(api, spec, W, H, 0)
    new_frame(sc)
    sc.render_aovs(1, 4)
    assert sc.stat("aov_lights") == 0
    sc.set_area_lights(lights)
    sc.denoise()
    sc.denoise_variance()
    sc.set_option("aov_lights", 1)
    sc.denoise()
    sc.render_aovs(1, 4)
    assert sc.stat("aov_lights") == 1
    sc.set_option("aov_lights", 0)
    sc.denoise()
    sc.denoise_variance()
    sc.temporal_accumulate()
    sc.close()


# ---------------------------------------------------------------------------- 5: consumers
def test_filters_match_their_models_on_lit_guides(api):
    spec, W, H = SC.primary_scenes()["front"]
    W = H = 32
    sc = framed(api, spec, W, H, 1)
    new_frame(sc, 4)
    sc.render_aovs(2, 4)
    alb, nd = sc.read_aovs()
    assert (alb[:, 3] == -2).any() and (alb[:, 3] == 0).any()
    out = sc.denoise()
    model = DR.atrous_model(sc.read_colors(), alb, nd, W, H, **api.denoise_defaults())
    err = np.abs(out[:, :3].astype(np.float64) - model[:, :3])
    tol = 2e-5 + 1e-4 * np.abs(model[:, :3])
    assert np.all(err <= tol), "pt_denoise: worst %g of the tolerance" % float((err / tol).max())
    out = sc.denoise_variance()
    model = V.variance_atrous_model(sc.read_colors(), sc.read_variance().reshape(-1), alb, nd, W, H, **api.denoise_variance_defaults())
    err = np.abs(out.astype(np.float64) - model)
    tol = 2e-5 + 1e-4 * np.abs(model)
    assert np.all(err <= tol), "pt_denoise_variance: worst %g of the tolerance" % float((err / tol).max())
    sc.close()


def parallax_spec():
    """a lamp in front of a wall, and between them a post whose edge lies behind the lamp: after the camera has stepped to the left, the
    wall behind some of the lamp's pixels is wall that the post hid from the previous view"""
    post = SC.quad((0.0, -6.0, 10.0), (5.0, -6.0, 10.0), (5.0, 6.0, 10.0), (0.0, 6.0, 10.0))
    return SC._spec("parallax", SC.wall_at(14.0) + post, [0, 0, 1, 1], [SC.sphere((-0.55, 0.1, 5.0), 1.0, (5.0, 4.0, 3.0))])


def test_temporal_accumulate_on_lit_guides(api):
    """tests/test_gpu_temporal.py's moving-camera check (its tolerances and exclusion rule) on lit guides, two frames of 4 spp with the
    camera stepping one unit to the left.  The model, fed each run's guides, picks the lamp's interior pixels (every neighbour on the lamp
    too) that it does not flag: with the option on they carry n = n_h' + k = 8; with it off the guides show the wall behind the lamp, whose
    point the post hid from the first view, so the same pixels have n = k = 4."""
    import opencl_path_tracer_amd.api as apimod
    W = H = 32
    spec = parallax_spec()
    result = {}
    for option in (1, 0):
        sc = framed(api, spec, W, H, option)
        sc.iterations = 4
        hist, shift = None, tuple(spec.shift)
        for i in range(2):
            if i:
                shift = apimod.camera_move(shift, spec.yaw, spec.pitch, 0.0, -1.0, 0.0)
            sc.set_view(spec.fov, spec.yaw, spec.pitch, shift)
            new_frame(sc, 4)
            sc.render_aovs(1, 4)
            sc.temporal_accumulate()
            alb, nd = sc.read_aovs()
            hist, info = T.accumulate(hist, sc.camera, sc.read_colors(), sc.sample_counts().reshape(-1), alb, nd, W, H, **api.temporal_defaults())
            rgbv, n = sc.read_temporal()
            ok = ~hist.bad
            assert ok.mean() >= 0.9, "option %d, frame %d: only %.4f of the pixels compared" % (option, i, ok.mean())
            err = np.abs(rgbv[ok, :3].astype(np.float64) - hist.c[ok]) - hist.tol_c[ok, None]
            assert np.all(err <= 0), "option %d, frame %d: colour, worst %r" % (option, i, err.max())
            assert np.all(np.abs(n[ok] - hist.n[ok]) <= 1e-5 * hist.n[ok])
        result[option] = (alb.copy(), n.copy(), hist.n.copy(), ok.copy())
        sc.close()
    lamp = (result[1][0][:, 3] == -2).reshape(H, W)
    interior = lamp.copy()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            interior &= np.roll(np.roll(lamp, dy, axis=0), dx, axis=1)
    interior = interior.reshape(-1)
    pick = interior & result[1][3] & result[0][3] & (result[1][2] == 8) & (result[0][2] == 4)
    print("lamp pixels %d, interior %d, picked by the model %d" % (int(lamp.sum()), int(interior.sum()), int(pick.sum())))
    assert pick.sum() >= 3
    assert np.all(result[1][1][pick] == 8) and np.all(result[0][1][pick] == 4)
    assert np.all(result[0][0][pick, 3] == 0)                            # (off: those pixels are the wall's)


# ---------------------------------------------------------------------------- 6: a tiled rank
def test_tiled_rank_renders_its_rows(api):
    spec, W, H = SC.primary_scenes()["two"]
    full = lit_scene(api, spec, W, H)
    want = guides(full, 2, 4, "geometric")
    full.close()
    sc = lit_scene(api, spec, W, H, rank=1, world=2, rows_per_block=4)
    ids = sc.local_pixel_ids()
    assert 0 < ids.size < W * H
    got = guides(sc, 2, 4, "geometric")
    assert sc.stat("aov_lights") == 1 and (got[0][:, 3] <= -2).any()
    assert same_bits(got[0], want[0][ids]) and same_bits(got[1], want[1][ids])
    sc.close()
