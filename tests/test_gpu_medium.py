"""-m gpu: the homogeneous medium of Scene.set_medium in Scene.render_nee and Scene.render_adaptive(path="nee") (pt_set_medium, the
medium instances of k_nee in pt_nee.hip, pt_debug_medium in pt_medium.hip; include/pt_api.h pins the free flight, the scatter vertex
and the transmittance of light samples).

  1 without a medium render_nee computes the bits it computed before; 2 a medium whose box the scene never enters renders, with the
  medium instances, the bits of every family they replace; 3 strategies light and mis against tests/medium_ref.py (float64, brute force,
  same LCG and hashes) on test_gpu_lights.py's replay scenes in bounded fog; 4 pt_debug_medium against the float64 statement; 5 closed
  forms: absorption in front of an emitter, single scattering around a point light; 6 the same mean in light and mis; 7 determinism,
  the flat preview, adaptive tiles, tiled ranks."""

import numpy as np
import pytest

import medium_ref as M
import nee_ref as R
import test_gpu_lights as TL

pytestmark = pytest.mark.gpu

CB_BOUNCES = TL.CB_BOUNCES
same_bits, state, same_state = TL.same_bits, TL.state, TL.same_state
# a box no ray of the Cornell scenes can enter: under the middle of the floor, which is 20,000 wide.  A ray starts above the floor, over
# it; to get below y = 0 it has to leave the floor's column first, and is then moving away from the box.  (A box far away in the open is
# not enough: a path that leaves the scene travels on for ever and would cross it)
FAR_BOX = ((-100.0, -3000.0, -100.0), (100.0, -2000.0, 100.0))


# ---------------------------------------------------------------------------- 1: no change without a medium
def test_no_medium_no_change(api, cb_spec):
    W, H = 48, 32
    for strategy in ("bsdf", "light", "mis"):
        fresh = api.Scene(W, H).load(cb_spec)
        fresh.iterations = CB_BOUNCES
        fresh.render_nee(3, strategy)
        want = state(fresh)
        zero = api.Scene(W, H).load(cb_spec)
        zero.set_medium(0.0, albedo=(0.5, 0.6, 0.7), g=0.6)
        cleared = api.Scene(W, H).load(cb_spec)
        cleared.set_medium(2e-3, albedo=0.9, g=0.6)
        cleared.clear_medium()
        for sc in (zero, cleared):
            sc.iterations = CB_BOUNCES
            sc.render_nee(3, strategy)
            assert same_state(state(sc), want), strategy
        zero.render(1)                                   # sigma_t = 0 refuses nothing
        fog = api.Scene(W, H).load(cb_spec)              # and a real medium does change the frame
        fog.set_medium(2e-3, albedo=0.9, g=0.6)
        fog.iterations = CB_BOUNCES
        fog.render_nee(3, strategy)
        got = fog.read_colors()
        assert np.isfinite(got).all() and not same_bits(got, want[0])
        with pytest.raises(api.PtError) as e:
            fog.render(1)
        assert e.value.code == api.PT_EINVAL and "pt_clear_medium" in str(e.value)


# ---------------------------------------------------------------------------- 2: a medium that is never entered
FAMILY_CASES = dict(TL.FAMILY_CASES)
FORMS = [(case, "plain") for case in sorted(FAMILY_CASES) + ["lights"]] + [(case, form) for form in ("env", "tiles", "env_tiles")
                                                                           for case in ("plain", "frosted_lens", "lights")]


@pytest.mark.parametrize("case,form", FORMS)
def test_a_medium_that_is_never_entered_keeps_every_familys_bits(api, case, form):
    """The box lies outside the scene where no ray can reach it (FAR_BOX): every clip is empty, so no segment draws a free flight and every T is exactly 1, but the
    medium instances are what launches (the other render paths refuse).  The frame must be, bit for bit, the one the family it replaces
    renders -- each of test_gpu_lights.py's family cases, and the lights family itself with a pickable set (flags bit 4) -- in the
    plain form for every family and in the env, tiles and env_tiles forms for the first, the richest and the lights family."""
    from opencl_path_tracer_amd import scenes
    W, H = 48, 40
    box, options, lens = FAMILY_CASES["plain" if case == "lights" else case]
    spec = scenes.cornell_box(**box)
    frames = []
    for medium in (False, True):
        sc = api.Scene(W, H).load(spec)
        for k, v in options.items():
            sc.set_option(k, v)
        if lens:
            sc.set_lens(25.0, 1600.0)
        if case == "lights":
            sc.set_lights([TL.box_light(api)], select=0.4)
        if form in ("env", "env_tiles"):
            sc.set_environment(scenes.sun_and_sky())
        if medium:
            sc.set_medium(5e-3, albedo=(0.9, 0.5, 0.2), g=0.6, bounds=FAR_BOX)
            with pytest.raises(api.PtError) as e:          # the medium is held: the medium family is what launches
                sc.render(1)
            assert e.value.code == api.PT_EINVAL and "pt_clear_medium" in str(e.value)
        sc.iterations = CB_BOUNCES
        if form in ("tiles", "env_tiles"):
            sc.render_adaptive(4, 8, 0.0, metric="half", path="nee", strategy="mis")
            frames.append((sc.read_colors().copy(), sc.read_rnds().copy(), sc.sample_counts().copy()))
        else:
            sc.render_nee(3, "mis")
            frames.append(state(sc))
    if form in ("tiles", "env_tiles"):
        assert same_bits(frames[0][0], frames[1][0]) and np.array_equal(frames[0][1], frames[1][1]) and np.array_equal(frames[0][2], frames[1][2])
    else:
        assert same_state(frames[0], frames[1]), (case, form)
    assert np.isfinite(frames[0][0]).all() and frames[0][0][:, :3].mean() > 0.0


# ---------------------------------------------------------------------------- 3: replay against the float64 model
# bounded fog in test_gpu_lights.py's replay room (x in [-5, 5], y in [-3, 5], z in [-1, 12], the eye at the origin): the box starts in
# front of the eye and stops short of the walls, so segments start outside it, inside it and cross it; the mean free path 1 / sigma_t is
# the room's depth
FOG = dict(sigma_t=0.08, albedo=(0.9, 0.7, 0.5), g=0.6, bounds=((-4.5, -2.5, 0.5), (4.5, 4.5, 11.5)))


def fog_replay_scene(api, sky, device=0):
    sc, spec, rgb = TL.replay_scene(api, sky, device=device)
    sc.set_medium(**FOG)
    return sc, spec, rgb


def fog_replay_model(api, sc, spec, rgb, sky):
    verts, mo = spec.objects[0]
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    env = dict(rgb=rgb, tables=sc.debug_environment(), scale=TL.REPLAY["scale"], yaw_degrees=TL.REPLAY["yaw_degrees"]) if sky else None
    return M.MediumModel(verts, recs["N"], mats, mo, sc.camera[0], sc.debug_lights(), sc.medium(), env=env, table=sc.debug_light_table())


def fog_glossy_replay_scene(api, device=0):
    sc, spec = TL.glossy_replay_scene(api, device=device)
    sc.set_medium(**FOG)
    return sc, spec


def fog_glossy_replay_model(api, sc, spec):
    verts = np.concatenate([v for v, _ in spec.objects])
    mo = np.concatenate([m for _, m in spec.objects])
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    vn = np.concatenate([np.zeros(v.shape, dtype=np.float32) if n is None else n for (v, _), n in zip(spec.objects, spec.normals)])
    return M.MediumModel(verts, recs["N"], mats, mo, sc.camera[0], sc.debug_lights(), sc.medium(), vnormals=vn, table=sc.debug_light_table())


def check_replay(sc, model, seeds, strategy, need):
    spp, bounces = TL.REPLAY["spp"], TL.REPLAY["bounces"]
    want, want_seeds, ties = model.render(seeds, bounces, spp, strategy)
    got = sc.read_colors()[:, :3].astype(np.float64)
    keep = ~ties
    events = {k: int(v[keep].sum()) for k, v in model.pixel_events.items()}
    print("near ties: %.2f %% (%d of %d pixels); events in the kept pixels: %s" % (100.0 * ties.mean(), int(ties.sum()), ties.size, events))
    assert keep.mean() > 0.9, "too many near-tie pixels: %d" % int(ties.sum())
    for name in need:
        assert events[name] > 0, name
    assert np.array_equal(sc.read_rnds()[keep], want_seeds[keep])
    scale = float(want[keep].max())
    err = np.abs(got[keep] - want[keep])
    worst = float((err / (np.abs(want[keep]) + 1e-6 * scale)).max())
    print("worst relative error %g" % worst)
    bad = err > 2e-3 * np.abs(want[keep]) + 1e-6 * scale
    assert not bad.any(), "%d of %d pixel channels differ; worst %g" % (int(bad.sum()), bad.size, worst)
    assert float(want[keep].mean()) > 0.0


@pytest.mark.parametrize("sky", [True, False])
@pytest.mark.parametrize("strategy", ["light", "mis"])
def test_matches_float64_model(api, strategy, sky):
    """test_gpu_lights.py's replay scene (48 x 32, 2 spp, 4 bounces, its three lights) in the bounded fog FOG.  The model alone, on these
    seeds, flags 0.52 % (sky) / 0.59 % (no sky) of the pixels as near ties in both strategies (measured on a host-only context before
    the first GPU run; cap 10 %).  In the kept pixels 1,453 of the 1,536 pixels scatter at least once: 3,745 / 3,737 scatter vertices
    in 3,072 samples, 1,842 / 2,179 light samples at one reach their light, 630 of them a delta light's, and 533 sky misses follow a
    scatter vertex.  The tolerance and the cap are that test's."""
    sc, spec, rgb = fog_replay_scene(api, sky)
    seeds = TL.replay_seeds()
    sc.upload_seeds(seeds)
    sc.iterations = TL.REPLAY["bounces"]
    sc.render_nee(TL.REPLAY["spp"], strategy)
    model = fog_replay_model(api, sc, spec, rgb, sky)
    assert model.pa == 0.5 and model.pe == (0.5 if sky else 0.0) and model.medium["sigma_t"] == float(np.float32(FOG["sigma_t"]))
    need = ("scatter", "scatter_light", "scatter_delta", "delta") + (("scatter_sky",) if sky and strategy == "mis" else ())
    check_replay(sc, model, seeds, api.NEE_STRATEGIES[strategy], need)


def test_matches_float64_model_under_smooth_normals_and_glossy(api):
    """Options smooth_normals + glossy on test_gpu_lights.py's glossy replay scene (a closed box: a type-4 floor, spheres with vertex
    normals, a glass sphere the path may be inside of) in the same fog, strategy mis.  The model alone flags 1.17 % of the pixels as near
    ties (host-only context, before the first GPU run; cap 10 %); the kept pixels hold 3,401 scatter vertices with 1,780 light samples
    (539 delta) next to 1,528 glossy vertices, and 48 emitter hits after a scatter vertex with W_b < 1."""
    sc, spec = fog_glossy_replay_scene(api)
    seeds = TL.replay_seeds()
    sc.upload_seeds(seeds)
    sc.iterations = TL.REPLAY["bounces"]
    sc.render_nee(TL.REPLAY["spp"], "mis")
    model = fog_glossy_replay_model(api, sc, spec)
    check_replay(sc, model, seeds, 2, ("scatter", "scatter_light", "scatter_delta", "glossy_vertex", "glossy_light", "delta_glossy"))


# ---------------------------------------------------------------------------- 4: pt_debug_medium
def dc(g):
    """what float32 leaves of the cosine computed through the inverse cdf.  Isotropic: 1 - 2 u1, two roundings of numbers up to 2.  Else
    r = (1 - g^2) / ((1 - g) + 2 g u1): g^2 is rounded (2^-24 g^2) before the cancellation in 1 - g^2, so r carries a relative error of
    2^-24 (g^2 / (1 - g^2) + 3) (the denominator's two roundings and the divide are the 3); c = ((1 + g^2) - r^2) / (2 g) with r <= 1 + g,
    r^2 <= 4: 2 r^2 times that, plus four roundings of numbers up to 4 in the numerator, over 2 |g|: 1.3e-5 for g = 0.99, 1.8e-6 for 0.6"""
    e = 2.0 ** -24
    if abs(g) < 1e-3:
        return 4 * e
    return (8 * e * (g * g / (1 - g * g) + 3) + 8 * e) / (2 * abs(g))


def debug_items():
    """hand-made rays against the box [0, 2] x [0, 4] x [0, 6] and random ones: {P, D, t, u, u1, u2, limit, 0}"""
    s3 = 1.0 / 3.0
    hand = [  # starts inside; starts outside; parallel to four faces, inside and outside their slabs; misses; u near 0 and near 1
        ([1, 1, 1], [0, 0, 1], 100.0, 0.25, 0.3, 0.6, 3.0), ([1, 1, -2], [0, 0, 1], np.inf, 0.5, 0.9, 0.1, np.inf),
        ([-5, 1, 1], [1, 0, 0], np.inf, 0.75, 0.5, 0.5, 6.0), ([-5, 4.5, 1], [1, 0, 0], np.inf, 0.75, 0.5, 0.5, np.inf),
        ([-1, 10, 1], [1, 0, 0], 50.0, 0.1, 0.2, 0.3, 20.0), ([-1, -2, -2], [s3, 2 * s3, 2 * s3], np.inf, 2.0 ** -24, 0.0, 0.0, np.inf),
        ([1, 2, 3], [0.6, 0, 0.8], 2.0, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24, 0.5), ([1, 2, 3], [0, -1, 0], np.inf, 0.0, 0.5, 0.25, np.inf)]
    rng = np.random.default_rng(5)
    items = [list(p) + list(d) + [t, u, u1, u2, lim, 0.0] for p, d, t, u, u1, u2, lim in hand]
    for _ in range(120):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        lim = np.inf if rng.random() < 0.3 else rng.uniform(0.5, 12.0)
        t = np.inf if rng.random() < 0.3 else rng.uniform(0.5, 12.0)
        items.append(list(rng.uniform(-3.0, 7.0, 3)) + list(d) + [t] + list(rng.random(3)) + [lim, 0.0])
    return np.asarray(items, dtype=np.float32)


@pytest.mark.parametrize("g", [0.0, 0.6, -0.6, 0.99])
def test_debug_medium_matches_the_float64_statement(api, cb_spec, g):
    """a, b (three roundings: 1 / D, the difference, the product), d (log1pf within 2 ulp, the divide) and T (expf, the product and what
    a and b carry into the exponent) to those float32 roundings; the direction unit; its cosine to D the inverse cdf's within dc(g); p_b
    HG of the returned angle and of the float64 cosine within what dc(g) leaves of q^1.5, q = 1 + g^2 - 2 g c (1.5 x 2 |g| dc / q: q
    is 1e-4 for g = 0.99 straight ahead)."""
    DC = dc(float(np.float32(g)))
    sc = api.Scene(16, 16).load(cb_spec)
    lo, hi = (0.0, 0.0, 0.0), (2.0, 4.0, 6.0)
    sigma = 0.35
    sc.set_medium(sigma, albedo=0.5, g=g, bounds=(lo, hi))
    items = debug_items()
    out = sc.debug_medium(items).astype(np.float64)
    assert np.isfinite(out[:, 2:]).all()
    g32, sig32 = float(np.float32(g)), float(np.float32(sigma))
    med = dict(sigma_t=sig32, lo=np.asarray(lo), hi=np.asarray(hi))
    scattered = 0
    for it, o in zip(items.astype(np.float64), out):
        P, D, t, u, u1, u2, lim = it[0:3], it[3:6], it[6], it[7], it[8], it[9], it[10]
        a, b, near = M.clip(med["lo"], med["hi"], P, D, t)
        ell = max(b - a, 0.0)
        tol = lambda v: 4e-7 * abs(v) + 1e-30
        if ell > 0 and not near:
            assert abs(o[0] - a) <= tol(a) and (o[1] == b or abs(o[1] - b) <= tol(b)), (it, o)
        else:
            assert not near and max(o[1] - o[0], 0.0) == 0.0 or near
        d = M.flight(sig32, u)
        assert abs(o[3] - d) <= 4e-7 * d, (u, o[3], d)
        if not near and not (np.isfinite(ell) and abs(d - ell) < M.FLIGHT_MARGIN * max(d, ell)):
            assert o[2] == float(d < ell), (it, o)
            scattered += int(d < ell)
        w = o[4:7]
        assert abs(np.linalg.norm(w) - 1.0) < 4e-7
        wd, pb, c = M.direction(g32, D / np.linalg.norm(D), u1, u2)
        cos_out = float(w @ D) / np.linalg.norm(D)
        assert abs(cos_out - c) <= DC + 4e-7, (g, u1, cos_out, c)
        s = np.sqrt(max(0.0, 1.0 - c * c))
        perp = (w - D * (w @ D) / (D @ D)) - (wd - D * (wd @ D) / (D @ D))
        assert np.abs(perp).max() <= 2e-6 + min(DC * abs(c) / max(s, 1e-12), np.sqrt(2 * DC)), (g, u1, u2)
        q = 1.0 + g32 * g32 - 2.0 * g32 * c
        rel = 1.5 * 2.0 * abs(g32) * (DC + 4e-7) / q + 1e-6
        assert abs(o[7] - pb) <= rel * pb and abs(o[7] - M.hg(g32, cos_out)) <= rel * pb, (g, u1, o[7], pb)
        T, nearT = M.transmittance(med, P, D, lim)
        aT, bT, _ = M.clip(med["lo"], med["hi"], P, D, lim)
        if not nearT:
            span = (abs(aT) + abs(bT)) if np.isfinite(aT) and np.isfinite(bT) else 0.0
            assert abs(o[8] - T) <= 4e-7 * (2.0 + sig32 * span) * T, (it, o[8], T)
            if max(bT - aT, 0.0) == 0.0:
                assert o[8] == 1.0
    assert scattered > 10
    # an unbounded medium: the whole segment, and T = 0 over an uncut shadow ray
    sc.set_medium(sigma, g=g)
    o = sc.debug_medium(items[:2])
    assert o[0, 0] == 0.0 and o[0, 1] == 100.0 and o[1, 1] == np.inf and o[1, 8] == 0.0
    assert abs(float(o[0, 8]) - np.exp(-sig32 * 3.0)) <= 4e-7 * np.exp(-sig32 * 3.0)


# ---------------------------------------------------------------------------- 5: closed forms
LE = (3.0, 2.0, 1.0)


def emitter_spec():
    """an emitting quad 80 x 80 at z = 20 facing a level camera at the origin (fov 60): every pixel sees it"""
    from opencl_path_tracer_amd import scenes
    mats = [((0, 0, 0), (0, 0, 0), LE, (0, 0, 0), (0, 0, 0), 0.0, 3)]
    a, b, c, d = (-40.0, -40.0, 20.0), (40.0, -40.0, 20.0), (40.0, 40.0, 20.0), (-40.0, 40.0, 20.0)
    spec = scenes.SceneSpec(materials=mats, fov=60.0, shift=TL.EYE_AT_ORIGIN, name="emitter")
    spec.objects.append((np.asarray([(a, b, c), (a, c, d)], dtype=np.float32), np.zeros(2, dtype=np.uint16)))
    return spec


@pytest.mark.parametrize("bounds", [None, ((-3.0, -np.inf, 5.0), (40.0, np.inf, 12.0))], ids=["unbounded", "slab"])
def test_absorption_in_front_of_an_emitter(api, bounds):
    """albedo 0, strategy bsdf, iterations = 2, one sample per pixel at 96 x 64: sample i is a Bernoulli trial -- it reaches the emitter
    with probability p_i = exp(-sigma_t l_i) and is then worth v_i = (factor_L + factor_B) Le cos_i = 2 Le cos_i (the reference's
    integrand at a directly seen emitter: both factors are 1 before the first type-0 vertex), else it is absorbed and worth 0; the
    emitter's own bounce leaves towards the camera's side and finds nothing.  The rays are known exactly (seeds uploaded, one sample),
    so the frame mean has expectation (1 / n) sum v_i p_i and, the trials being independent, variance (1 / n^2) sum v_i^2 p_i (1 - p_i)
    (the binomial model with unequal trials).  The tolerance is five of those standard deviations, per channel; l_i is the clip of the
    ray up to its hit in float64 (the slab box spans z in [5, 12] and is cut at x = -3, so the rays cross it obliquely, for a short or a long way)."""
    W, H = 96, 64
    spec = emitter_spec()
    sigma = 0.05
    sc = api.Scene(W, H).load(spec)
    seeds = np.random.default_rng(23).integers(1, 2 ** 31 - 2, W * H).astype(np.int32)
    sc.upload_seeds(seeds)
    sc.iterations = 2
    sc.render_nee(1, "bsdf")
    clear = sc.read_colors()[:, :3].astype(np.float64)
    verts, mo = spec.objects[0]
    model = R.Model(verts, api.triangles_from_vertices(verts, mo)["N"], np.concatenate([api.Material(*m) for m in spec.materials]), mo, sc.camera[0])
    lo, hi = (np.full(3, -np.inf), np.full(3, np.inf)) if bounds is None else (np.asarray(bounds[0]), np.asarray(bounds[1]))
    v, p = np.zeros((W * H, 3)), np.zeros(W * H)
    for i in range(W * H):
        s, r1 = R.lcg(int(seeds[i]))
        s, r2 = R.lcg(s)
        P, D = model.camera_ray(i, r1, r2)
        t = 20.0 / D[2]
        a, b, _ = M.clip(lo, hi, P, D, t)
        v[i] = 2.0 * np.asarray(LE) * D[2]
        p[i] = np.exp(-sigma * max(b - a, 0.0))
    assert np.allclose(clear, v, rtol=1e-5)                          # the fog-free frame is v itself
    sc.set_medium(sigma, albedo=0.0, g=0.3, bounds=bounds)
    sc.current_sample = 0
    sc.upload_seeds(seeds)
    sc.render_nee(1, "bsdf")
    got = sc.read_colors()[:, :3].astype(np.float64)
    reached = got.any(axis=1)
    assert np.allclose(got[reached], v[reached], rtol=1e-5)          # a sample is worth v_i or nothing
    want = (v * p[:, None]).mean(axis=0)
    sd = np.sqrt((v * v * (p * (1.0 - p))[:, None]).sum(axis=0)) / (W * H)
    print("absorption: mean %s, expected %s, standard deviation %s, survivors %.3f (expected %.3f)" % (got.mean(axis=0), want, sd, reached.mean(), p.mean()))
    assert 0.2 < p.mean() < 0.9 and (bounds is None or (p.max() > 0.95 and p.min() < 0.75))      # (the slab: short and long crossings)
    assert (np.abs(got.mean(axis=0) - want) <= 5.0 * sd).all()


def airlight_spec():
    """nothing in view: one small black triangle behind the camera, and a point light beside the view"""
    from opencl_path_tracer_amd import scenes
    mats = [((0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0)]
    spec = scenes.SceneSpec(materials=mats, fov=60.0, shift=TL.EYE_AT_ORIGIN, name="airlight")
    spec.objects.append((np.asarray([((-1.0, -1.0, -5.0), (1.0, -1.0, -5.0), (0.0, 1.0, -5.0))], dtype=np.float32), np.zeros(1, dtype=np.uint16)))
    return spec


AIR = dict(W=32, H=24, spp=128, sigma=0.15, albedo=(0.9, 0.6, 0.3), light=(6.0, 1.0, 8.0), I=(40.0, 30.0, 20.0), block=(slice(4, 20), slice(8, 24)))


def airlight_quadrature(cam, gid, g, f=np.float64):
    """the expectation of one sample of pixel gid: over the pixel's footprint (2 x 2 Gauss points) the integral along the ray of
    (factor_L + factor_B) albedo sigma_t e^{-sigma_t s} HG(g, cos) I / r^2 e^{-sigma_t r} ds, substituted u = 1 - e^{-sigma_t s} and
    summed by Gauss-Legendre on 16 panels of 48 points"""
    model = R.Model(np.zeros((1, 3, 3)) + np.eye(3), np.array([[0.0, 0.0, 1.0]]), [dict(emission=np.zeros(4), type=0)], [0], cam)
    x, w = np.polynomial.legendre.leggauss(48)
    edges = np.linspace(0.0, 1.0, 17)
    gp = 0.5 + np.array([-0.5, 0.5]) / np.sqrt(3.0)
    sigma, Lp = AIR["sigma"], np.asarray(AIR["light"])
    total = np.zeros(3)
    for r1 in gp:
        for r2 in gp:
            P, D = model.camera_ray(gid, r1, r2)
            acc = 0.0
            for lo, hi in zip(edges[:-1], edges[1:]):
                u = 0.5 * (hi - lo) * x + 0.5 * (hi + lo)
                s = -np.log1p(-u) / sigma
                pts = P[None, :] + D[None, :] * s[:, None]
                dv = Lp[None, :] - pts
                r = np.linalg.norm(dv, axis=1)
                cosv = (dv @ D) / r
                acc += float((M.hg(g, cosv) / (r * r) * np.exp(-sigma * r) * w).sum()) * 0.5 * (hi - lo)
            total += 0.25 * acc * 2.0 * np.asarray(AIR["albedo"]) * np.asarray(AIR["I"])
    return total


@pytest.mark.parametrize("g", [0.0, 0.6])
def test_single_scattering_around_a_point_light(api, g):
    """a point light in unbounded fog, no surface in view, iterations = 2, strategy light: every sample scatters once on segment 0 and
    takes one light sample (P_ana = P_light = 1), so a pixel's expectation is the airlight integral (airlight_quadrature; factor_L +
    factor_B = 2 as at a directly seen emitter).  The mean of a 16 x 16 block of pixels, 128 samples each, against the mean of their
    quadratures; the tolerance is five standard errors of that mean, the per-sample deviation taken from 4 samples per pixel of
    tests/medium_ref.py's model of the same pixels (other seeds), not from the frame."""
    W, H, spp = AIR["W"], AIR["H"], AIR["spp"]
    spec = airlight_spec()
    sc = api.Scene(W, H).load(spec)
    sc.set_lights([api.point_light(AIR["light"], AIR["I"])])
    sc.set_medium(AIR["sigma"], albedo=AIR["albedo"], g=g)
    assert sc.debug_lights()["P_ana"] == 1.0
    sc.iterations = 2
    sc.render_nee(spp, "light")
    got = sc.read_colors()[:, :3].astype(np.float64).reshape(H, W, 3)[AIR["block"]].reshape(-1, 3)
    ids = np.arange(W * H).reshape(H, W)[AIR["block"]].reshape(-1)
    want = np.array([airlight_quadrature(sc.camera[0], int(i), float(np.float32(g))) for i in ids])
    verts, mo = spec.objects[0]
    model = M.MediumModel(verts, api.triangles_from_vertices(verts, mo)["N"], np.concatenate([api.Material(*m) for m in spec.materials]), mo,
                          sc.camera[0], sc.debug_lights(), sc.medium(), table=sc.debug_light_table())
    rng = np.random.default_rng(3)
    samples = np.array([[model.sample(int(i), int(rng.integers(1, 2 ** 31 - 2)), 2, 1)[0] for _ in range(4)] for i in ids])      # (pixels, 4, 3)
    assert abs(samples.mean(axis=(0, 1)) / want.mean(axis=0) - 1.0).max() < 0.2                  # the model itself is on the quadrature
    sd = samples.reshape(-1, 3).std(axis=0, ddof=1)
    se = sd / np.sqrt(len(ids) * spp)
    print("airlight g = %g: block mean %s, quadrature %s, standard error %s" % (g, got.mean(axis=0), want.mean(axis=0), se))
    assert (want.mean(axis=0) > 0).all() and (se < 0.05 * want.mean(axis=0)).all()
    assert (np.abs(got.mean(axis=0) - want.mean(axis=0)) <= 5.0 * se).all()


# ---------------------------------------------------------------------------- 6: the same expectation in both strategies
def test_light_and_mis_agree_in_the_fogged_box(api):
    """scenes.cornell_box(fog=1e-3), 32 x 24, 256 samples, option moments: the frame's mean luminance in light and in mis, each with the
    variance of that mean from the per-pixel variance read-out (pixels are independent: the sum of their variances over n^2); they must
    agree within five combined standard errors."""
    from opencl_path_tracer_amd import scenes
    W, H, spp = 32, 24, 256
    mean, var = {}, {}
    for k, strategy in enumerate(("light", "mis")):
        sc = api.Scene(W, H).load(scenes.cornell_box(fog=1e-3))
        sc.set_option("moments", 1)
        sc.upload_seeds(np.random.default_rng(100 + k).integers(1, 2 ** 31 - 2, W * H).astype(np.int32))
        sc.iterations = CB_BOUNCES
        sc.render_nee(spp, strategy)
        c = sc.read_colors()[:, :3].astype(np.float64)
        v = sc.read_variance().astype(np.float64).reshape(-1)
        assert np.isfinite(c).all() and np.isfinite(v).all()
        mean[strategy] = float((0.2126 * c[:, 0] + 0.7152 * c[:, 1] + 0.0722 * c[:, 2]).mean())
        var[strategy] = float(v.sum()) / (W * H) ** 2
    z = abs(mean["light"] - mean["mis"]) / np.sqrt(var["light"] + var["mis"])
    print("light %.6g, mis %.6g, combined standard error %.3g: z = %.2f" % (mean["light"], mean["mis"], np.sqrt(var["light"] + var["mis"]), z))
    assert mean["mis"] > 0 and z < 5.0


# ---------------------------------------------------------------------------- 7: other paths
def fog_box(api, W, H, sky=False, **kw):
    from opencl_path_tracer_amd import scenes
    sc = api.Scene(W, H, **kw).load(scenes.cornell_box(fog=1.5e-3))
    if sky:
        sc.set_environment(scenes.sun_and_sky())
    sc.set_lights([TL.box_light(api)], select=0.4)
    sc.iterations = CB_BOUNCES
    return sc


def test_runs_repeat_and_the_flat_preview_is_the_surface_or_black(api, cb_spec):
    W, H = 48, 40
    runs = []
    for _ in range(2):
        sc = fog_box(api, W, H)
        sc.render_nee(2, "mis")
        sc.render_nee(1, "mis")
        runs.append(state(sc))
    assert same_state(runs[0], runs[1])
    plain = api.Scene(W, H).load(cb_spec)
    plain.iterations = 1
    plain.render_nee(1, "mis")
    flat = plain.read_colors()[:, :3]
    fog = fog_box(api, W, H)
    fog.iterations = 1
    fog.render_nee(1, "mis")
    got = fog.read_colors()[:, :3]
    black = ~got.any(axis=1)
    assert 0 < black.sum() < W * H and same_bits(got[~black], flat[~black])      # one iteration: a scatter ends the sample black


@pytest.mark.parametrize("sky", [False, True])
def test_adaptive_nee_tiles_hold_render_nee_bits(api, sky):
    """k_nee_tiles_medium / k_nee_env_tiles_medium against k_nee_medium / k_nee_env_medium at 36 x 20: ragged tiles on the right and at
    the bottom"""
    W, H = 36, 20
    sc = fog_box(api, W, H, sky)
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
        fresh = fog_box(api, W, H, sky)
        fresh.render_nee(k, "mis")
        sel = counts == k
        assert same_bits(cols[sel, :3], fresh.read_colors()[sel, :3]) and np.array_equal(rnds[sel], fresh.read_rnds()[sel]), k


def test_tiled_ranks_assemble_the_single_context_frame(api):
    W, H, world = 48, 36, 2
    one = fog_box(api, W, H)
    one.render_nee(3, "mis")
    whole = state(one)
    seen = np.zeros(W * H, dtype=bool)
    for r in range(world):
        sc = fog_box(api, W, H, rank=r, world=world, rows_per_block=8)
        sc.render_nee(3, "mis")
        ids = sc.local_pixel_ids()
        assert same_state(state(sc), tuple(a[ids] for a in whole)), r
        seen[ids] = True
    assert seen.all()
