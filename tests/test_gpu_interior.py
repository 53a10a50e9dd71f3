"""-m gpu: interiors of dielectrics on Scene.render_nee (Scene.set_material_interior; include/pt_api.h pins the estimator, DESIGN.md
section 5.21): the eleventh k_nee family, stat "nee_family" 10.

  1 a null binding keeps every bit of the unbound frame, with fog, with a grid and with neither, in all four forms
  2 pt_debug_interior against the float64 statement
  3 a float64 replay (tests/interior_ref.py) in a closed box with a glass sphere, with and without fog, and one with a type-6 boundary
  4 Beer-Lambert in closed form through a glass slab
  5 scattering keeps energy under a constant sky
  6 a nearly index-matched box with an interior against the same box as bounded fog, in the mean
  7 every instance: four forms x four node modes, bit for bit
  8 adaptive tiles and tiled ranks hold render_nee's bits
  9 a binding on a material that is neither of type 2 nor 6 is ignored"""

import numpy as np
import pytest

import interior_ref as IR
import medium_ref as M
import nee_instances as I
import nee_ref as R
import test_gpu_coated as TC
import test_gpu_frosted as TF
import test_gpu_lights as TL
import test_gpu_medium as TM
import test_gpu_nee_instances as TI
import test_interior_host as TH

pytestmark = pytest.mark.gpu

same_bits, state, same_state = TL.same_bits, TL.state, TL.same_state
FAMILY = 10


def glass_materials(spec):
    return [i for i, m in enumerate(spec.materials) if m[6] in (2, 6)]


def bind(sc, spec, **kw):
    mats = glass_materials(spec)
    assert mats
    for m in mats:
        sc.set_material_interior(m, **kw)
    return mats


# ---------------------------------------------------------------------------- 1: the null binding
@pytest.mark.parametrize("form", range(4), ids=I.FORMS)
@pytest.mark.parametrize("base", ["fog", "grid", "neither"])
def test_a_null_binding_keeps_every_bit(api, base, form):
    """tests/nee_instances.py's small scene with every feature live (types 2 and 6 on the second sphere), the tree in LDS: an all-zero
    interior on both glass materials takes family 10 and renders the colours, rnds and rays (the sample counts of a tiled form) of the
    unbound frame, which family 8 (fog), 9 (a 3 x 2 x 2 grid) or 7 (neither) rendered."""
    config = "lights" if base == "neither" else "medium"
    frames, thr = [], None
    for bound in (False, True):
        sc, mode = I.build(api, "small", config, "lds", sky=bool(form & 1))
        if base == "grid":
            sc.set_medium_density(np.linspace(0.25, 2.0, 12, dtype=np.float32).reshape(2, 2, 3))
        if bound:
            bind(sc, I.scene_spec("small", True, True))
        if form & 2 and thr is None:
            sc.iterations = TL.CB_BOUNCES
            thr = TI.threshold_of(sc)
        frames.append(TI.render(sc, form, thr))
        want = FAMILY if bound else {"fog": 8, "grid": 9, "neither": 7}[base]
        assert (int(sc.stat("nee_family")), int(sc.stat("nee_form")), int(sc.stat("node_mode"))) == (want, form, mode)
        sc.close()
    assert frames[0][0][:, :3].mean() > 0.0 and TI.same_frames(frames[1], frames[0])


# ---------------------------------------------------------------------------- 2: pt_debug_interior
def test_debug_interior_matches_the_float64_statement(api, cb_spec):
    """d and l to test_gpu_medium.py's tolerance for its debug call (4e-7 |v| + 1e-30: log1pf within 2 ulp, the divide); the scatter
    decision exactly, away from ties (FLIGHT_MARGIN); the factor expf(-(sigma_a l)) to the product's rounding and l's error in the
    exponent x (6e-7 x) plus expf's 1 ulp and the format's half ulp (2.4e-7), exactly 1 for a channel without absorption; the
    direction as that test holds the medium's (unit, its cosine within dc(g))."""
    sc = api.Scene(16, 16).load(cb_spec)
    rng = np.random.default_rng(9)
    items = []
    for g in (0.0, 0.6, -0.6, 0.99):
        for _ in range(60):
            D = rng.normal(size=3)
            D /= np.linalg.norm(D)
            sa = rng.uniform(0.0, 1.5, 3) * (rng.random(3) < 0.7)
            ss = 0.0 if rng.random() < 0.2 else rng.uniform(0.05, 2.0)
            items.append(list(sa) + [ss, g, rng.uniform(0.05, 6.0)] + list(rng.random(3)) + list(D))
    items.append([0.3, 0.0, 0.1, 0.8, 0.3, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])                       # u = 0: a scatter at distance 0
    items.append([0.3, 0.0, 0.1, 0.8, 0.3, 2.0, 1.0 - 2.0 ** -24, 0.5, 0.5, 0.0, 1.0, 0.0])          # the largest u
    items = np.asarray(items, dtype=np.float32)
    out = sc.debug_interior(items).astype(np.float64)
    assert np.isfinite(out).all()
    tol = lambda v: 4e-7 * abs(v) + 1e-30
    scattered = survived = 0
    for it, o in zip(items.astype(np.float64), out):
        sa, ss, g, t, u, u1, u2, D = it[0:3], it[3], it[4], it[5], it[6], it[7], it[8], it[9:12]
        if ss > 0:
            d = M.flight(ss, u)
            assert abs(o[0] - d) <= tol(d), (it, o)
            tie = abs(d - t) < M.FLIGHT_MARGIN * max(d, t)
            sc_ = d < t
        else:
            assert o[0] == -1.0
            d, tie, sc_ = np.inf, False, False
        if tie:
            continue
        assert o[1] == float(sc_), (it, o)
        scattered += int(sc_)
        survived += int(not sc_)
        ell = d if sc_ else t
        assert abs(o[2] - ell) <= tol(ell) and (sc_ or o[2] == t)
        for c in range(3):
            x = sa[c] * ell
            f = np.exp(-x)
            assert abs(o[3 + c] - f) <= f * (6e-7 * x + 2.4e-7), (it, o)
            if sa[c] == 0.0:
                assert o[3 + c] == 1.0
        w = o[6:9]
        assert abs(np.linalg.norm(w) - 1.0) < 4e-7
        _, _, c = M.direction(g, D / np.linalg.norm(D), u1, u2)
        assert abs(float(w @ D) / np.linalg.norm(D) - c) <= TM.dc(g) + 4e-7
        assert o[9] == 0.0
    assert scattered > 40 and survived > 40


# ---------------------------------------------------------------------------- 3: the float64 replay
INTERIOR = dict(sigma_a=(0.4, 0.1, 0.02), sigma_s=0.77, g=0.5)      # the glass sphere's diameter is 2.6: two mean free paths across
REPLAY_BOUNCES = TL.REPLAY["bounces"] + 4
GLASS_SPHERE = 6                                                     # its material in test_gpu_lights.glossy_replay_spec


def interior_replay_scene(api, fog, device=0):
    sc, spec = TL.glossy_replay_scene(api, device=device)
    if fog:
        sc.set_medium(**TM.FOG)
    sc.set_material_interior(GLASS_SPHERE, **INTERIOR)
    return sc, spec


def interior_replay_model(api, sc, spec):
    verts = np.concatenate([v for v, _ in spec.objects])
    mo = np.concatenate([m for _, m in spec.objects])
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    vn = np.concatenate([np.zeros(v.shape, dtype=np.float32) if n is None else n for (v, _), n in zip(spec.objects, spec.normals)])
    return IR.InteriorModel(verts, recs["N"], mats, mo, sc.camera[0], sc.debug_lights(), sc.medium(), {GLASS_SPHERE: sc.material_interior(GLASS_SPHERE)},
                            vnormals=vn, table=sc.debug_light_table())


def check_replay(sc, model, seeds, strategy, need, bounces, spp=TL.REPLAY["spp"]):
    """test_gpu_medium.check_replay -- its tolerance, its cap of 10 % on near ties -- at a given number of bounces"""
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


NEED = ("interior_scatter", "interior_absorbed", "interior_exit", "interior_then_light")


@pytest.mark.parametrize("fog", [False, True], ids=["clear", "fog"])
def test_matches_float64_model(api, fog):
    """test_gpu_lights.py's glossy replay scene (a closed box, a type-4 floor, spheres with vertex normals, three analytic lights) at
    48 x 32, 2 spp, strategy mis, 8 bounces, the glass sphere holding INTERIOR; once in test_gpu_medium.py's fog as well.  The model
    alone, on these seeds, flags 1.89 % (clear) / 1.76 % (fog) of the 1,536 pixels as near ties (measured on a host-only context before
    the first GPU run; cap 10 %).  In the kept pixels, clear / fog: 1,126 / 919 interior scatter vertices, 722 / 556 segments that reach
    the boundary absorbed, 281 / 246 exits after a scatter inside, and 5 / 4 emitter hits later on a path that scattered inside (the
    fog adds 5,246 scatter vertices of its own).  The model takes 13 to 15 s of CPU time per case (eight bounces, brute force)."""
    sc, spec = interior_replay_scene(api, fog)
    seeds = TL.replay_seeds()
    sc.upload_seeds(seeds)
    sc.iterations = REPLAY_BOUNCES
    sc.render_nee(TL.REPLAY["spp"], "mis")
    assert sc.stat("nee_family") == FAMILY
    model = interior_replay_model(api, sc, spec)
    assert (model.medium is not None) == fog and model.interiors[GLASS_SPHERE]["sigma_s"] == float(np.float32(INTERIOR["sigma_s"]))
    check_replay(sc, model, seeds, 2, NEED + (("scatter",) if fog else ()), REPLAY_BOUNCES)


FROSTED_BOUNCES = TF.REPLAY["bounces"] + 4


def frosted_replay_scene(api, device=0):
    """test_gpu_frosted.replay_scene (options smooth_normals, glossy, coated and frosted on test_gpu_frosted.replay_spec: a type-6 sphere
    and a type-6 pane with a single face) with INTERIOR bound to the type-6 material"""
    spec = TF.replay_spec()
    sc = api.Scene(TF.REPLAY["W"], TF.REPLAY["H"], device=device).load(spec)
    for opt in ("smooth_normals", "glossy", "coated", "frosted"):
        sc.set_option(opt, 1)
    sc.set_material_interior(TF.FROSTED, **INTERIOR)
    return sc, spec


def frosted_replay_seeds():
    return np.random.default_rng(17).integers(1, 2 ** 31 - 2, TF.REPLAY["W"] * TF.REPLAY["H"]).astype(np.int32)


def frosted_replay_model(api, sc, spec):
    verts = np.concatenate([v for v, _ in spec.objects])
    mo = np.concatenate([m for _, m in spec.objects])
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    vn = np.concatenate([np.zeros(v.shape, dtype=np.float32) if n is None else n for (v, _), n in zip(spec.objects, spec.normals)])
    _, _, _, _, ps_err = TC.float32_restatement(TC.coated_inputs())
    _, _, _, _, fm_err, disc_err = TF.float32_restatement(TF.frosted_inputs())
    return IR.InteriorFrostedModel(verts, recs["N"], mats, mo, sc.camera[0], vn, table=sc.debug_light_table(), ps_margin=ps_err,
                                   fm_margin=max(fm_err, disc_err), interiors={TF.FROSTED: sc.material_interior(TF.FROSTED)})


def test_matches_float64_model_with_a_frosted_boundary(api):
    """test_gpu_frosted.py's replay scene (32 x 24, 4 spp, strategy mis; a type-6 sphere of alpha 0.25 and a type-6 pane with a single
    face, through which a path stays `inside` in the open room, so that segments that end on the sphere there take its interior too)
    at 8 bounces with INTERIOR bound to the type-6 material, against tests/interior_ref.py's InteriorFrostedModel: FrostedModel's
    estimator with the interior rule added.  That test's margins for near ties, check_replay's tolerance and its cap of 10 %.  The
    model alone, on these seeds, flags 4.95 % (38) of the 768 pixels as near ties (measured on a host-only context before the first
    GPU run).  In the kept pixels: 726 interior scatter vertices, 383 segments that reach the boundary absorbed, 129 exits after a
    scatter inside, 16 emitter hits later on a path that scattered inside; 1,259 frosted refractions, 383 type-6 vertices met from
    inside, 171 total internal reflections.  The model takes 16 s of CPU time."""
    sc, spec = frosted_replay_scene(api)
    seeds = frosted_replay_seeds()
    sc.upload_seeds(seeds)
    sc.iterations = FROSTED_BOUNCES
    sc.render_nee(TF.REPLAY["spp"], "mis")
    assert sc.stat("nee_family") == FAMILY
    model = frosted_replay_model(api, sc, spec)
    check_replay(sc, model, seeds, 2, NEED + ("frosted_refract", "frosted_inside"), FROSTED_BOUNCES, spp=TF.REPLAY["spp"])


# ---------------------------------------------------------------------------- 4: Beer-Lambert in closed form
SLAB = dict(z0=6.0, z1=8.5, n=1.5, W=48, H=32, spp=2, Le=(2.0, 2.0, 2.0))


def slab_spec():
    """a closed glass slab (n = 1.5, [-30, 30]^2 x [6, 8.5]) between a level camera at the origin and a grey emitter quad at z = 20, in
    a dark room (nothing else): with three segments a sample sees the emitter only straight through both faces"""
    from opencl_path_tracer_amd import scenes
    n = SLAB["n"]
    mats = [((0, 0, 0), (0, 0, 0), (0, 0, 0), (n, n, n), (0, 0, 0), 0.0, 2), ((0, 0, 0), (0, 0, 0), SLAB["Le"], (0, 0, 0), (0, 0, 0), 0.0, 3)]
    x0, y0, z0, x1, y1, z1 = -30.0, -30.0, SLAB["z0"], 30.0, 30.0, SLAB["z1"]
    c = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    tris, mo = [], []
    for a, b, cc, d in [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (3, 7, 6, 2), (0, 4, 7, 3), (1, 2, 6, 5)]:
        tris += [(c[a], c[b], c[cc]), (c[a], c[cc], c[d])]
        mo += [0, 0]
    a, b, cc, d = (-60.0, -60.0, 20.0), (60.0, -60.0, 20.0), (60.0, 60.0, 20.0), (-60.0, 60.0, 20.0)
    tris += [(a, b, cc), (a, cc, d)]
    mo += [1, 1]
    spec = scenes.SceneSpec(materials=mats, fov=60.0, shift=TL.EYE_AT_ORIGIN, name="interior_slab")
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.asarray(mo, dtype=np.uint16)))
    return spec


def test_beer_lambert_through_a_slab(api):
    """iterations = 3, absorption only: rnds are the unbound frame's, and per pixel and channel tinted / clear lies in
    [exp(-sigma_a l_max), exp(-sigma_a l_min)] (rtol 1e-5), l = (thickness - 0.001) / cos(theta_t) by Snell's law in float64 over the pixel's
    footprint (the refracted segment starts 0.001 below the front face along its normal, as every refracted segment does): the cosine to the slab's normal is D.z, smallest at one of the footprint's corners and largest at another, or 1 where
    the footprint holds the axis.  Swapping sigma_a of red and green swaps those two channels bit for bit (the lamp and the glass are
    grey)."""
    W, H, spp = SLAB["W"], SLAB["H"], SLAB["spp"]
    spec = slab_spec()
    seeds = np.random.default_rng(31).integers(1, 2 ** 31 - 2, W * H).astype(np.int32)

    def frame(sigma_a):
        sc = api.Scene(W, H).load(spec)
        if sigma_a is not None:
            sc.set_material_interior(0, sigma_a=sigma_a)
        sc.upload_seeds(seeds)
        sc.iterations = 3
        sc.render_nee(spp, "mis")
        assert sc.stat("nee_family") == (FAMILY if sigma_a is not None else 0)
        out = sc.read_colors()[:, :3].astype(np.float64), sc.read_rnds().copy(), sc.camera[0]
        sc.close()
        return out
    sa = (0.35, 0.08, 0.9)
    clear, rnds, cam = frame(None)
    tinted, rnds_t, _ = frame(sa)
    swapped, rnds_s, _ = frame((sa[1], sa[0], sa[2]))
    assert np.array_equal(rnds, rnds_t) and np.array_equal(rnds, rnds_s)
    assert same_bits(tinted[:, 0], swapped[:, 1]) and same_bits(tinted[:, 1], swapped[:, 0]) and same_bits(tinted[:, 2], swapped[:, 2])
    verts, mo = spec.objects[0]
    model = R.Model(verts, api.triangles_from_vertices(verts, mo)["N"], np.concatenate([api.Material(*m) for m in spec.materials]), mo, cam)
    thick, n = SLAB["z1"] - SLAB["z0"], SLAB["n"]
    lit = clear.min(axis=1) > 0.0
    assert lit.mean() > 0.9 and not tinted[~lit].any()
    sa32 = np.asarray(sa, dtype=np.float32).astype(np.float64)
    seen = []
    for i in np.flatnonzero(lit):
        corners = [model.camera_ray(int(i), r1, r2)[1] for r1 in (0.0, 1.0) for r2 in (0.0, 1.0)]
        cz = [float(D[2] / np.linalg.norm(D)) for D in corners]
        xs, ys = [D[0] / D[2] for D in corners], [D[1] / D[2] for D in corners]
        cmax = 1.0 if min(xs) <= 0.0 <= max(xs) and min(ys) <= 0.0 <= max(ys) else max(cz)
        ell = [(thick - 0.001) / np.sqrt(1.0 - (1.0 - c * c) / (n * n)) for c in (cmax, min(cz))]
        ratio = tinted[i] / clear[i]
        lo, hi = np.exp(-sa32 * ell[1]) * (1.0 - 1e-5), np.exp(-sa32 * ell[0]) * (1.0 + 1e-5)
        assert (ratio >= lo).all() and (ratio <= hi).all(), (i, ratio, lo, hi)
        seen.append(ell[1] / ell[0])
    assert max(seen) > 1.002                      # (the footprints at the frame's edge span lengths the bound has to follow)


# ---------------------------------------------------------------------------- 5: scattering keeps energy
def energy_scene(api, device=0):
    """slab_spec()'s glass slab alone, 2.5 thick and wider than the view, under a constant sky, with sigma_s = 0.75 and no absorption"""
    spec = slab_spec()
    verts, mo = spec.objects[0]
    spec.objects = [(verts[:12], mo[:12])]
    rgb = np.broadcast_to(ENERGY["E"], (8, 16, 3)).copy()
    sc = api.Scene(ENERGY["W"], ENERGY["H"], device=device).load(spec)
    sc.set_environment(rgb)
    sc.set_material_interior(0, sigma_s=0.75, g=0.3)
    return sc, spec, rgb


def energy_model(api, sc, spec, rgb):
    verts, mo = spec.objects[0]
    recs = api.triangles_from_vertices(verts, mo)
    return IR.InteriorModel(verts, recs["N"], np.concatenate([api.Material(*m) for m in spec.materials]), mo, sc.camera[0], None, None,
                            {0: sc.material_interior(0)}, env=dict(rgb=rgb, tables=sc.debug_environment()), table=sc.debug_light_table())


ENERGY = dict(W=48, H=32, bounces=12, E=np.asarray((0.8, 0.6, 0.4), dtype=np.float32))


def test_scattering_keeps_energy_under_a_constant_sky(api):
    """One closed glass slab (n = 1.5, a grey F0; it fills the view) under a constant sky E, sigma_a = 0, sigma_s = 0.75 (1.9 mean free
    paths across), 1 spp, 12 bounces, strategy bsdf: every factor a path takes is 1 up to rounding (F / prob and (1 - F) / (1 - prob)
    of a grey F), so a pixel is what the sky is worth at the end of a path without a diffuse vertex -- (factor_L + factor_B) E = 2 E,
    the reference's integrand, as test_gpu_medium.py's emitter is worth 2 Le cos -- within rtol 1e-5 or, where the path was cut off at
    12 segments, 0.  The share of zeros lies within five binomial standard deviations of InteriorModel's share on independent seeds
    (both shares are samples of 1,536: the variance of their difference is the sum of the two; the model's share is 0.367)."""
    W, H, bounces = ENERGY["W"], ENERGY["H"], ENERGY["bounces"]
    sc, spec, rgb = energy_scene(api)
    seeds = np.random.default_rng(41).integers(1, 2 ** 31 - 2, W * H).astype(np.int32)
    sc.upload_seeds(seeds)
    sc.iterations = bounces
    sc.render_nee(1, "bsdf")
    assert (sc.stat("nee_family"), sc.stat("nee_form")) == (FAMILY, 1)
    got = sc.read_colors()[:, :3].astype(np.float64)
    zero = ~got.any(axis=1)
    E = 2.0 * ENERGY["E"].astype(np.float64)
    print("worst deviation from 2 E: %g" % float(np.abs(got[~zero] / E - 1.0).max()))
    assert np.allclose(got[~zero], E, rtol=1e-5, atol=0.0)
    model = energy_model(api, sc, spec, rgb)
    other = np.random.default_rng(43).integers(1, 2 ** 31 - 2, W * H)
    mzero = np.asarray([not model.sample(g, int(other[g]), bounces, 0)[0].any() for g in range(W * H)])
    p, q = zero.mean(), mzero.mean()
    pool = 0.5 * (p + q)
    sd = np.sqrt(2.0 * pool * (1.0 - pool) / (W * H))
    print("truncated paths: device %.4f, model %.4f, standard deviation of the difference %.4f" % (p, q, sd))
    assert 0.01 < q < 0.6 and abs(p - q) <= 5.0 * sd


# ---------------------------------------------------------------------------- 6: the cross-check against the fog
MATCH = dict(W=96, H=64, spp=1024, few=4, frames=16, bounces=16)


def test_index_matched_box_agrees_with_bounded_fog_in_the_mean(api):
    """test_interior_host.py's box (type 2, n = 1.0005, F0 its Fresnel value 6.2e-8; CROSS there) with a grey interior against the same
    box without a boundary as bounded fog of sigma_t = sigma_a + sigma_s and albedo = sigma_s / sigma_t, under scenes.sun_and_sky(),
    strategy mis, 16 bounces.  Behind the box, in both scenes, stands a black diffuse quad that fills what the compared pixels see
    through it (the flat preview of the block is black): without it the two expectations differ by construction, because a sky miss
    on segment 0 is worth E and every later one (factor_L + factor_B) E = 2 E, and the ray that crosses unscattered misses on
    segment 0 through the fog and on segment 2 through the glass.  With it that ray is worth 0 in both, and all light arrives by
    scattering, after which a miss is worth 2 E in both.  The two estimators differ -- a factor per segment and no light sample at
    a scatter vertex against an albedo and a light sample per scatter vertex -- and have the same expectation up to the bending of a
    ray at the boundary, which the host-side run of the two models (test_premise_of_the_cross_check_against_the_fog) shows below its
    standard error at this n.
    Compared: the mean luminance over the 24 x 16 block of pixels that sees the box, 1,024 samples per pixel.  The per-sample deviation
    is taken from the frames themselves at a few samples per pixel, as test_gpu_medium.py's airlight test takes its own from four
    samples per pixel: 16 frames of 4 samples each on seeds of their own, the deviation of their pixels pooled over the block (a mean
    of 4 independent samples: times 2), and the standard error is that over sqrt(384 x 1,024).  The interior reaches the sun only
    through the phase function (the stated limitation), so its deviation is many times its mean: hence the sample count.  The means
    agree within five combined standard errors.  Measured on these seeds: interior 0.92870 (per-sample deviation 17.7, standard error
    0.0283), fog 0.91401 (deviation 1.0, standard error 0.0016): 0.5 combined standard errors apart.  (Without the backdrop the same
    run read 1.23329 against 1.12507: the unscattered ray's E exp(-sigma_t l) of difference, about 0.10 for this block.)"""
    from opencl_path_tracer_amd import scenes
    W, H, C = MATCH["W"], MATCH["H"], TH.CROSS
    backdrop = np.asarray([((-2.0, -2.0, 8.0), (2.0, 2.0, 8.0), (2.0, -2.0, 8.0)), ((-2.0, -2.0, 8.0), (-2.0, 2.0, 8.0), (2.0, 2.0, 8.0))], dtype=np.float32)

    def with_backdrop(spec, shift):
        verts, mo = spec.objects[0]
        spec.materials.append(((0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0))      # black, diffuse
        black = len(spec.materials) - 1
        spec.objects = [(np.concatenate([verts[:12] + np.float32(shift), backdrop]), np.concatenate([mo[:12], np.full(2, black, dtype=np.uint16)]))]
        return spec
    glass = with_backdrop(TH.box_spec(C["n"]), 0.0)              # the box and the backdrop: the sky lights them
    far = with_backdrop(TH.box_spec(C["n"]), 1000.0)             # the same box out of sight: the fog stands alone in front of the backdrop
    sig_t = C["sigma_a"] + C["sigma_s"]
    rgb = scenes.sun_and_sky()
    block = (slice(3 * H // 8, 5 * H // 8), slice(3 * W // 8, 5 * W // 8))
    npix = (H // 4) * (W // 4)
    rng = np.random.default_rng(61)

    def luminance(sc):
        c = sc.read_colors()[:, :3].astype(np.float64).reshape(H, W, 3)[block].reshape(-1, 3)
        return 0.2126 * c[:, 0] + 0.7152 * c[:, 1] + 0.0722 * c[:, 2]
    mean, se = {}, {}
    for name, spec in (("interior", glass), ("fog", far)):
        sc = api.Scene(W, H).load(spec)
        sc.set_environment(rgb)
        if name == "fog":                          # the flat preview: no compared pixel sees the sky past the backdrop
            sc.iterations = 1
            sc.render_nee(1, "mis")
            assert not luminance(sc).any() and sc.read_colors()[0, :3].any()
        if name == "interior":
            sc.set_material_interior(0, sigma_a=C["sigma_a"], sigma_s=C["sigma_s"], g=C["g"])
        else:
            sc.set_medium(sig_t, albedo=C["sigma_s"] / sig_t, g=C["g"], bounds=((-1.0, -1.0, 4.0), (1.0, 1.0, 6.0)))
        sc.iterations = MATCH["bounces"]
        few = []
        for _ in range(MATCH["frames"]):
            sc.current_sample = 0
            sc.upload_seeds(rng.integers(1, 2 ** 31 - 2, W * H).astype(np.int32))
            sc.render_nee(MATCH["few"], "mis")
            few.append(luminance(sc))
        assert len(few[0]) == npix
        sd = np.sqrt(MATCH["few"]) * float(np.concatenate(few).std(ddof=1))
        sc.current_sample = 0
        sc.upload_seeds(rng.integers(1, 2 ** 31 - 2, W * H).astype(np.int32))
        sc.render_nee(MATCH["spp"], "mis")
        assert int(sc.stat("nee_family")) == (FAMILY if name == "interior" else 8)
        mean[name] = float(luminance(sc).mean())
        se[name] = sd / np.sqrt(npix * MATCH["spp"])
        print("%s: block mean luminance %.5f, per-sample deviation %.3f, standard error %.5f" % (name, mean[name], sd, se[name]))
        sc.close()
    both = float(np.hypot(se["interior"], se["fog"]))
    print("difference %.5f, combined standard error %.5f" % (mean["interior"] - mean["fog"], both))
    assert mean["fog"] > 0.0 and both < 0.1 * mean["fog"] and abs(mean["interior"] - mean["fog"]) <= 5.0 * both


# ---------------------------------------------------------------------------- 7: the instances
WAX = dict(sigma_a=(2e-3, 5e-4, 1e-4), sigma_s=5e-3, g=0.7)          # the spheres of the small scene have diameter 400: two mean free paths


def block_of(form, mode):
    return I.block_of(8, form, mode)              # kWideAll, as the medium family's


@pytest.mark.parametrize("form", range(4), ids=I.FORMS)
def test_node_modes_render_the_same_bits(api, form):
    """tests/test_gpu_nee_instances.py's equalities for the sixteen new instances, every feature and the fog live and WAX bound to the glass
    materials: small scene, mode 0 = 1 = 3 = 3 with the stack overflowing; mesh, mode 1 = 2 = 3; the stats are the cell's; the frame
    is not the unbound one."""
    differs = []
    for scene, first in (("small", "lds"), ("mesh", "treelet")):
        spec = I.scene_spec(scene, True, True)
        frames, thr = {}, None
        for placement in I.PLACEMENTS[scene]:
            sc, mode = I.build(api, scene, "medium", placement, sky=bool(form & 1))
            bind(sc, spec, **WAX)
            if form & 2 and thr is None:
                sc.iterations = TL.CB_BOUNCES
                thr = TI.threshold_of(sc)
            frames[placement] = TI.render(sc, form, thr)
            got = tuple(int(sc.stat(k)) for k in ("node_mode", "nee_family", "nee_form", "nee_block"))
            assert got == (mode, FAMILY, form, block_of(form, mode)), (scene, placement, got)
            sc.close()
        want = frames[first]
        assert np.isfinite(want[0]).all() and want[0][:, :3].mean() > 0.0
        for placement, got in frames.items():
            assert TI.same_frames(got, want), (I.FORMS[form], scene, placement)
        differs.append(not same_bits(want[0], TI.reference_frame(api, scene, "medium", form)))
    assert all(differs), differs


# ---------------------------------------------------------------------------- 8: adaptive and tiled
def wax_box(api, W, H, sky=False, **kw):
    from opencl_path_tracer_amd import scenes
    sc = api.Scene(W, H, **kw).load(scenes.cornell_box(fog=1.5e-3, tint=(0.9, 0.5, 0.2), wax=2.0))
    if sky:
        sc.set_environment(scenes.sun_and_sky())
    sc.set_lights([TL.box_light(api)], select=0.4)
    sc.iterations = TL.CB_BOUNCES
    return sc


@pytest.mark.parametrize("sky", [False, True])
def test_adaptive_nee_tiles_hold_render_nee_bits(api, sky):
    """k_nee_tiles_interior / k_nee_env_tiles_interior against k_nee_interior / k_nee_env_interior at 36 x 20 (ragged tiles), as
    test_gpu_medium.py's"""
    W, H = 36, 20
    sc = wax_box(api, W, H, sky)
    sc.render_adaptive(4, 16, 0.0, metric="half", path="nee", strategy="mis")
    thr = float(np.median(sc.tile_state()[1]))
    assert np.isfinite(thr) and thr > 0.0
    sc.current_sample = 0
    sc.seed_default()
    sc.render_adaptive(4, 16, thr, metric="half", path="nee", strategy="mis")
    assert (sc.stat("nee_family"), sc.stat("nee_form")) == (FAMILY, 2 | int(sky))
    counts = sc.sample_counts().reshape(-1)
    cols, rnds = sc.read_colors(), sc.read_rnds()
    seen = sorted(set(int(c) for c in np.unique(counts)))
    assert set(seen) <= {4, 8, 16} and len(seen) >= 2, seen
    for k in seen:
        fresh = wax_box(api, W, H, sky)
        fresh.render_nee(k, "mis")
        sel = counts == k
        assert same_bits(cols[sel, :3], fresh.read_colors()[sel, :3]) and np.array_equal(rnds[sel], fresh.read_rnds()[sel]), k


def test_tiled_ranks_assemble_the_single_context_frame(api):
    W, H, world = 48, 36, 2
    one = wax_box(api, W, H)
    one.render_nee(3, "mis")
    whole = state(one)
    clear = wax_box(api, W, H)
    clear.clear_material_interiors()
    clear.render_nee(3, "mis")
    assert clear.stat("nee_family") == 8 and not same_bits(whole[0], clear.read_colors())       # (the interior shows)
    seen = np.zeros(W * H, dtype=bool)
    for r in range(world):
        sc = wax_box(api, W, H, rank=r, world=world, rows_per_block=8)
        sc.render_nee(3, "mis")
        ids = sc.local_pixel_ids()
        assert same_state(state(sc), tuple(a[ids] for a in whole)), r
        seen[ids] = True
    assert seen.all()


# ---------------------------------------------------------------------------- 9: a binding that does not count
def test_a_binding_on_a_diffuse_material_is_ignored(api):
    """slab_spec()'s glass slab with a white diffuse quad embedded in it (z = 7.2, smaller than the view): paths inside the glass end on the
    quad while `inside` is true, and its diffuse bounce leaves through the front face to a constant sky.  A strongly absorbing, scattering interior bound to the quad's material -- type 0 -- takes family 10 and
    leaves every bit of the unbound frame: the device table holds `bound` only for types 2 and 6.  Bound to the glass as well, the
    frame changes."""
    from opencl_path_tracer_amd import scenes
    spec = slab_spec()
    spec.materials.append(scenes.BUILTIN_MATERIALS[scenes.WHITE_DIFFUSE])
    quad = np.asarray([((-1.5, -1.0, 7.2), (1.5, -1.0, 7.2), (1.5, 1.0, 7.2)), ((-1.5, -1.0, 7.2), (1.5, 1.0, 7.2), (-1.5, 1.0, 7.2))], dtype=np.float32)
    spec.objects.append((quad, np.full(2, 2, dtype=np.uint16)))
    W, H = SLAB["W"], SLAB["H"]
    frames = []
    for bound in ((), (2,), (2, 0)):
        sc = api.Scene(W, H).load(spec)
        sc.set_environment(np.full((8, 16, 3), 0.7, dtype=np.float32))
        for m in bound:
            sc.set_material_interior(m, sigma_a=(5.0, 3.0, 1.0), sigma_s=2.0, g=0.2)
        sc.iterations = 6
        sc.render_nee(4, "mis")
        assert sc.stat("nee_family") == (FAMILY if bound else 0) and sc.stat("nee_form") == 1
        frames.append(state(sc))
        sc.close()
    centre = frames[0][0].reshape(H, W, 4)[H // 2, W // 2, :3]
    assert centre.min() > 0.0                              # the quad is lit by the sky, through the glass
    assert same_state(frames[1], frames[0]) and not same_bits(frames[2][0], frames[0][0])
