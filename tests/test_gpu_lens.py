"""-m gpu: the thin-lens camera of Scene.set_lens in Scene.render_nee and Scene.render_adaptive(path="nee") (the lens instances of k_nee in
pt_nee.hip, k_debug_lens and k_focus_at of pt_lens.hip; include/pt_api.h pins the lens ray).

  1 the device function (Scene.debug_lens) against tests/lens_ref.py's float64 statement; 2 aperture 0 and clear_lens change no bit;
  3 a wall in the focal plane is imaged as by the pinhole; 4 an edge off the focal plane is blurred by the closed-form disc;
  5 a constant sky stays constant; 6 MIS frames of scenes.focus_row() against the float64 model with the lens mixin;
  7 adaptive NEE tiles hold render_nee's bits under the lens; 8 focus_at; 9 determinism."""

import numpy as np
import pytest

import coated_ref as K
import lens_ref as L
import nee_ref as R
import test_gpu_glossy as TG

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = 36, 20
BOUNCES = 4
same_bits, state, same_state = TG.same_bits, TG.state, TG.same_state


class LensModel(L.LensMixin, K.CoatedModel):
    """coated_ref.CoatedModel (glossy = coated = False and no vertex normals: nee_ref.Model's estimator with the glass vertex and inert
    types 4 and 5) seen through the lens"""


def grey(kd):
    return ((kd, kd, kd), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0)


def wall_spec(dist, xs, ys, kds):
    """A wall perpendicular to the optical axis of the default view (eye (500, 500, -1299.037842), looking along +z) at axial distance
    dist: patches between the boundaries xs and ys (wall coordinates relative to the axis), patch (j, i) grey kds[j][i]"""
    from opencl_path_tracer_amd import scenes
    ex, ey, ez = 500.0, 500.0, float(F32(-1299.037842))
    z = ez + dist
    mats, tris, mo = [], [], []
    for j in range(len(ys) - 1):
        for i in range(len(xs) - 1):
            a, b, c, d = ((ex + xs[i], ey + ys[j], z), (ex + xs[i + 1], ey + ys[j], z), (ex + xs[i + 1], ey + ys[j + 1], z), (ex + xs[i], ey + ys[j + 1], z))
            tris += TG.quad(a, b, c, d)
            mo += [len(mats)] * 2
            mats.append(grey(kds[j][i]))
    spec = scenes.SceneSpec(materials=mats, name="lens_wall")
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.asarray(mo, dtype=np.uint16)))
    return spec


def ahead_length(cam):
    """|lookat - eye| of the default view, in pixels: a pixel's footprint at axial distance z is z / ahead_length wide"""
    return float(cam["lookat"][0, 2]) - float(cam["eye"][0, 2])


def frame(api, spec, lens, spp, iterations=1, strategy="mis", sky=None):
    sc = api.Scene(W, H).load(spec)
    if sky is not None:
        sc.set_environment(sky)
    if lens is not None:
        sc.set_lens(*lens)
    sc.iterations = iterations
    sc.render_nee(spp, strategy)
    out = state(sc)
    sc.close()
    return out


# ---------------------------------------------------------------------------- 1: the device function
def lens_items():
    """4,096 items: the 720 pixels of a 36 x 20 frame in turn, each with its own LCG state (a multiplicative sequence over [1, 2^31 - 2])"""
    k = np.arange(4096, dtype=np.int64)
    gid = (k * 7) % (W * H)
    S = (12345 + k * 524287 * 4093) % (R.M31 - 1) + 1
    return np.stack([gid, S], 1).astype(np.int32)


LENSES = [(3.0, 20.0), (40.0, 20.0), (3.0, 1000.0), (40.0, 1000.0)]       # |lookat - eye| = 31.2: a focus distance on either side of it


def test_device_function_matches_float64(api):
    """Scene.debug_lens against lens_ref.lens_rays in float64, for a view with yaw 20 and pitch -10 from the default eye.  Errors of P and
    of D as vectors, relative to the wanted vector's length.  Bound: 4 x the largest error of the float32 restatement (lens_rays with
    dtype float32, numpy without fma) on the same items, never below 4 x 2^-24.  Measured on the CPU, restatement against float64,
    largest error of (P, D) per lens (aperture, focus distance):
      (3, 20) 8.3e-08, 6.9e-06   (40, 20) 8.5e-08, 6.2e-06   (3, 1000) 8.3e-08, 3.1e-06   (40, 1000) 8.5e-08, 3.1e-06
    (D carries the cancellation in Q - O: coordinates near 1,300 with half an ulp of 6e-5 each against a difference of 20 or 1,000; the
    restatement's own Q lies 1.1e-4 / 3.5e-3 off its ray at focus distance 20 / 1,000).  The distance of the float64 point in focus Q
    from the device's ray must stay within the same bound (of D) times the focus distance: 5e-4 / 1.2e-2.
    Measured on the device: see profiles/lens/README.md."""
    items = lens_items()
    sc = api.Scene(W, H)
    sc.set_view(60.0, 20.0, -10.0, (0.0, 0.0, 0.0))
    cam = sc.camera[0]
    for a, F in LENSES:
        P, D, Q = L.lens_rays(cam, a, F, items[:, 0], items[:, 1])
        lowP, lowD, _ = L.lens_rays(cam, a, F, items[:, 0], items[:, 1], dtype=np.float32)
        cpu = L.ray_errors(np.concatenate([lowP, lowD], 1), P, D).max(axis=0)
        bound = 4.0 * np.maximum(cpu, 2.0 ** -24)
        got = sc.debug_lens(a, F, items)
        assert np.isfinite(got).all()
        err = L.ray_errors(got, P, D).max(axis=0)
        dist = float(L.distance_to_ray(Q, got[:, :3].astype(np.float64), got[:, 3:6].astype(np.float64)).max())
        print("lens (%g, %g): float32 model vs float64 P %.3g D %.3g; device vs float64 P %.3g D %.3g; Q off the device's ray by %.3g (bound %.3g)"
              % (a, F, cpu[0], cpu[1], err[0], err[1], dist, bound[1] * F))
        assert (err <= bound).all(), (a, F, err, bound)
        assert dist <= bound[1] * F, (a, F, dist)
        assert np.abs(np.linalg.norm(got[:, 3:6].astype(np.float64), axis=1) - 1.0).max() < 1e-6
    sc.close()


# ---------------------------------------------------------------------------- 2: no lens, no change
def test_noops_are_bit_exact(api, cb_spec):
    def nee(touch):
        sc = api.Scene(W, H).load(cb_spec)
        touch(sc)
        sc.iterations = BOUNCES
        sc.render_nee(4, "mis")
        return sc, state(sc)

    def adaptive(touch):
        sc = api.Scene(W, H).load(cb_spec)
        touch(sc)
        sc.iterations = BOUNCES
        sc.render_adaptive(4, 8, 0.05, metric="half", path="nee", strategy="mis")
        return sc, state(sc)

    def set_and_clear(sc):
        sc.set_lens(25.0, 1500.0)
        sc.clear_lens()

    for run in (nee, adaptive):
        plain, want = run(lambda sc: None)
        plain.close()
        for touch in (lambda sc: sc.set_lens(0.0, 1500.0), set_and_clear):
            sc, got = run(touch)
            assert same_state(got, want), run.__name__
            sc.current_sample = 0
            sc.render(1)                       # pt_render works again
            sc.close()
        sc, lens = run(lambda sc: sc.set_lens(25.0, 1500.0))
        assert not same_bits(lens[0], want[0]), run.__name__
        with pytest.raises(api.PtError) as e:
            sc.current_sample = 0
            sc.render(1)
        assert e.value.code == api.PT_EINVAL and "pt_clear_lens" in str(e.value)
        sc.close()


# ---------------------------------------------------------------------------- 3: the focal plane
FOCAL = 1000.0
PATCH_KD = [[0.2, 0.4], [0.6, 0.8]]


def focal_wall(cam):
    """the 2 x 2 wall at axial distance FOCAL, split through the middle of pixel column 18 and of pixel row 10, and the mask of the pixels
    whose whole footprint (from the pinhole geometry) lies inside one patch, with a margin of 1e-3 pixels"""
    s = FOCAL / ahead_length(cam)                                  # a pixel's footprint
    big = 40.0 * s
    spec = wall_spec(FOCAL, [-big, 0.5 * s, big], [-big, 0.5 * s, big], PATCH_KD)
    x0, y0 = (np.arange(W) - W / 2.0) * s, (np.arange(H) - H / 2.0) * s
    clear_x = (x0 + s < 0.5 * s - 1e-3 * s) | (x0 > 0.5 * s + 1e-3 * s)
    clear_y = (y0 + s < 0.5 * s - 1e-3 * s) | (y0 > 0.5 * s + 1e-3 * s)
    return spec, (clear_y[:, None] & clear_x[None, :]).reshape(-1)


def test_a_wall_in_the_focal_plane_is_imaged_as_by_the_pinhole(api):
    cam = api.Camera(60.0, 0.0, 0.0, (0.0, 0.0, 0.0), W, H)
    spec, whole = focal_wall(cam)
    assert whole.mean() >= 0.8
    pin = frame(api, spec, None, 16)[0][:, :3].astype(np.float64)
    lens = frame(api, spec, (0.2 * FOCAL, FOCAL), 16)[0][:, :3].astype(np.float64)
    assert len({round(float(v), 6) for v in pin[whole, 0]}) == 4                # the four patches are seen
    rel = np.abs(lens[whole] - pin[whole]) / pin[whole]
    print("pixels inside one patch: %.1f %%; largest relative difference there %.3g; pixels that differ elsewhere: %d"
          % (100.0 * whole.mean(), rel.max(), int((lens[~whole] != pin[~whole]).any(axis=1).sum())))
    assert rel.max() <= 1e-6
    # and off the focal plane the same lens does blur the patch boundaries
    off = frame(api, spec, (0.2 * FOCAL, 0.5 * FOCAL), 16)[0][:, :3].astype(np.float64)
    assert (np.abs(off[whole] - pin[whole]) / pin[whole]).max() > 1e-2


# ---------------------------------------------------------------------------- 4: the circle of confusion
def disc_edge(u, Rr):
    """P(x + dx > 0) for dx uniform on a disc of radius Rr, at signed distance u of x from the edge: 1/2 + (u sqrt(R^2 - u^2) + R^2 asin(u / R)) / (pi R^2)"""
    c = np.clip(u, -Rr, Rr)
    return 0.5 + (c * np.sqrt(Rr * Rr - c * c) + Rr * Rr * np.arcsin(c / Rr)) / (np.pi * Rr * Rr)


def expected_columns(s, Rr, n=64):
    """per pixel column, the mean of disc_edge over the column's footprint [s (c - W/2), s (c + 1 - W/2)]: Gauss-Legendre, float64"""
    x, w = np.polynomial.legendre.leggauss(n)
    lo = (np.arange(W) - W / 2.0) * s
    u = lo[:, None] + (0.5 * (x + 1.0))[None, :] * s
    return (disc_edge(u, Rr) * (0.5 * w)[None, :]).sum(axis=1)


@pytest.mark.parametrize("ratio", [2.0, 0.5])
def test_an_edge_off_the_focal_plane_is_blurred_by_the_disc(api, ratio):
    """A black / white edge on the optical axis (the boundary of pixel columns 17 and 18) at axial distance z = ratio x F, iterations = 1
    (the preview colour: 0 or 1 per sample), 64 spp.  A thin lens moves the pinhole's wall point by the lens offset times (1 - z / F):
    uniform on a disc of radius aperture |1 - z / F|.  The aperture makes that disc 3 pixel footprints wide at z = 2 F (the blur spans
    columns 15 to 20) and 6 at z = F / 2 (columns 12 to 23), whole footprints, so no column has a probability that is tiny but not 0.
    Each sample is a Bernoulli draw with the column's expected value p: the column mean over 20 rows x 64 samples lies within four
    standard errors sqrt(p (1 - p) / 1280) of p (plus 64 x 2^-24 for the float32 running mean)."""
    cam = api.Camera(60.0, 0.0, 0.0, (0.0, 0.0, 0.0), W, H)
    A = ahead_length(cam)
    F = 400.0
    z = ratio * F
    aperture = 6.0 * F / A
    s = z / A
    Rr = aperture * abs(1.0 - z / F)
    assert abs(Rr / s - (3.0 if ratio == 2.0 else 6.0)) < 1e-9
    spp = 64
    big = 60.0 * s
    spec = wall_spec(z, [-big, 0.0, big], [-big, big], [[0.0, 1.0]])
    want = expected_columns(s, Rr)
    assert ((want > 1e-9) & (want < 1.0 - 1e-9)).sum() >= 6
    got = frame(api, spec, (aperture, F), spp)[0][:, 0].astype(np.float64).reshape(H, W).mean(axis=0)
    se = np.sqrt(want * (1.0 - want) / (H * spp))
    z_score = np.abs(got - want) / np.maximum(se, 1e-12)
    print("columns (expected, rendered):", [(round(float(a), 4), round(float(b), 4)) for a, b in zip(want, got) if 0 < a < 1])
    print("largest |rendered - expected| / standard error over the blurred columns: %.2f" % float(z_score[se > 0].max()))
    assert (np.abs(got - want) <= 4.0 * se + 64 * 2.0 ** -24).all(), (got, want)
    pin = frame(api, spec, None, spp)[0][:, 0].astype(np.float64).reshape(H, W).mean(axis=0)
    assert np.array_equal(pin, (np.arange(W) >= W // 2).astype(np.float64))           # the pinhole's edge is sharp


# ---------------------------------------------------------------------------- 5: a constant sky
def behind_spec():
    """no geometry in view: one small triangle behind the camera, which no ray that leaves the lens forwards can meet"""
    from opencl_path_tracer_amd import scenes
    spec = scenes.SceneSpec(materials=[grey(0.5)], name="lens_sky")
    tri = [((490.0, 490.0, -1500.0), (510.0, 490.0, -1500.0), (500.0, 510.0, -1500.0))]
    spec.objects.append((np.asarray(tri, dtype=np.float32), np.zeros(1, dtype=np.uint16)))
    return spec


def test_a_constant_sky_stays_constant(api):
    sky = np.full((1, 1, 3), (0.25, 0.5, 0.75), dtype=np.float32)
    pin = frame(api, behind_spec(), None, 4, BOUNCES, sky=sky)
    lens = frame(api, behind_spec(), (30.0, 500.0), 4, BOUNCES, sky=sky)
    assert same_bits(lens[0], pin[0]) and np.array_equal(lens[1], pin[1])
    assert (pin[0][:, :3] == np.asarray([0.25, 0.5, 0.75], dtype=F32)).all()
    assert not same_bits(lens[3], pin[3])                                  # the rays are the lens's


# ---------------------------------------------------------------------------- 6: the float64 model
REPLAY = dict(W=32, H=24, spp=4, bounces=4, lens=(0.35, 9.0))
CONFIGS = {"on": dict(options=1, sky=False), "off": dict(options=0, sky=False), "sky": dict(options=1, sky=True)}


def replay_seeds():
    return np.random.default_rng(29).integers(1, 2 ** 31 - 2, REPLAY["W"] * REPLAY["H"]).astype(np.int32)


def replay_model(api, cam, spec, on, env=None, table=None):
    verts = np.concatenate([v for v, _ in spec.objects])
    mo = np.concatenate([m for _, m in spec.objects])
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    vn = np.concatenate([np.zeros(v.shape, dtype=np.float32) if n is None or not on else n for (v, _), n in zip(spec.objects, spec.normals)])
    m = LensModel(verts, recs["N"], mats, mo, cam, vn, env=env, table=table, glossy=bool(on), coated=bool(on))
    return m.set_lens(*REPLAY["lens"])


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_mis_matches_float64_model(api, config):
    """scenes.focus_row() (a type-0, a glass, a type-4 and a type-5 sphere) through a lens of radius 0.35 focused at 9, 32 x 24, 4 spp, 4
    bounces, MIS, from uploaded seeds.  "on": smooth_normals, textures (none bound), glossy and coated on; "off": all off, types 4 and 5
    inert; "sky": on, under scenes.sun_and_sky().  Tolerance 2e-3 |want| + 1e-6 scale, the existing replays'; rnds equal.  Near-tie share
    of the model alone on these seeds, measured on the CPU before the first GPU run (light table in add order, the sky's tables from
    env_ref.tables): on 0.26 %, off 0.13 %, sky 2.34 % (cap 10 %); the kept pixels of "on" hold 77 type-4 and 21 type-5 vertices."""
    from opencl_path_tracer_amd import scenes
    Wr, Hr, spp, bounces = REPLAY["W"], REPLAY["H"], REPLAY["spp"], REPLAY["bounces"]
    cfg = CONFIGS[config]
    spec = scenes.focus_row()
    sc = api.Scene(Wr, Hr).load(spec)
    env = None
    if cfg["sky"]:
        rgb = scenes.sun_and_sky()
        sc.set_environment(rgb)
        env = dict(rgb=rgb, tables=sc.debug_environment())
    for opt in ("smooth_normals", "textures", "glossy", "coated"):
        sc.set_option(opt, cfg["options"])
    sc.set_lens(*REPLAY["lens"])
    seeds = replay_seeds()
    sc.upload_seeds(seeds)
    sc.iterations = bounces
    sc.render_nee(spp, "mis")
    model = replay_model(api, sc.camera[0], spec, cfg["options"], env, table=sc.debug_light_table())
    want, want_seeds, ties = model.render(seeds, bounces, spp, 2)
    got = sc.read_colors()[:, :3].astype(np.float64)
    keep = ~ties
    print("%s: kept share %.3f; events in the kept pixels: %s" % (config, keep.mean(), {k: int(v[keep].sum()) for k, v in model.pixel_events.items()}))
    assert keep.mean() > 0.9, "too many near-tie pixels: %d" % int(ties.sum())
    assert np.array_equal(sc.read_rnds()[keep], want_seeds[keep])
    scale = float(want[keep].max())
    err = np.abs(got[keep] - want[keep])
    tol = 2e-3 * np.abs(want[keep]) + 1e-6 * scale
    print("worst error / bound: %.3g" % float((err / tol).max()))
    assert not (err > tol).any(), "%d of %d pixel channels differ" % (int((err > tol).sum()), err.size)
    assert float(want[keep].mean()) > 0.0
    if cfg["options"]:
        for name in ("glossy_vertex", "coated_coat", "coated_base"):
            assert int(model.pixel_events[name][keep].sum()) > 0, name
    # the lens is not a no-op here: the pinhole frame of the same seeds differs
    sc.clear_lens()
    sc.current_sample = 0
    sc.upload_seeds(seeds)
    sc.render_nee(spp, "mis")
    assert not same_bits(sc.read_colors()[:, :3], got.astype(F32))
    sc.close()


# ---------------------------------------------------------------------------- 7: adaptive NEE frames
@pytest.mark.parametrize("sky,opts,mode", [(False, {}, 0), (True, {}, 0), (True, {"wide_nodes": 2}, 3)])
def test_adaptive_nee_tiles_hold_render_nee_bits(api, sky, opts, mode):
    """k_nee_tiles_lens / k_nee_env_tiles_lens against k_nee_lens / k_nee_env_lens on scenes.focus_row(), 36 x 20: ragged tiles on the
    right and at the bottom"""
    from opencl_path_tracer_amd import scenes
    spec = scenes.focus_row()

    def scene(lens=True):
        c = api.Scene(W, H)
        for k, v in opts.items():
            c.set_option(k, v)
        c.load(spec)
        assert c.stat("node_mode") == mode
        if sky:
            c.set_environment(scenes.sun_and_sky())
        for opt in ("smooth_normals", "glossy", "coated"):
            c.set_option(opt, 1)
        if lens:
            c.set_lens(*REPLAY["lens"])
        c.iterations = BOUNCES
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
        fresh.close()
    pin = scene(lens=False)
    pin.render_nee(16, "mis")
    sel = counts == 16
    assert not same_bits(cols[sel, :3], pin.read_colors()[sel, :3])
    pin.close()
    sc.close()


# ---------------------------------------------------------------------------- 8: autofocus
def test_focus_at(api):
    cam = api.Camera(60.0, 0.0, 0.0, (0.0, 0.0, 0.0), W, H)
    spec, whole = focal_wall(cam)
    sc = api.Scene(W, H).load(spec)
    found = {xy: sc.focus_at(*xy) for xy in ((W // 2, H // 2), (0, 0), (W - 1, H - 1))}
    print("focus_at on the wall at %g: %s" % (FOCAL, found))
    for xy, d in found.items():
        assert abs(d - FOCAL) <= 1e-5 * FOCAL, xy
    for bad in ((-1, 0), (W, 0), (0, H)):
        with pytest.raises(api.PtError) as e:
            sc.focus_at(*bad)
        assert e.value.code == api.PT_EINVAL
    # focusing there and rendering reproduces the focal-plane equality
    sc.iterations = 1
    sc.render_nee(16, "mis")
    pin = sc.read_colors()[:, :3].astype(np.float64)
    sc.set_lens(0.2 * FOCAL, found[(0, 0)])
    sc.current_sample = 0
    sc.seed_default()
    sc.render_nee(16, "mis")
    lens = sc.read_colors()[:, :3].astype(np.float64)
    assert (np.abs(lens[whole] - pin[whole]) / pin[whole]).max() <= 1e-6
    sc.close()
    miss = api.Scene(W, H).load(behind_spec())
    assert miss.focus_at(W // 2, H // 2) == float("inf")
    miss.close()


# ---------------------------------------------------------------------------- 9: determinism
def test_determinism(api):
    from opencl_path_tracer_amd import scenes
    spec = scenes.focus_row()

    def scene():
        c = api.Scene(W, H).load(spec)
        c.set_environment(scenes.sun_and_sky())
        for opt in ("smooth_normals", "glossy", "coated"):
            c.set_option(opt, 1)
        c.set_lens(*REPLAY["lens"])
        c.iterations = BOUNCES
        return c
    a, b = scene(), scene()
    a.render_nee(4, "mis")
    a.render_nee(4, "mis")
    b.render_nee(8, "mis")
    assert same_state(state(a), state(b))
    a.close()
    b.close()
