"""-m gpu: environment lighting in Scene.render_nee (pt_set_environment, k_nee_env in pt_nee.hip; include/pt_api.h pins it).

  * without a sky (never set, set and cleared, or all zero) render_nee computes the bits it computed before;
  * the three strategies against tests/env_ref.py (float64, brute force, same LCG and hashes) on a scene of 13 triangles;
  * closed forms under a constant and a half-lit sky, the same mean in every strategy, lower RMSE with MIS;
  * rnds / rays are pt_render's, determinism, the flat preview, tiled ranks, the refusals of the other render paths, and the
    variance / guide / denoise / temporal passes on a sky-lit frame."""

import numpy as np
import pytest

import env_ref as E

pytestmark = pytest.mark.gpu

STRATEGIES = ("bsdf", "light", "mis")
CB_BOUNCES = 8
EYE_AT_ORIGIN = (-500.0, -500.0, 1299.0378)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def state(sc):
    rays = sc.read_rays()
    return sc.read_colors().copy(), sc.read_rnds().copy(), rays["P"][:, :3].copy(), rays["D"][:, :3].copy()


def same_state(a, b):
    return same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2]) and same_bits(a[3], b[3])


def open_box_spec(lamp=False):
    """The Cornell box without its ceiling (and without its lamp): the spheres under an open sky."""
    from opencl_path_tracer_amd import scenes
    spec = scenes.cornell_box()
    verts, mati = spec.objects[0]
    keep = np.ones(len(verts), dtype=bool)
    keep[8:10] = False                      # ceiling
    if not lamp:
        keep[0:2] = False
    spec.objects[0] = (verts[keep], mati[keep])
    spec.name = "open_box"
    return spec


def hot_texel_map(w=64, h=32, row=8, col=20):
    rgb = np.full((h, w, 3), 0.02, dtype=np.float32)
    rgb[row, col] = (3000.0, 2700.0, 2200.0)
    t = E.luminance(rgb) * E.solid_angles(w, h)[:, None]
    assert t[row, col] / t.sum() >= 0.9
    return rgb


# ---------------------------------------------------------------------------- 1: no change without a sky
def test_no_sky_no_change(api, cb_spec):
    from opencl_path_tracer_amd import scenes
    W, H = 48, 40
    for strategy in STRATEGIES:
        fresh = api.Scene(W, H).load(cb_spec)
        fresh.iterations = CB_BOUNCES
        fresh.render_nee(3, strategy)
        want = state(fresh)
        cleared = api.Scene(W, H).load(cb_spec)
        cleared.set_environment(scenes.sun_and_sky())
        cleared.clear_environment()
        zero = api.Scene(W, H).load(cb_spec)
        zero.set_environment(np.zeros((8, 16, 3), dtype=np.float32))
        for sc in (cleared, zero):
            sc.iterations = CB_BOUNCES
            sc.render_nee(3, strategy)
            assert same_state(state(sc), want), strategy
        lit = api.Scene(W, H).load(cb_spec)          # and a sky does change the frame
        lit.set_environment(scenes.sun_and_sky())
        lit.iterations = CB_BOUNCES
        lit.render_nee(3, strategy)
        assert not same_bits(lit.read_colors(), want[0])


# ---------------------------------------------------------------------------- 2: replay against the float64 model
def replay_spec():
    """A box with an open top: glossy floor, three walls, an occluder, a mirror and one emitting triangle (13 triangles)."""
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
    spec = scenes.SceneSpec(materials=mats, name="env_replay", shift=EYE_AT_ORIGIN)
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.asarray(mo, dtype=np.uint16)))
    assert spec.ntris <= 20
    return spec


def replay_map():
    """16 x 8: a dim gradient and one hot texel in the upper hemisphere"""
    h, w = 8, 16
    rgb = np.zeros((h, w, 3), dtype=np.float32)
    rgb[...] = (0.05 + 0.3 * (np.arange(h)[:, None] / h) + 0.1 * (np.arange(w)[None, :] / w))[..., None] * np.array([0.8, 0.9, 1.0])
    rgb[1, 5] = (60.0, 50.0, 40.0)
    return rgb


REPLAY = dict(W=48, H=32, spp=2, bounces=4, scale=1.25, yaw_degrees=25.0, select=0.5)


def replay_model(api, sc, spec, rgb):
    verts, mo = spec.objects[0]
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    return E.EnvModel(verts, recs["N"], mats, mo, sc.camera[0], rgb, sc.debug_environment(), scale=REPLAY["scale"],
                      yaw_degrees=REPLAY["yaw_degrees"], table=sc.debug_light_table())


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_matches_float64_model(api, strategy):
    """The model alone, on these seeds, flags 0.3 % / 0.6 % / 0.6 % of the pixels as near-ties in bsdf / light / mis (measured on the
    CPU before the first GPU run): far below the 10 % cap."""
    W, H, spp, bounces = REPLAY["W"], REPLAY["H"], REPLAY["spp"], REPLAY["bounces"]
    spec, rgb = replay_spec(), replay_map()
    sc = api.Scene(W, H).load(spec)
    sc.set_environment(rgb, scale=REPLAY["scale"], yaw_degrees=REPLAY["yaw_degrees"], select=REPLAY["select"])
    seeds = np.random.default_rng(17).integers(1, 2 ** 31 - 2, W * H).astype(np.int32)
    sc.upload_seeds(seeds)
    sc.iterations = bounces
    sc.render_nee(spp, strategy)
    model = replay_model(api, sc, spec, rgb)
    assert len(model.lights) == 1 and model.pe == 0.5
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


# ---------------------------------------------------------------------------- 3: closed forms
def floor_spec(kd):
    from opencl_path_tracer_amd import scenes
    mats = [((kd, kd, kd), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0)]
    fy, big = -10.0, 1e4
    tris = [((-big, fy, -big), (big, fy, big), (big, fy, -big)), ((-big, fy, -big), (-big, fy, big), (big, fy, big))]
    spec = scenes.SceneSpec(materials=mats, fov=60.0, shift=EYE_AT_ORIGIN, name="floor")
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.zeros(2, dtype=np.uint16)))
    return spec


@pytest.mark.parametrize("sky", ["constant", "half"])
def test_closed_form_floor_under_sky(api, sky):
    """An (effectively) infinite diffuse floor seen from 10 above it by a level camera, iterations = 2.  Constant sky L: the floor is
    E[kd cos] L = 2/3 kd L under the cosine density and the sky is exactly L.  L on one half of the phi range, 0 on the other: the
    floor's upper hemisphere is split in two mirror halves, so kd L / 3.  Batch means against batch-to-batch standard errors."""
    W, H, batches, spp = 16, 16, 32, 64
    kd = 0.5
    L = np.array([2.0, 1.0, 0.5])
    rgb = np.tile(L.astype(np.float32), (1, 1, 1)) if sky == "constant" else np.array([[L, 0 * L]], dtype=np.float32)
    expect = (2.0 / 3.0 if sky == "constant" else 1.0 / 3.0) * kd * L
    sc = api.Scene(W, H).load(floor_spec(kd))
    sc.set_environment(rgb)
    assert sc.debug_environment()["P_env"] == 1.0
    # rows below the horizon row see only floor, rows above it only sky (row H/2 - 1 holds the floor's far edge): the flat preview says so
    floor = np.zeros((H, W), dtype=bool)
    floor[:H // 2 - 1] = True
    above = np.zeros((H, W), dtype=bool)
    above[H // 2:] = True
    sc.iterations = 1
    sc.render_nee(64, "mis")
    flat = sc.read_colors()[:, :3].reshape(H, W, 3)
    assert (flat[floor] == np.float32(kd)).all()
    if sky == "constant":
        assert (flat[above] == L.astype(np.float32)).all()
    sc.iterations = 2
    rng = np.random.default_rng(23)
    for strategy in STRATEGIES:
        per = []
        for b in range(batches):
            sc.upload_seeds(rng.integers(1, 2 ** 31 - 2, W * H).astype(np.int32))
            sc.current_sample = 0
            sc.render_nee(spp, strategy)
            per.append(sc.read_colors()[:, :3].reshape(H, W, 3).astype(np.float64))
        per = np.asarray(per)
        if sky == "constant":
            assert (per[:, above] == L).all(), strategy
        mean = per.mean(axis=0)[floor]
        se = per.std(axis=0, ddof=1)[floor] / np.sqrt(batches)
        assert (se > 0).all()
        z = np.abs(mean - expect) / se
        print("%s %s: max |z| %.2f, mean ratio %s" % (sky, strategy, z.max(), mean.mean(axis=0) / expect))
        assert z.max() < 5.0, "%s: max |z| %.2f" % (strategy, z.max())


# ---------------------------------------------------------------------------- 4: same mean
def block_means(cols, W, H):
    return cols[:, :3].reshape(H // 8, 8, W // 8, 8, 3).mean(axis=(1, 3))


@pytest.mark.parametrize("lamp", [False, True])
def test_same_mean_per_block(api, lamp):
    """lamp = False: the sky is the only light (P_env forced to 1).  lamp = True: the box keeps its lamp and select = 0.5, so the sky
    and the light table are both sampled and the triangle pdfs carry 1 - P_env."""
    from opencl_path_tracer_amd import scenes
    W = H = 64
    batches, spp = 32, 64
    sc = api.Scene(W, H).load(open_box_spec(lamp))
    sc.set_environment(scenes.sun_and_sky(), select=0.5)
    assert sc.debug_environment()["P_env"] == (0.5 if lamp else 1.0)
    sc.iterations = CB_BOUNCES
    rng = np.random.default_rng(11)
    per = {s: [] for s in STRATEGIES}
    for b in range(batches):
        for s in per:
            sc.upload_seeds(rng.integers(1, 2 ** 31 - 2, W * H).astype(np.int32))
            sc.current_sample = 0
            sc.render_nee(spp, s)
            per[s].append(block_means(sc.read_colors(), W, H))
    m = {s: np.mean(v, axis=0) for s, v in per.items()}
    se = {s: np.std(v, axis=0, ddof=1) / np.sqrt(batches) for s, v in per.items()}
    for s in ("light", "mis"):
        z = np.abs(m[s] - m["bsdf"]) / np.sqrt(se[s] ** 2 + se["bsdf"] ** 2)
        print("%s: max |z| %.2f" % (s, z.max()))
        assert z.max() < 5.0, "%s: max |z| %.2f" % (s, z.max())


# ---------------------------------------------------------------------------- 5: it helps
def rmse(a, b):
    return float(np.sqrt(np.mean((a[:, :3].astype(np.float64) - b[:, :3].astype(np.float64)) ** 2)))


def test_mis_lowers_rmse_under_a_small_bright_source(api):
    """One texel of 64 x 32 holds more than 90 % of the map's power.  16 spp against a 4096-spp BSDF frame from other seeds: MIS RMSE
    is lower than BSDF RMSE.  Measured: MIS / BSDF = 0.512 (profiles/env/README.md); the bar is the geometric mean of that and 1."""
    W = H = 64
    spec, rgb = open_box_spec(), hot_texel_map()
    ref = api.Scene(W, H).load(spec)
    ref.set_environment(rgb)
    ref.iterations = CB_BOUNCES
    ref.upload_seeds(np.random.default_rng(5).integers(1, 2 ** 31 - 2, W * H).astype(np.int32))
    ref.render_nee(4096, "bsdf")
    reference = ref.read_colors()
    err = {}
    for s in ("bsdf", "mis"):
        sc = api.Scene(W, H).load(spec)
        sc.set_environment(rgb)
        sc.iterations = CB_BOUNCES
        sc.render_nee(16, s)
        err[s] = rmse(sc.read_colors(), reference)
    print("RMSE at 16 spp: %s, MIS / BSDF %.3f" % (err, err["mis"] / err["bsdf"]))
    assert err["mis"] < np.sqrt(0.512) * err["bsdf"], err


# ---------------------------------------------------------------------------- 6: stream and state
@pytest.mark.parametrize("lamp", [False, True])
def test_lcg_stream_is_renders_and_runs_repeat(api, oracle, lamp):
    """rnds against pt_render on a second context without a sky; rays against the oracle's frame, pt_render's parity target (the
    fused pt_render keeps its rays in registers and does not write them back), as tests/test_gpu_nee.py does."""
    from opencl_path_tracer_amd import scenes
    W, H = 48, 40
    spec = open_box_spec(lamp)
    plain = api.Scene(W, H).load(spec)
    plain.iterations = CB_BOUNCES
    plain.render(3)
    want_cols, want_rnds = plain.read_colors().copy(), plain.read_rnds().copy()
    fr = oracle.OracleFrame(W, H)
    fr.render(oracle.load_scene(spec), oracle.make_camera(spec.fov, spec.yaw, spec.pitch, spec.shift, W, H), CB_BOUNCES, 0, 3, nthreads=16)
    assert np.array_equal(want_rnds, fr.rnds())
    orays = fr.rays()
    for strategy in STRATEGIES:
        runs = []
        for _ in range(2):
            sc = api.Scene(W, H).load(spec)
            sc.set_environment(scenes.sun_and_sky(), select=0.4)
            assert sc.debug_environment()["P_env"] == (float(np.ceil(float(np.float32(0.4)) * 2.0 ** 24) / 2.0 ** 24) if lamp else 1.0)
            sc.iterations = CB_BOUNCES
            sc.render_nee(2, strategy)
            sc.render_nee(1, strategy)
            runs.append(state(sc))
        assert same_state(runs[0], runs[1]), strategy
        assert np.array_equal(runs[0][1], want_rnds), strategy
        assert same_bits(runs[0][2], orays["P"][:, :3]) and same_bits(runs[0][3], orays["D"][:, :3]), strategy
        assert not same_bits(runs[0][0], want_cols)


# ---------------------------------------------------------------------------- 7: flat preview
def test_flat_preview_shows_the_sky(api):
    W, H = 48, 32
    spec, rgb = replay_spec(), replay_map()
    spec.pitch = -30.0                       # looking up: the box's open top fills the upper part of the frame
    seeds = np.random.default_rng(29).integers(1, 2 ** 31 - 2, W * H).astype(np.int32)
    plain = api.Scene(W, H).load(spec)
    plain.upload_seeds(seeds)
    plain.iterations = 1
    plain.render_nee(1, "mis")
    before = plain.read_colors()[:, :3]
    sc = api.Scene(W, H).load(spec)
    sc.set_environment(rgb, scale=REPLAY["scale"], yaw_degrees=REPLAY["yaw_degrees"])
    sc.upload_seeds(seeds)
    sc.iterations = 1
    sc.render_nee(1, "mis")
    got = sc.read_colors()[:, :3]
    model = replay_model(api, sc, spec, rgb)
    miss = np.zeros(W * H, dtype=bool)
    sure = np.zeros(W * H, dtype=bool)
    want = np.zeros((W * H, 3))
    for i in range(W * H):
        s, r1 = E.R.lcg(int(seeds[i]))
        s, r2 = E.R.lcg(s)
        P, D = model.camera_ray(i, r1, r2)
        ti, _, tie = model.intersect(P, D)
        if tie:
            continue
        sure[i] = True
        if ti < 0:
            want[i], _, edge = model.sky(D)
            miss[i] = True
            sure[i] = not edge
    assert 0.05 < (miss & sure).mean() < 0.95
    sel = miss & sure
    assert np.array_equal(got[sel], want[sel].astype(np.float32))
    hit = sure & ~miss
    assert same_bits(got[hit], before[hit]) and not before[sel].any()


# ---------------------------------------------------------------------------- 8: ranks
def test_tiled_ranks_assemble_the_single_context_frame(api):
    from opencl_path_tracer_amd import scenes
    W, H, world = 64, 52, 3
    spec, rgb = open_box_spec(lamp=True), scenes.sun_and_sky()
    one = api.Scene(W, H).load(spec)
    one.set_environment(rgb, yaw_degrees=40.0)
    one.iterations = CB_BOUNCES
    one.render_nee(3, "mis")
    whole = state(one)
    seen = np.zeros(W * H, dtype=bool)
    for r in range(world):
        sc = api.Scene(W, H, rank=r, world=world, rows_per_block=8).load(spec)
        sc.set_environment(rgb, yaw_degrees=40.0)
        sc.iterations = CB_BOUNCES
        sc.render_nee(3, "mis")
        ids = sc.local_pixel_ids()
        assert same_state(state(sc), tuple(a[ids] for a in whole)), r
        seen[ids] = True
    assert seen.all()


# ---------------------------------------------------------------------------- 9: refusals
def test_other_render_paths_refuse_while_a_sky_is_set(api, cb_spec):
    from opencl_path_tracer_amd import scenes
    W, H = 32, 32

    def frames(sc):
        out = []
        sc.iterations = 4
        sc.render(2)
        out.append(state(sc))
        sc.seed_default()
        sc.current_sample = 0
        sc.render(2, fused=False)
        out.append(state(sc))
        sc.seed_default()
        sc.current_sample = 0
        sc.render_adaptive(2, 8, 0.05)
        out.append(state(sc))
        sc.seed_default()
        sc.current_sample = 0
        sc.set_option("variant", 1)
        sc.render(2)
        out.append(state(sc))
        sc.set_option("variant", 0)
        return out

    want = frames(api.Scene(W, H).load(cb_spec))
    sc = api.Scene(W, H).load(cb_spec)
    sc.iterations = 4
    for rgb in (scenes.sun_and_sky(), np.zeros((2, 4, 3), dtype=np.float32)):
        sc.set_environment(rgb)
        calls = [lambda: sc.render(2), lambda: sc.render(1, fused=False), lambda: sc.generate_rays(), lambda: sc.trace_rays(),
                 lambda: sc.render_adaptive(2, 8, 0.05)]
        for call in calls:
            with pytest.raises(api.PtError) as e:
                call()
            assert e.value.code == api.PT_EINVAL and "pt_render_nee" in str(e.value)
        sc.set_option("variant", 1)
        with pytest.raises(api.PtError) as e:
            sc.render(2)
        assert e.value.code == api.PT_EINVAL and "pt_render_nee" in str(e.value)
        sc.set_option("variant", 0)
    assert sc.current_sample == 0
    sc.clear_environment()
    got = frames(sc)
    for a, b in zip(got, want):
        assert same_state(a, b)


# ---------------------------------------------------------------------------- 10: composition
def test_sky_lit_frame_composes_with_variance_guides_denoise_and_temporal(api):
    from opencl_path_tracer_amd import scenes
    W, H = 64, 48
    sc = api.Scene(W, H).load(open_box_spec(lamp=True))
    sc.set_environment(scenes.sun_and_sky())
    sc.set_option("moments", 1)
    sc.iterations = CB_BOUNCES
    sc.render_nee(8, "mis")
    cols = sc.read_colors()
    assert np.isfinite(cols).all()
    var = sc.read_variance()
    assert np.isfinite(var).all() and (var >= 0).all()
    sc.render_aovs(1, 4)
    nd = sc.read_aovs()[1]
    sky = (nd[:, 3] < 0).reshape(H, W)
    assert 0.05 < sky.mean() < 0.95
    assert (cols[sky.reshape(-1), :3].sum(axis=1) > 0).all()            # the sky is lit
    iterations = 2
    reach = 2 * sum(2 ** i for i in range(iterations))
    results = {"denoise_variance": sc.denoise_variance(iterations=iterations)}
    tmp = sc.temporal_accumulate()
    assert np.isfinite(tmp).all()
    results["denoise_temporal"] = sc.denoise_temporal(iterations=iterations)
    assert same_bits(sc.read_colors(), cols)
    img = cols[:, :3].reshape(H, W, 3)
    for name, dn in results.items():
        assert np.isfinite(dn).all(), name
        f = dn[:, :3].reshape(H, W, 3)
        for y, x in zip(*np.nonzero(sky)):
            ys, xs = slice(max(0, y - reach), y + reach + 1), slice(max(0, x - reach), x + reach + 1)
            around = img[ys, xs][sky[ys, xs]]
            lo, hi = around.min(axis=0), around.max(axis=0)
            tol = 1e-5 * hi + 1e-7
            assert (f[y, x] >= lo - tol).all() and (f[y, x] <= hi + tol).all(), (name, y, x)
