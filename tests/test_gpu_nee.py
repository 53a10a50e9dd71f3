"""-m gpu: next-event estimation with MIS (Scene.render_nee, pt_nee.hip).

  * PT_NEE_BSDF is pt_render's estimator: colors, rnds and rays equal the oracle's bit for bit (three node modes, tiled rank);
  * the light samples never touch the LCG: rnds and rays equal the oracle's after LIGHT and MIS frames too;
  * MIS against tests/nee_ref.py (float64, brute force, same LCG and hash) on a scene of 17 triangles;
  * LIGHT and MIS have BSDF's mean (per 8x8 block, 5 sigma from independent batches), a closed form, determinism,
    and the point of it all: lower RMSE at equal spp."""

import numpy as np
import pytest

import nee_ref as R

pytestmark = pytest.mark.gpu

CB_BOUNCES = 8


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def oracle_frame(oracle, osc, spec, W, H, bounces, spp):
    cam = oracle.make_camera(spec.fov, spec.yaw, spec.pitch, spec.shift, W, H)
    fr = oracle.OracleFrame(W, H)
    fr.render(osc, cam, bounces, 0, spp, nthreads=16)
    return fr


def check_lcg_and_rays(sc, fr, ids=None):
    ornds, orays = fr.rnds(), fr.rays()
    if ids is not None:
        ornds, orays = ornds[ids], orays[ids]
    rays = sc.read_rays()
    assert np.array_equal(sc.read_rnds(), ornds)
    assert same_bits(rays["P"][:, :3], orays["P"][:, :3]) and same_bits(rays["D"][:, :3], orays["D"][:, :3])


# ---------------------------------------------------------------------------- 1 + 2: skeleton exact, LCG untouched
@pytest.mark.parametrize("lds,wide,mode", [(2, 1, 0), (0, 1, 1), (2, 2, 3)])
@pytest.mark.parametrize("W,H", [(64, 48), (37, 29)])
def test_bsdf_strategy_is_render_bit_for_bit(api, oracle, cb_spec, cb_oracle_scene, lds, wide, mode, W, H):
    fr = oracle_frame(oracle, cb_oracle_scene, cb_spec, W, H, CB_BOUNCES, 3)
    for strategy in ("bsdf", "light", "mis"):
        sc = api.Scene(W, H)
        sc.set_option("wide_nodes", wide)
        sc.load(cb_spec)
        sc.set_option("lds_scene", lds)
        assert sc.stat("node_mode") == mode
        sc.iterations = CB_BOUNCES
        sc.render_nee(2, strategy)
        sc.render_nee(1, strategy)
        assert sc.current_sample == 3
        check_lcg_and_rays(sc, fr)
        if strategy == "bsdf":
            assert same_bits(sc.read_colors()[:, :3], fr.colors()[:, :3])
        else:
            assert not same_bits(sc.read_colors()[:, :3], fr.colors()[:, :3])


def test_bsdf_strategy_tiled_rank_and_wavefront_variant(api, oracle, cb_spec, cb_oracle_scene):
    W, H = 64, 52
    fr = oracle_frame(oracle, cb_oracle_scene, cb_spec, W, H, CB_BOUNCES, 3)
    for r in range(2):
        sc = api.Scene(W, H, rank=r, world=2, rows_per_block=8).load(cb_spec)
        sc.iterations = CB_BOUNCES
        sc.render_nee(3, "bsdf")
        ids = sc.local_pixel_ids()
        assert same_bits(sc.read_colors()[:, :3], fr.colors()[ids, :3])
        check_lcg_and_rays(sc, fr, ids)
        sc.seed_default()
        sc.current_sample = 0
        sc.render_nee(3, "mis")
        check_lcg_and_rays(sc, fr, ids)
    sc = api.Scene(W, H).load(cb_spec)
    sc.set_option("variant", 1)
    sc.iterations = CB_BOUNCES
    sc.render_nee(3, "bsdf")
    assert same_bits(sc.read_colors()[:, :3], fr.colors()[:, :3])


@pytest.mark.parametrize("treelet,wide,mode", [(40, 1, 2), (0, 2, 3)])
def test_bsdf_strategy_mesh_treelet_and_wide_overflow(api, oracle, treelet, wide, mode):
    """The other two launch shapes on a tree too large for whole-tree staging: the treelet instance (1,024-thread blocks, the top
    40 nodes in LDS) and 4-wide nodes with only 6 stack entries per lane in LDS (the rest in global memory).  BSDF bit for bit,
    and rnds / rays after an MIS frame."""
    from opencl_path_tracer_amd import scenes
    spec = scenes.displaced_grid_mesh(6000)
    osc = oracle.load_scene(spec)
    W = H = 64
    fr = oracle_frame(oracle, osc, spec, W, H, 6, 3)
    for strategy in ("bsdf", "mis"):
        sc = api.Scene(W, H)
        sc.set_option("treelet", treelet)
        sc.set_option("lds_scene", 2)
        sc.set_option("wide_nodes", wide)
        if wide == 2:
            sc.set_option("wide_lds_entries", 6)
        sc.load(spec)
        assert sc.stat("node_mode") == mode
        assert len(sc.debug_light_table()[0]) > 0
        sc.iterations = 6
        sc.render_nee(3, strategy)
        check_lcg_and_rays(sc, fr)
        if strategy == "bsdf":
            assert same_bits(sc.read_colors()[:, :3], fr.colors()[:, :3])


# ---------------------------------------------------------------------------- 3: replay against the float64 model
def replay_spec(api):
    from opencl_path_tracer_amd import scenes
    mats = [
        ((0.6, 0.6, 0.6), (0.2, 0.2, 0.2), (0, 0, 0), (0, 0, 0), (0, 0, 0), 20.0, 0),      # 0 white, glossy lobe
        ((0.6, 0.1, 0.1), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),             # 1 red
        ((0.1, 0.6, 0.1), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),             # 2 green
        ((0, 0, 0), (0, 0, 0), (6.0, 5.0, 4.0), (0, 0, 0), (0, 0, 0), 0.0, 3),             # 3 lamp
        ((0, 0, 0), (0, 0, 0), (12.0, 4.0, 2.0), (0, 0, 0), (0, 0, 0), 0.0, 3),            # 4 small hot emitter
        scenes.BUILTIN_MATERIALS[scenes.CHROMIUM],                                           # 5 mirror
    ]

    def quad(a, b, c, d):
        return [(a, b, c), (a, c, d)]
    x0, x1, y0, y1, z0, z1 = -5.0, 5.0, -3.0, 5.0, -1.0, 12.0
    tris, mo = [], []
    for q, m in ((quad((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)), 0),      # floor
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
    spec = scenes.SceneSpec(materials=mats, name="nee_replay", shift=(-500.0, -500.0, 1299.0378))
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.asarray(mo, dtype=np.uint16)))
    assert spec.ntris <= 20
    return spec


def test_mis_matches_float64_model(api):
    W, H, spp, bounces = 48, 32, 2, 4
    spec = replay_spec(api)
    sc = api.Scene(W, H).load(spec)
    seeds = sc.read_rnds().copy()
    sc.iterations = bounces
    sc.render_nee(spp, "mis")
    verts, mo = spec.objects[0]
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    model = R.Model(verts, recs["N"], mats, mo, sc.camera[0], table=sc.debug_light_table())
    assert len(model.lights) == 3
    want, want_seeds, ties = model.render(seeds, bounces, spp, 2)
    got = sc.read_colors()[:, :3].astype(np.float64)
    # near-tie pixels (a ray of the model within 1e-4 barycentric of an edge, or two hits within 1e-5 relative: float32 and
    # float64 may pick different triangles there) are excluded; the rest agree in LCG state and within 2e-3 relative
    keep = ~ties
    assert keep.mean() > 0.9, "too many near-tie pixels: %d" % int(ties.sum())
    assert np.array_equal(sc.read_rnds()[keep], want_seeds[keep])
    scale = float(want[keep].max())
    err = np.abs(got[keep] - want[keep])
    bad = err > 2e-3 * np.abs(want[keep]) + 1e-6 * scale
    assert not bad.any(), "%d of %d pixel channels differ; worst %g" % (int(bad.sum()), bad.size, float((err / (np.abs(want[keep]) + 1e-6 * scale)).max()))
    assert float(want[keep].mean()) > 0.0


# ---------------------------------------------------------------------------- 4: same mean
def block_means(cols, W, H):
    return cols[:, :3].reshape(H // 8, 8, W // 8, 8, 3).mean(axis=(1, 3))


def test_same_mean_per_block(api, cb_spec):
    W = H = 64
    batches, spp = 32, 64
    sc = api.Scene(W, H).load(cb_spec)
    sc.iterations = CB_BOUNCES
    rng = np.random.default_rng(11)
    per = {s: [] for s in ("bsdf", "light", "mis")}
    for b in range(batches):
        seeds = rng.integers(1, 2 ** 31 - 2, W * H).astype(np.int32)
        for s in per:
            sc.upload_seeds(seeds if s == "bsdf" else rng.integers(1, 2 ** 31 - 2, W * H).astype(np.int32))
            sc.current_sample = 0
            sc.render_nee(spp, s)
            per[s].append(block_means(sc.read_colors(), W, H))
    m = {s: np.mean(v, axis=0) for s, v in per.items()}
    se = {s: np.std(v, axis=0, ddof=1) / np.sqrt(batches) for s, v in per.items()}
    for s in ("light", "mis"):
        z = np.abs(m[s] - m["bsdf"]) / np.sqrt(se[s] ** 2 + se["bsdf"] ** 2)
        assert z.max() < 5.0, "%s: max |z| %.2f" % (s, z.max())


# ---------------------------------------------------------------------------- 5: closed form; no lobe vertex, no change
def test_closed_form_square_over_floor(api):
    """Emitting 1 x 1 square 2 above an (effectively) infinite diffuse floor, iterations = 2:
    colour(x) = E kd / pi  Int cos_x^2 cos_y^2 / r^2 dA over the square (h = 2 - 0.001: the offset origin)."""
    from opencl_path_tracer_amd import scenes
    W = H = 16
    kd, E, h, cx = 0.5, 10.0, 2.0, -3.0
    mats = [((kd, kd, kd), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),
            ((0, 0, 0), (0, 0, 0), (E, E, E), (0, 0, 0), (0, 0, 0), 0.0, 3)]
    fy = -10.0                         # floor 10 below the eye (at the origin), camera looking straight down
    big = 1e4
    tris = [((-big, fy, -big), (big, fy, big), (big, fy, -big)), ((-big, fy, -big), (-big, fy, big), (big, fy, big)),
            ((cx - 0.5, fy + h, -0.5), (cx + 0.5, fy + h, -0.5), (cx + 0.5, fy + h, 0.5)),
            ((cx - 0.5, fy + h, -0.5), (cx + 0.5, fy + h, 0.5), (cx - 0.5, fy + h, 0.5))]
    spec = scenes.SceneSpec(materials=mats, fov=20.0, pitch=90.0, shift=(-500.0, -500.0, 1299.0378), name="square")
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.array([0, 0, 1, 1], dtype=np.uint16)))
    sc = api.Scene(W, H).load(spec)
    sc.iterations = 2
    sc.render_nee(1024, "mis")
    got = sc.read_colors()[:, 0].astype(np.float64)
    # quadrature per pixel, averaged over a 4 x 4 grid of floor points inside the pixel
    cam = sc.camera[0]
    model = R.Model(np.asarray(tris, np.float64), np.tile([0.0, 1.0, 0.0], (4, 1)), np.concatenate([api.Material(*m) for m in mats]),
                    np.array([0, 0, 1, 1]), cam)
    g = (np.arange(64) + 0.5) / 64 - 0.5
    sx, sz = np.meshgrid(cx + g, g)
    want = np.zeros(W * H)
    for i in range(W * H):
        acc = 0.0
        for a in range(4):
            for b in range(4):
                P, D = model.camera_ray(i, (a + 0.5) / 4, (b + 0.5) / 4)
                t = (fy - P[1]) / D[1]
                x, z = P[0] + t * D[0], P[2] + t * D[2]
                hh = h - 0.001
                r2 = (sx - x) ** 2 + (sz - z) ** 2 + hh * hh
                acc += float(np.sum(hh ** 4 / r2 ** 3)) / 64 ** 2
        want[i] = E * kd / np.pi * acc / 16
    rel = np.abs(got - want) / want
    assert rel.max() < 0.04, rel.max()
    assert abs(got.mean() / want.mean() - 1.0) < 0.005


def test_mirror_to_emitter_mis_equals_bsdf(api):
    """Camera -> mirror -> planar emitter: no lobe vertex precedes an emitter hit, and a light sample from the emitter itself
    has cos_x <= 0, so MIS adds and weighs nothing: the same bits as BSDF."""
    from opencl_path_tracer_amd import scenes
    mats = [scenes.BUILTIN_MATERIALS[scenes.CHROMIUM], scenes.BUILTIN_MATERIALS[scenes.LAMP]]
    tris = [((-20, -20, 10), (20, -20, 10), (20, 20, 10)), ((-20, -20, 10), (20, 20, 10), (-20, 20, 10)),      # mirror facing the camera
            ((-4, -4, -2), (4, -4, -2), (4, 4, -2)), ((-4, -4, -2), (4, 4, -2), (-4, 4, -2))]                    # emitter behind the eye
    spec = scenes.SceneSpec(materials=mats, shift=(-500.0, -500.0, 1299.0378), name="mirror")
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.array([0, 0, 1, 1], dtype=np.uint16)))
    out = {}
    for s in ("bsdf", "mis"):
        sc = api.Scene(32, 32).load(spec)
        sc.iterations = 6
        sc.render_nee(4, s)
        out[s] = sc.read_colors()[:, :3]
        assert len(sc.debug_light_table()[0]) == 2
    assert out["bsdf"].max() > 0
    assert same_bits(out["mis"], out["bsdf"])


# ---------------------------------------------------------------------------- 6: determinism
def test_determinism(api, cb_spec):
    W, H = 48, 40
    a = api.Scene(W, H).load(cb_spec)
    b = api.Scene(W, H).load(cb_spec)
    a.iterations = b.iterations = CB_BOUNCES
    a.render_nee(8, "mis")
    a.render_nee(8, "mis")
    b.render_nee(16, "mis")
    ca = a.read_colors()
    assert same_bits(ca[:, :3], b.read_colors()[:, :3]) and np.array_equal(a.read_rnds(), b.read_rnds())
    a.seed_default()
    a.current_sample = 0
    a.render_nee(16, "mis")
    assert same_bits(ca[:, :3], a.read_colors()[:, :3])


# ---------------------------------------------------------------------------- 7: it helps
def walls_spec():
    from opencl_path_tracer_amd import scenes
    spec = scenes.SceneSpec(materials=list(scenes.BUILTIN_MATERIALS), name="cornell_walls")
    spec.objects.append(scenes.cornell_walls())
    return spec


def rmse(a, b):
    return float(np.sqrt(np.mean((a[:, :3].astype(np.float64) - b[:, :3].astype(np.float64)) ** 2)))


def emitter_edges(api, spec, W, H):
    """Pixels whose primary ray may see an emitter: the render_aovs material of the pixel or of a neighbour is type 3.  Their
    error is the camera's jitter across the lamp's edge (a 2 E |cos| step), which every strategy keeps (weight 1)."""
    sc = api.Scene(W, H).load(spec)
    sc.render_aovs(1, 0)
    mat = sc.read_aovs()[0][:, 3].astype(np.int64)
    emit = np.isin(mat, [i for i, m in enumerate(spec.materials) if m[6] == 3]).reshape(H, W)
    p = np.pad(emit, 1)
    out = np.zeros_like(emit)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + H, dx:dx + W]
    return out.reshape(-1)


def rmse_runs(api, spec, W, H, spp):
    ref = api.Scene(W, H).load(spec)
    ref.iterations = CB_BOUNCES
    ref.upload_seeds(np.random.default_rng(5).integers(1, 2 ** 31 - 2, W * H).astype(np.int32))
    ref.render(4096)
    reference = ref.read_colors()
    out = {}
    for s in ("bsdf", "mis"):
        sc = api.Scene(W, H).load(spec)
        sc.iterations = CB_BOUNCES
        sc.render_nee(spp, s)
        out[s] = sc.read_colors()
    return reference, out


@pytest.mark.parametrize("which", ["walls", "cornell"])
def test_mis_lowers_rmse(api, cb_spec, which):
    """Walls only, 128 x 128, 16 spp: away from the pixels that see the lamp's edge, MIS RMSE <= 0.5 x BSDF RMSE; over the
    whole frame (and on the full Cornell box, whose caustics NEE cannot reach) MIS RMSE < BSDF RMSE."""
    W = H = 128
    spec = walls_spec() if which == "walls" else cb_spec
    reference, cols = rmse_runs(api, spec, W, H, 16)
    err = {s: rmse(c, reference) for s, c in cols.items()}
    assert err["mis"] < err["bsdf"], err
    if which == "walls":
        keep = ~emitter_edges(api, spec, W, H)
        assert 0.5 < keep.mean() < 1.0
        em = {s: rmse(c[keep], reference[keep]) for s, c in cols.items()}
        assert em["mis"] <= 0.5 * em["bsdf"], (em, err)


@pytest.mark.xfail(strict=True, reason="over the whole 128 x 128 frame the pixels on the lamp's edge (camera jitter across a 2 E |cos| "
                                       "step, weight 1 in every strategy) dominate the error: MIS / BSDF RMSE is 0.57 there, 0.22 at "
                                       "1920 x 1080, whose narrower vertical view shows less of the lamp (profiles/nee/README.md)")
def test_mis_halves_rmse_whole_frame_walls(api):
    reference, cols = rmse_runs(api, walls_spec(), 128, 128, 16)
    assert rmse(cols["mis"], reference) <= 0.5 * rmse(cols["bsdf"], reference)


# ---------------------------------------------------------------------------- 8: composes
def test_nee_frame_composes_with_denoiser_and_resolve(api, cb_spec):
    W, H = 64, 48
    sc = api.Scene(W, H).load(cb_spec)
    sc.iterations = CB_BOUNCES
    sc.render_nee(4, "mis")
    cols = sc.read_colors()
    sc.render_aovs(1, 4)
    dn = sc.denoise()
    assert dn.shape == cols.shape and np.isfinite(dn).all()
    assert same_bits(sc.read_colors(), cols)          # the filter never writes colors
    ldr = sc.resolve_ldr(0)
    lit = cols[:, :3].sum(axis=1) > 0                  # black pixels resolve to NaN, like the reference's (test_ldr_resolve)
    assert lit.mean() > 0.5 and np.isfinite(ldr[lit]).all() and ldr[lit, :3].max() > 0
    # and pt_render continues the same running mean
    sc.render(2)
    assert sc.current_sample == 6


def test_adaptive_frame_blocks_render_nee(api, cb_spec):
    sc = api.Scene(32, 32).load(cb_spec)
    sc.iterations = 4
    sc.render_adaptive(2, 8, 1e9)
    with pytest.raises(api.PtError) as e:
        sc.render_nee(1)
    assert e.value.code == api.PT_EINVAL and "adaptive" in str(e.value)
    sc.current_sample = 0
    sc.render_nee(1)
