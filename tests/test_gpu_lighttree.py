"""-m gpu: the light hierarchy on Scene.render_nee (option light_tree; include/pt_api.h pins the tree, the walk and the probabilities,
DESIGN.md section 5.22): the twelfth k_nee family, stat "nee_family" 11.

  1 k_debug_light_tree equals the library's host walk bit for bit
  2 null cases, bit for bit against the option-off frame in all four forms: one emitting triangle, no emitting triangle under a sky,
    PT_NEE_BSDF on many_lights(16); the Cornell box differs; rnds and rays are the option-off frame's in every strategy
  3 many_lights(16) under PT_NEE_LIGHT and PT_NEE_MIS against the float64 model (tests/lighttree_ref.py), with the tolerance and the
    exclusion rule of tests/test_gpu_nee.py's MIS replay
  4 the same mean as the option-off frame (five standard errors from independent 4-spp frames), under LIGHT and MIS
  5 lower variance on many_lights(64)
  6 the sixteen instances: node modes bit for bit, adaptive tiles and tiled ranks hold render_nee's bits
  7 with a sky (P_env), a light set (P_ana), bounded fog (a scatter vertex culls nothing) and a live interior binding (flags bit 7):
    each by rule 4, the option-off mean within five standard errors"""

import numpy as np
import pytest

import lighttree_ref as LT
import nee_instances as I
import nee_ref as R
import test_gpu_lights as TL
import test_gpu_nee_instances as TI
import test_lighttree_host as TH

pytestmark = pytest.mark.gpu

same_bits, state, same_state = TL.same_bits, TL.state, TL.same_state
FAMILY = 11
BOUNCES = 4


def corridor(api, W, H, n=16, tree=True, **kw):
    from opencl_path_tracer_amd import scenes
    sc = api.Scene(W, H, **kw).load(scenes.many_lights(n))
    sc.set_option("light_tree", 1 if tree else 0)
    sc.iterations = BOUNCES
    return sc


# ---------------------------------------------------------------------------- 1: the debug kernel
def test_device_walk_equals_the_host_walk(api):
    from opencl_path_tracer_amd import scenes
    host = TH.host_scene(api, scenes.many_lights(TH.N_LAMPS))
    dev = api.Scene(16, 16).load(scenes.many_lights(TH.N_LAMPS))
    nodes, tri = host.debug_light_tree()
    dn, dt = dev.debug_light_tree()
    assert nodes.tobytes() == dn.tobytes() and tri.tobytes() == dt.tobytes()
    rng = np.random.default_rng(5)
    z1 = 3.0 * TH.N_LAMPS + 2.0
    n = 64 * 64
    pts = np.stack([rng.uniform(-1.99, 1.99, n), rng.uniform(-1.499, 1.499, n), rng.uniform(-0.9, z1 - 0.1, n)], axis=1).astype(np.float32)
    g = rng.normal(size=(n, 3))
    nrm = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    nrm[::3] = (0.0, 1.0, 0.0)
    pts[::3, 1] = -1.499                       # the floor, where the horizon culls
    nrm[1::9] = 0.0                            # scatter vertices
    u0 = (rng.integers(0, 1 << 24, size=n) * 2.0 ** -24).astype(np.float32)
    tris = rng.integers(0, 2 * TH.N_LAMPS + 6, size=n)          # lights, and some walls
    a = host.debug_light_tree_eval(pts, nrm, u0, tris)
    b = dev.debug_light_tree_eval(pts, nrm, u0, tris, on_device=True)
    assert a.tobytes() == b.tobytes()
    assert len(np.unique(a["slot"])) > TH.N_LAMPS and (a["p_weight"] == 0.0).any() and (a["p_weight"] > 0.0).any()


# ---------------------------------------------------------------------------- 2: null cases
def one_light_spec():
    """tests/test_gpu_nee.py's replay scene with one emitting triangle left: the small emitter on the left wall"""
    import test_gpu_nee as TN
    spec = TN.replay_spec(None)
    v, mo = spec.objects[0]
    keep = mo != 3
    spec.objects[0] = (v[keep], mo[keep])
    return spec


def frames_on_off(api, make, form, strategy="mis", family_off=None):
    """the compared states of option off and on, the stats checked; a tiled form shares the option-off frame's threshold"""
    out, thr = [], None
    for on in (0, 1):
        sc = make()
        sc.set_option("light_tree", on)
        if form & 2:
            if thr is None:
                sc.iterations = BOUNCES
                thr = TI.threshold_of(sc)
            sc.iterations = BOUNCES
            sc.render_adaptive(4, 16, thr, metric="half", path="nee", strategy=strategy)
            out.append((sc.read_colors().copy(), sc.read_rnds().copy(), sc.sample_counts().copy()))
        else:
            sc.iterations = BOUNCES
            sc.render_nee(3, strategy)
            out.append(state(sc))
        fam = int(sc.stat("nee_family"))
        assert int(sc.stat("nee_form")) == form
        if family_off is not None:
            assert fam == (family_off[1] if on else family_off[0]), (on, fam)
        sc.close()
    return out


@pytest.mark.parametrize("form", range(4), ids=I.FORMS)
def test_null_cases_keep_every_bit(api, form):
    from opencl_path_tracer_amd import scenes
    sky = bool(form & 1)

    def with_sky(sc):
        if sky:
            sc.set_environment(scenes.sun_and_sky())
        return sc
    # one emitting triangle: P = 1 and inv_area is P_sel / area
    off, on = frames_on_off(api, lambda: with_sky(api.Scene(48, 32).load(one_light_spec())), form, family_off=(0, FAMILY))
    assert off[0][:, :3].mean() > 0.0 and TI.same_frames(on, off)
    # PT_NEE_BSDF on many_lights(16): no light sample is taken
    off, on = frames_on_off(api, lambda: with_sky(api.Scene(32, 32).load(scenes.many_lights(16))), form, strategy="bsdf", family_off=(0, FAMILY))
    assert off[0][:, :3].mean() > 0.0 and TI.same_frames(on, off)
    # no emitting triangle, under a sky: the table is empty and the family stays what it was
    if sky:
        spec = scenes.many_lights(4)
        spec.materials[1] = spec.materials[2] = spec.materials[0]
        spec.objects[0] = (spec.objects[0][0][:-4], spec.objects[0][1][:-4])          # (open at the right and behind: the sky gets in)
        off, on = frames_on_off(api, lambda: with_sky(api.Scene(32, 32).load(spec)), form, family_off=(0, 0))
        assert off[0][:, :3].mean() > 0.0 and TI.same_frames(on, off)


def test_cornell_box_differs_and_keeps_the_lcg(api, cb_spec):
    """The lamp's two triangles share one bounding box, so their spheres and phi are equal and pL is exactly 0.5 from every vertex, as
    P_sel is: the LIGHT and MIS frames differ from the table's because the tree orders the two triangles the other way round (the
    centroids' box is as long in x as in z and the tie goes to z), not because a probability moved.  rnds and rays never differ."""
    W = H = 64
    frames = {}
    for strategy in ("bsdf", "light", "mis"):
        for on in (0, 1):
            sc = api.Scene(W, H).load(cb_spec)
            sc.set_option("light_tree", on)
            sc.iterations = 8
            sc.render_nee(3, strategy)
            assert sc.stat("nee_family") == (FAMILY if on else 0)
            frames[strategy, on] = state(sc)
            sc.close()
        a, b = frames[strategy, 0], frames[strategy, 1]
        assert all(same_bits(x, y) if x.dtype == np.float32 else np.array_equal(x, y) for x, y in zip(a[1:], b[1:])), strategy      # rnds, rays
        assert same_bits(a[0], b[0]) == (strategy == "bsdf"), strategy


# ---------------------------------------------------------------------------- 3: the float64 model
@pytest.mark.parametrize("strategy", ["light", "mis"])
def test_matches_float64_model(api, strategy):
    from opencl_path_tracer_amd import scenes
    W, H, spp = 32, 32, 2
    spec = scenes.many_lights(16)
    sc = corridor(api, W, H)
    seeds = sc.read_rnds().copy()
    sc.render_nee(spp, strategy)
    assert sc.stat("nee_family") == FAMILY
    verts, mo = spec.objects[0]
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    model = LT.TreeModel(verts, recs["N"], mats, mo, sc.camera[0], table=sc.debug_light_table(), tree=LT.Tree(*sc.debug_light_tree()))
    want, want_seeds, ties = model.render(seeds, BOUNCES, spp, {"light": 1, "mis": 2}[strategy])
    got = sc.read_colors()[:, :3].astype(np.float64)
    keep = ~ties                                   # tests/test_gpu_nee.py's rule and tolerance
    assert keep.mean() > 0.9, "too many near-tie pixels: %d" % int(ties.sum())
    assert np.array_equal(sc.read_rnds()[keep], want_seeds[keep])
    scale = float(want[keep].max())
    err = np.abs(got[keep] - want[keep])
    bad = err > 2e-3 * np.abs(want[keep]) + 1e-6 * scale
    print("worst relative error %.3g over %d pixels" % (float((err / (np.abs(want[keep]) + 1e-6 * scale)).max()), int(keep.sum())))
    assert not bad.any(), "%d of %d pixel channels differ; worst %g" % (int(bad.sum()), bad.size, float((err / (np.abs(want[keep]) + 1e-6 * scale)).max()))
    assert float(want[keep].mean()) > 0.0


# ---------------------------------------------------------------------------- 4: the same mean
def block_means(cols, W, H):
    return cols[:, :3].astype(np.float64).reshape(H // 8, 8, W // 8, 8, 3).mean(axis=(1, 3))


def check_same_mean(make, W, H, strategy, seed, batches=256, spp=4):
    """block means of batches x spp samples with the option on and off, from independent frames of spp samples on independent seeds,
    agree within five standard errors; returns the largest |z|"""
    rng = np.random.default_rng(seed)
    per = {}
    for on in (0, 1):
        sc = make()
        sc.set_option("light_tree", on)
        sc.iterations = BOUNCES
        got = []
        for _ in range(batches):
            sc.upload_seeds(rng.integers(1, 2 ** 31 - 2, W * H).astype(np.int32))
            sc.current_sample = 0
            sc.render_nee(spp, strategy)
            got.append(block_means(sc.read_colors(), W, H))
        per[on] = np.asarray(got)
        sc.close()
    m = {k: v.mean(axis=0) for k, v in per.items()}
    se = {k: v.std(axis=0, ddof=1) / np.sqrt(batches) for k, v in per.items()}
    assert m[0].mean() > 0.0
    z = np.abs(m[1] - m[0]) / np.sqrt(se[0] ** 2 + se[1] ** 2 + 1e-300)
    print("max |z| %.2f, variance of a block mean off / on %.3f" % (float(z.max()), float((se[0] ** 2).mean() / (se[1] ** 2).mean())))
    assert z.max() < 5.0, "max |z| %.2f" % z.max()
    return float(z.max())


@pytest.mark.parametrize("strategy", ["light", "mis"])
def test_same_mean_as_the_table(api, strategy):
    from opencl_path_tracer_amd import scenes
    W = H = 32
    check_same_mean(lambda: api.Scene(W, H).load(scenes.many_lights(16)), W, H, strategy, seed=21)


# ---------------------------------------------------------------------------- 5: variance
def test_lower_variance_on_many_lights_64(api):
    W = H = 64
    spp = 64
    v = {}
    for on in (0, 1):
        sc = corridor(api, W, H, n=64, tree=bool(on))
        sc.set_option("moments", 1)
        sc.render_nee(spp, "mis")
        v[on] = float(np.asarray(sc.read_variance(), dtype=np.float64).mean())
        sc.close()
    print("mean per-pixel variance of the mean: table %.6g, tree %.6g, ratio %.3f" % (v[0], v[1], v[0] / v[1]))
    assert v[1] < v[0]


# ---------------------------------------------------------------------------- 6: the instances
def everything(api, scene, placement, sky):
    """tests/nee_instances.py's scene with every feature and the fog live, a waxy interior in the glass, and the option on"""
    import test_gpu_interior as TG
    sc, mode = I.build(api, scene, "medium", placement, sky=sky)
    TG.bind(sc, I.scene_spec(scene, True, True), **TG.WAX)
    sc.set_option("light_tree", 1)
    return sc, mode


@pytest.mark.parametrize("form", range(4), ids=I.FORMS)
def test_node_modes_render_the_same_bits(api, form):
    import test_gpu_interior as TG
    for scene, first in (("small", "lds"), ("mesh", "treelet")):
        frames, thr = {}, None
        for placement in I.PLACEMENTS[scene]:
            sc, mode = everything(api, scene, placement, bool(form & 1))
            if form & 2 and thr is None:
                sc.iterations = TL.CB_BOUNCES
                thr = TI.threshold_of(sc)
            frames[placement] = TI.render(sc, form, thr)
            got = tuple(int(sc.stat(k)) for k in ("node_mode", "nee_family", "nee_form", "nee_block"))
            assert got == (mode, FAMILY, form, TG.block_of(form, mode)), (scene, placement, got)
            sc.close()
        want = frames[first]
        assert np.isfinite(want[0]).all() and want[0][:, :3].mean() > 0.0
        for placement, got in frames.items():
            assert TI.same_frames(got, want), (I.FORMS[form], scene, placement)


@pytest.mark.parametrize("sky", [False, True])
def test_adaptive_nee_tiles_hold_render_nee_bits(api, sky):
    from opencl_path_tracer_amd import scenes
    W, H = 36, 20

    def make():
        sc = corridor(api, W, H)
        if sky:
            sc.set_environment(scenes.sun_and_sky())
        return sc
    sc = make()
    thr = TI.threshold_of(sc)
    sc.render_adaptive(4, 16, thr, metric="half", path="nee", strategy="mis")
    assert (sc.stat("nee_family"), sc.stat("nee_form")) == (FAMILY, 2 | int(sky))
    counts = sc.sample_counts().reshape(-1)
    cols, rnds = sc.read_colors(), sc.read_rnds()
    seen = sorted(set(int(c) for c in np.unique(counts)))
    assert set(seen) <= {4, 8, 16} and len(seen) >= 2, seen
    for k in seen:
        fresh = make()
        fresh.render_nee(k, "mis")
        sel = counts == k
        assert same_bits(cols[sel, :3], fresh.read_colors()[sel, :3]) and np.array_equal(rnds[sel], fresh.read_rnds()[sel]), k


def test_tiled_ranks_assemble_the_single_context_frame(api):
    W, H, world = 48, 36, 2
    one = corridor(api, W, H)
    one.render_nee(3, "mis")
    whole = state(one)
    off = corridor(api, W, H, tree=False)
    off.render_nee(3, "mis")
    assert off.stat("nee_family") == 0 and not same_bits(whole[0], off.read_colors())
    seen = np.zeros(W * H, dtype=bool)
    for r in range(world):
        sc = corridor(api, W, H, rank=r, world=world, rows_per_block=8)
        sc.render_nee(3, "mis")
        ids = sc.local_pixel_ids()
        assert same_state(state(sc), tuple(a[ids] for a in whole)), r
        seen[ids] = True
    assert seen.all()


# ---------------------------------------------------------------------------- 7: combined with the other branches
@pytest.mark.parametrize("what", ["env", "lights", "fog", "interior"])
def test_combined_keeps_the_mean(api, what):
    """Each by the rule of 4 (not the float64 model): the option-on block means of many_lights(16) equal the option-off ones within five
    standard errors, under MIS, with a sky (P_env), with a point light in the corridor (P_ana), with bounded fog (its scatter vertices
    cull nothing) and with a tinted glass pane across the corridor (a live interior binding: flags bit 7)."""
    from opencl_path_tracer_amd import scenes
    W = H = 32
    spec = scenes.many_lights(16)
    if what == "interior":
        spec.materials.append(scenes.BUILTIN_MATERIALS[scenes.GLASS])
        z = 12.0
        pane = []
        for zz, flip in ((z, False), (z + 0.5, True)):
            a, b, c, d = (-2.0, -1.5, zz), (2.0, -1.5, zz), (2.0, 1.5, zz), (-2.0, 1.5, zz)
            pane += [(a, c, b), (a, d, c)] if flip else [(a, b, c), (a, c, d)]
        spec.objects.append((np.asarray(pane, dtype=np.float32), np.full(4, 3, dtype=np.uint16)))

    def make():
        sc = api.Scene(W, H).load(spec)
        if what == "env":
            sc.set_environment(scenes.sun_and_sky())
        if what == "lights":
            sc.set_lights([api.point_light((0.0, 0.0, 6.0), (30.0, 30.0, 30.0))], select=0.4)
        if what == "fog":
            sc.set_medium(0.05, albedo=(0.9, 0.9, 0.9), g=0.3, bounds=((-2.0, -1.5, -1.0), (2.0, 1.5, 50.0)))
        if what == "interior":
            sc.set_material_interior(3, sigma_a=(0.2, 0.6, 1.0))
        return sc
    probe = make()
    probe.set_option("light_tree", 1)
    probe.iterations = BOUNCES
    probe.render_nee(1, "mis")
    assert probe.stat("nee_family") == FAMILY and probe.stat("nee_form") == (1 if what == "env" else 0)
    probe.close()
    check_same_mean(make, W, H, "mis", seed=31, batches=128)
