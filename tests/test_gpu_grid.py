"""-m gpu: the medium's density grid of Scene.set_medium_density in Scene.render_nee and Scene.render_adaptive(path="nee")
(pt_set_medium_density, the grid instances of k_nee in pt_nee_grid.hip, grid_walk in pt_device.hpp, pt_debug_grid in pt_medium.hip;
include/pt_api.h pins the walk).

  1 pt_debug_grid against tests/grid_ref.py's float64 walk; 2 a 1 x 1 x 1 grid of 1 renders the homogeneous medium's bits; 3 strategies
  light and mis against grid_ref.GridModel on test_gpu_lights.py's replay scene; 4 closed form: absorption through two layers; 5 the
  four node modes render the same bits in every form; 6 adaptive tiles hold render_nee's bits."""

import numpy as np
import pytest

import grid_ref as GR
import nee_instances as I
import nee_ref as R
import test_gpu_lights as TL
import test_gpu_medium as TM
import test_gpu_nee_instances as TI

pytestmark = pytest.mark.gpu

same_bits, state, same_state = TL.same_bits, TL.state, TL.same_state
GRID_FAMILY = 9

# ---------------------------------------------------------------------------- 1: pt_debug_grid
# cells 2 x 1.5 x 0.5, all exact in float32, so a ray laid into a plane of the grid lies in it in both precisions
WALK_BOX = ((-1.0, 0.5, 2.0), (7.0, 5.0, 3.0))
WALK_SIGMA = 0.35
# the worst deviation measured on the MI355X, relative to the optical depth involved: 1.47e-5 for the optical depth (a clip 0.15 long
# that starts 8.4 from the origin: the float32 roundings of a and b), 3.6e-7 for -log T, 1.5e-7 for s (test 1's docstring).  WALK_TOL is
# at most four times that, and below the 1e-4 it may never exceed
WALK_MEASURED = 1.47e-5
WALK_TOL = 5.8e-5


def walk_density():
    rho = np.random.default_rng(3).uniform(0.2, 3.0, (2, 3, 4)).astype(np.float32)        # 4 x 3 x 2: an axis mix-up changes the answer
    rho[0, 1, 2] = 0.0
    rho[1, 2, 1] = 8.0
    return rho


def walk_items(lo, hi, n):
    """{P, D, t, u, limit, 0, 0, 0} per item, a few hundred: see the test's docstring"""
    lo, hi, n = np.asarray(lo), np.asarray(hi), np.asarray(n)
    cell = (hi - lo) / n
    rng = np.random.default_rng(7)
    items = []

    def add(P, D, t=np.inf, u=None, limit=np.inf):
        D = np.asarray(D, dtype=np.float64)
        items.append(list(P) + list(D / np.linalg.norm(D)) + [t, rng.random() if u is None else u, limit, 0.0, 0.0, 0.0])
    for _ in range(200):                                            # random: origins inside and outside, towards the box or anywhere
        P = rng.uniform(lo - 2.0, hi + 2.0) if rng.random() < 0.6 else rng.uniform(lo, hi)
        D = rng.uniform(lo, hi) - P if rng.random() < 0.7 else rng.normal(size=3)
        add(P, D, np.inf if rng.random() < 0.4 else rng.uniform(0.3, 9.0), None, np.inf if rng.random() < 0.4 else rng.uniform(0.3, 9.0))
    for ax in range(3):                                             # parallel to one axis (two zero components), both ways, in and out
        for sign in (1.0, -1.0):
            for _ in range(4):
                P = rng.uniform(lo - 1.0, hi + 1.0)
                P[ax] = lo[ax] - 1.0 if sign > 0 else hi[ax] + 1.0
                add(P, sign * np.eye(3)[ax])
            add(rng.uniform(lo, hi), sign * np.eye(3)[ax], rng.uniform(0.5, 3.0))
    for ax in range(3):                                             # one zero component: parallel to one pair of planes
        for _ in range(6):
            D = rng.normal(size=3)
            D[ax] = 0.0
            add(rng.uniform(lo - 1.0, hi + 1.0), D)
    for _ in range(24):                                             # through a vertex of the grid, and through a point of an edge
        k = np.array([rng.integers(0, n[0] + 1), rng.integers(0, n[1] + 1), rng.integers(0, n[2] + 1)])
        X = lo + k * cell
        if rng.random() < 0.5:
            ax = int(rng.integers(0, 3))
            X[ax] = rng.uniform(lo[ax], hi[ax])
        P = rng.uniform(lo - 2.0, hi + 2.0)
        add(P, X - P)
    for ax in range(3):                                             # lying in a plane of the grid: the box's faces and an inner plane
        for k in (0, 1, int(n[ax])):
            if k > n[ax]:
                continue
            for _ in range(3):
                P = rng.uniform(lo - 1.0, hi + 1.0)
                P[ax] = lo[ax] + k * cell[ax]
                D = rng.uniform(lo, hi) - P
                D[ax] = 0.0
                add(P, D)
    for _ in range(12):                                             # t shorter than the box: ends in the first voxels
        P = rng.uniform(lo, hi)
        add(P, rng.normal(size=3), rng.uniform(0.05, 0.6), None, rng.uniform(0.05, 0.6))
    for u in (0.0, 2.0 ** -24, 3.0 * 2.0 ** -24, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -23):       # u near 0 and near 1
        for _ in range(4):
            P = rng.uniform(lo - 1.0, hi + 1.0)
            add(P, rng.uniform(lo, hi) - P, np.inf, u)
    return np.asarray(items, dtype=np.float32)


@pytest.mark.parametrize("dims", ["4x3x2", "1x1x1"])
def test_debug_grid_matches_the_float64_walk(api, cb_spec, dims):
    """pt_debug_grid on 335 items -- random rays from inside and outside the box, rays along an axis and with one zero component, rays
    through vertices and edges of the grid, rays lying in a face of the box and in an inner plane, t shorter than the box, limit =
    +inf, u = 0, 2^-24, 1 - 2^-24 -- against grid_ref.walk in float64 on the float32 inputs, on a 4 x 3 x 2 grid (one voxel 0, one 8)
    and on a 1 x 1 x 1 grid.  Compared: the optical depth over [0, t]; T over [0, limit], as -log T; s where both scatter, as the depth
    |s - s64| sigma(voxel) it stands for; each relative to the optical depth involved (the whole depth; tau).  Two of them have a floor
    that the number format sets, not the walk: s itself is a float32 (4e-7 |s|, as depth), and T is one next to 1 (2e-7 in -log T: expf
    within 1 ulp and T's own rounding).
    The scatter flag and the voxel agree wherever the float64 margin |d - seg| / max(d, seg) of every voxel is at least
    grid_ref.SCATTER_MARGIN; the voxel count is within nx + ny + nz + 3 everywhere and the float64 walk's where no two planes are
    crossed together.  The worst deviation measured on the MI355X is WALK_MEASURED = 1.47e-5 of the optical depth (the depth itself;
    3.6e-7 for -log T, 1.5e-7 for s, above their floors); WALK_TOL = 5.8e-5 is just under four times that, and under the 1e-4 it may never
    exceed.  On the 1 x 1 x 1 grid of density 1 the outputs are also pt_debug_medium's, bit for bit."""
    lo, hi = WALK_BOX
    rho = walk_density() if dims == "4x3x2" else np.ones((1, 1, 1), dtype=np.float32)
    n = rho.shape[::-1]
    sc = api.Scene(16, 16).load(cb_spec)
    sc.set_medium(WALK_SIGMA, albedo=0.5, g=0.0, bounds=WALK_BOX)
    sc.set_medium_density(rho)
    items = walk_items(lo, hi, n)
    out = sc.debug_grid(items).astype(np.float64)
    assert np.isfinite(out[:, 2:]).all() and len(items) > 300
    sig = float(np.float32(WALK_SIGMA))
    flat = rho.reshape(-1).astype(np.float64)
    worst = dict(depth=0.0, T=0.0, s=0.0)
    scattered = decided = crossed = 0
    bound = sum(n) + 3
    for it, o in zip(items.astype(np.float64), out):
        P, D, t, u, limit = it[0:3], it[3:6], it[6], it[7], it[8]
        tau = -np.log1p(-u)
        full = GR.walk(sig, rho, lo, hi, P, D, t, np.inf)
        fl = GR.walk(sig, rho, lo, hi, P, D, t, tau)
        thr = GR.walk(sig, rho, lo, hi, P, D, limit, np.inf)
        assert 0 <= o[6] <= bound and o[6] == int(o[6]), (it, o)
        assert (o[2] == 1.0) == (o[7] >= 0.0) == (o[3] >= 0.0) and -1 <= o[7] < flat.size
        if full["near_clip"] or thr["near_clip"]:
            continue
        if not max(full["b"] - full["a"], 0.0) > 0.0:
            assert o[4] == 0.0 and o[2] == 0.0 and o[6] == 0.0 and o[3] == -1.0
        else:
            crossed += 1
            assert abs(o[0] - full["a"]) <= 4e-7 * abs(full["a"]) + 1e-30 and abs(o[1] - full["b"]) <= 4e-7 * abs(full["b"])
            err = abs(o[4] - full["acc"])
            assert err <= WALK_TOL * full["acc"], (it, o[4], full["acc"])
            worst["depth"] = max(worst["depth"], err / max(full["acc"], 1e-30))
            if fl["margin"] >= GR.SCATTER_MARGIN:
                decided += 1
                assert o[2] == float(fl["scatter"]), (it, o, fl["margin"])
                if not fl["near"]:
                    assert o[7] == fl["voxel"] and o[6] == fl["visited"], (it, o, fl["voxel"], fl["visited"])
            if o[2] == 1.0 and fl["scatter"]:
                scattered += 1
                sv = sig * flat[fl["voxel"]]
                err = abs(o[3] - fl["s"]) * sv
                assert err <= WALK_TOL * tau + 4e-7 * abs(fl["s"]) * sv, (it, o[3], fl["s"])
                worst["s"] = max(worst["s"], max(err - 4e-7 * abs(fl["s"]) * sv, 0.0) / max(tau, 1e-30))
                assert o[0] <= o[3] <= o[1]
        if not max(thr["b"] - thr["a"], 0.0) > 0.0:
            assert o[5] == 1.0
        else:
            assert 0.0 <= o[5] <= 1.0
            if thr["acc"] < 80.0:                                     # (beyond that T is a float32 denormal or 0)
                err = abs(-np.log(o[5]) - thr["acc"])
                assert err <= WALK_TOL * thr["acc"] + 2e-7, (it, o[5], thr["acc"])
                worst["T"] = max(worst["T"], max(err - 2e-7, 0.0) / max(thr["acc"], 1e-30))
    print("pt_debug_grid %s: worst deviation relative to the optical depth: %s; %d of %d items cross the box, "
          "%d decided, %d scatter" % (dims, {k: float(v) for k, v in worst.items()}, crossed, len(items), decided, scattered))
    assert crossed > 200 and decided > 200 and scattered > 60
    if dims == "1x1x1":                                              # the homogeneous medium's own numbers, bit for bit
        med = items.copy()
        med[:, 8:] = 0.0
        med[:, 10] = items[:, 8]
        hom = sc.debug_medium(med)
        got = sc.debug_grid(items)
        assert same_bits(got[:, 0:2], hom[:, 0:2]) and np.array_equal(got[:, 2], hom[:, 2]) and same_bits(got[:, 5], hom[:, 8])
        sel = got[:, 2] == 1.0
        assert sel.sum() > 60 and same_bits(got[sel, 3], (hom[sel, 0] + hom[sel, 3]).astype(np.float32))       # s = a + d, one float32 addition


# ---------------------------------------------------------------------------- 2: a unit grid is the homogeneous medium
@pytest.mark.parametrize("sky", [False, True])
def test_a_unit_grid_renders_the_homogeneous_mediums_bits(api, sky):
    """scenes.cornell_box(fog=1e-3) at 52 x 36, 2 spp, 4 bounces, strategy mis: with a 1 x 1 x 1 grid of 1.0 the grid instances launch
    (stat nee_family 9 against 8) and colours, rnds and rays are the frame's without a grid, bit for bit; so are they again once the
    grid is cleared."""
    from opencl_path_tracer_amd import scenes
    W, H = I.FRAME
    frames = []
    for grid in (False, True):
        sc = api.Scene(W, H).load(scenes.cornell_box(fog=1e-3))
        if sky:
            sc.set_environment(scenes.sun_and_sky())
        if grid:
            sc.set_medium_density(np.ones((1, 1, 1), dtype=np.float32))
        sc.iterations = 4
        sc.render_nee(2, "mis")
        assert (sc.stat("nee_family"), sc.stat("nee_form")) == (GRID_FAMILY if grid else 8, int(sky))
        frames.append(state(sc))
        if grid:
            sc.clear_medium_density()
            sc.current_sample = 0
            sc.seed_default()
            sc.render_nee(2, "mis")
            assert sc.stat("nee_family") == 8
            frames.append(state(sc))
    assert same_state(frames[0], frames[1]) and same_state(frames[0], frames[2])
    assert np.isfinite(frames[0][0]).all() and frames[0][0][:, :3].mean() > 0.0


# ---------------------------------------------------------------------------- 3: replay against the float64 model
# test_gpu_medium.py's bounded fog in test_gpu_lights.py's replay room (the eye at the origin looks along +z; the box spans z in [0.5, 11.5])
# as a 5 x 4 x 3 grid: thin fog (1) in front, an empty slab across the middle third of the depth, and behind it half-density fog with a
# dense blob (6) of 2 x 2 voxels in the middle
GRID_FOG = dict(TM.FOG)


def replay_density():
    rho = np.ones((3, 4, 5), dtype=np.float32)
    rho[1] = 0.0
    rho[2] = 0.5
    rho[2, 1:3, 1:3] = 6.0
    return rho


def grid_replay_scene(api, sky, device=0):
    sc, spec, rgb = TL.replay_scene(api, sky, device=device)
    sc.set_medium(**GRID_FOG)
    sc.set_medium_density(replay_density())
    return sc, spec, rgb


def grid_replay_model(api, sc, spec, rgb, sky):
    verts, mo = spec.objects[0]
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    env = dict(rgb=rgb, tables=sc.debug_environment(), scale=TL.REPLAY["scale"], yaw_degrees=TL.REPLAY["yaw_degrees"]) if sky else None
    return GR.GridModel(verts, recs["N"], mats, mo, sc.camera[0], sc.debug_lights(), sc.medium(), env=env, table=sc.debug_light_table(),
                        density=sc.medium_density(), dense_from=6.0)


@pytest.mark.parametrize("strategy", ["light", "mis"])
def test_matches_float64_model(api, strategy):
    """test_gpu_lights.py's replay scene (48 x 32, 2 spp, 4 bounces, its three lights, no sky) in the 5 x 4 x 3 grid of replay_density()
    under test_gpu_medium.check_replay: its tolerance and its 10 % cap on near ties, to which grid_ref.GridModel adds the segments whose
    scatter decision in some voxel falls within its margin and those that cross two planes together.
    The model alone, on these seeds (host-only context, before the first GPU run), flags 0.59 % of the 1,536 pixels (9) as near ties in
    both strategies.  In the kept pixels, in either strategy: 3,021 scatter vertices, 1,728 of them in voxels of density below 6 (the
    thin fog in front and the half-density fog behind the slab) and 1,293 in the dense blob; 4,171 free flights cross the empty slab
    with fog before or after it on their way; 1,882 light samples at a scatter vertex reach their light (618 a delta light's), and
    4,118 light samples in all pass through at least two voxels of fog with 0 < T < 1.  The model takes 7 to 11 s of CPU time per
    strategy."""
    sc, spec, rgb = grid_replay_scene(api, False)
    seeds = TL.replay_seeds()
    sc.upload_seeds(seeds)
    sc.iterations = TL.REPLAY["bounces"]
    sc.render_nee(TL.REPLAY["spp"], strategy)
    assert sc.stat("nee_family") == GRID_FAMILY
    model = grid_replay_model(api, sc, spec, rgb, False)
    assert model.pa == 0.5 and model.density.shape == (3, 4, 5) and model.medium["sigma_t"] == float(np.float32(GRID_FOG["sigma_t"]))
    need = ("scatter", "scatter_light", "scatter_delta", "delta", "grid_scatter_thin", "grid_scatter_dense", "grid_empty_crossed", "grid_light_partial")
    TM.check_replay(sc, model, seeds, api.NEE_STRATEGIES[strategy], need)


# ---------------------------------------------------------------------------- 4: closed form
@pytest.mark.parametrize("layers", [(0.5, 3.0), (3.0, 0.5)], ids=["thin_first", "dense_first"])
def test_absorption_through_two_layers(api, layers):
    """test_gpu_medium.py's absorption case through two layers along the view axis: the emitter at z = 20 seen through the box z in
    [5, 12], a 1 x 1 x 2 grid of densities (rho1, rho2), albedo 0, strategy bsdf, iterations = 2, one sample per pixel at 96 x 64.  Ray i
    crosses each layer over l_i = 3.5 / D_z, so it reaches the emitter with probability p_i = exp(-sigma_t (rho1 + rho2) l_i) and is then
    worth v_i = 2 Le cos_i, else 0: the frame mean has expectation (1 / n) sum v_i p_i and variance (1 / n^2) sum v_i^2 p_i (1 - p_i), and
    the tolerance is five of those standard deviations per channel, as there.  Swapping the layers leaves every p_i as it was.  The
    survivors are then the same rays too, but for a ray whose tau lies within a rounding of its depth: the two orders sum the same two
    products, so they differ by 1e-7 of the depth at most, and a tie that close has probability 6,144 x 1e-7: none is allowed."""
    W, H = 96, 64
    spec = TM.emitter_spec()
    sigma = 0.05
    bounds = ((-40.0, -40.0, 5.0), (40.0, 40.0, 12.0))
    sc = api.Scene(W, H).load(spec)
    seeds = np.random.default_rng(23).integers(1, 2 ** 31 - 2, W * H).astype(np.int32)
    verts, mo = spec.objects[0]
    model = R.Model(verts, api.triangles_from_vertices(verts, mo)["N"], np.concatenate([api.Material(*m) for m in spec.materials]), mo, sc.camera[0])
    v, p = np.zeros((W * H, 3)), np.zeros(W * H)
    for i in range(W * H):
        s, r1 = R.lcg(int(seeds[i]))
        s, r2 = R.lcg(s)
        P, D = model.camera_ray(i, r1, r2)
        assert abs(P[0] + D[0] * 12.0 / D[2]) < 40.0 and abs(P[1] + D[1] * 12.0 / D[2]) < 40.0          # the ray leaves through z = 12
        v[i] = 2.0 * np.asarray(TM.LE) * D[2]
        p[i] = np.exp(-sigma * (layers[0] + layers[1]) * 3.5 / D[2])
    frames = []
    for rho in (layers, layers[::-1]):
        sc.set_medium(sigma, albedo=0.0, g=0.3, bounds=bounds)
        sc.set_medium_density(np.asarray(rho, dtype=np.float32).reshape(2, 1, 1))
        sc.current_sample = 0
        sc.upload_seeds(seeds)
        sc.iterations = 2
        sc.render_nee(1, "bsdf")
        assert sc.stat("nee_family") == GRID_FAMILY
        frames.append(sc.read_colors()[:, :3].astype(np.float64))
    got = frames[0]
    reached = got.any(axis=1)
    assert np.allclose(got[reached], v[reached], rtol=1e-5)          # a sample is worth v_i or nothing
    want = (v * p[:, None]).mean(axis=0)
    sd = np.sqrt((v * v * (p * (1.0 - p))[:, None]).sum(axis=0)) / (W * H)
    print("absorption %s: mean %s, expected %s, standard deviation %s, survivors %.3f (expected %.3f)" % (layers, got.mean(axis=0), want, sd, reached.mean(), p.mean()))
    assert 0.2 < p.mean() < 0.9
    assert (np.abs(got.mean(axis=0) - want) <= 5.0 * sd).all()
    assert np.array_equal(frames[1].any(axis=1), reached) and np.array_equal(frames[1], got)      # swapped: the same transmittance, ray by ray


# ---------------------------------------------------------------------------- 5: node modes
def grid_block(mode):
    """the 512-thread rule (launch_lanes_wide): every form of the family takes it"""
    return {0: 512, 1: 256, 2: 512, 3: 256}[mode]


@pytest.mark.parametrize("form", range(4), ids=I.FORMS)
def test_node_modes_render_the_same_bits(api, form):
    """nee_instances.build's small and mesh scenes in the `medium` configuration (every feature live) with scenes.smoke_plume(8) on top:
    on small, modes 0, 1, 3 and 3 with an overflowing stack, on mesh modes 1, 2 and 3 render one frame bit for bit; after each render
    stats nee_family, nee_form, nee_block and node_mode are the grid family's cell; and the frame is not the one of the same configuration
    without a grid."""
    from opencl_path_tracer_amd import scenes
    plume = scenes.smoke_plume(8)
    for scene, first in (("small", "lds"), ("mesh", "treelet")):
        frames, thr, modes = {}, None, set()
        for placement in I.PLACEMENTS[scene]:
            sc, mode = I.build(api, scene, "medium", placement, sky=bool(form & 1))
            sc.set_medium_density(plume)
            if form & 2 and thr is None:
                sc.iterations = TL.CB_BOUNCES
                thr = TI.threshold_of(sc)
            frames[placement] = TI.render(sc, form, thr)
            got = tuple(int(sc.stat(k)) for k in ("node_mode", "nee_family", "nee_form", "nee_block"))
            assert got == (mode, GRID_FAMILY, form, grid_block(mode)), (scene, placement, got)
            modes.add(mode)
            sc.close()
        assert modes == ({0, 1, 3} if scene == "small" else {1, 2, 3})
        want = frames[first]
        assert np.isfinite(want[0]).all() and want[0][:, :3].mean() > 0.0, scene
        if form & 2:
            seen = sorted(set(int(c) for c in np.unique(want[2])))
            assert set(seen) <= {4, 8, 16} and len(seen) >= 2, (scene, seen)
        for placement, got in frames.items():
            assert TI.same_frames(got, want), (I.FORMS[form], scene, placement)
        assert not same_bits(want[0], TI.reference_frame(api, scene, "medium", form)), scene


# ---------------------------------------------------------------------------- 6: adaptive
@pytest.mark.parametrize("sky", [False, True])
def test_adaptive_nee_tiles_hold_render_nee_bits(api, sky):
    """test_gpu_medium.py's check with scenes.smoke_plume(8) in its fogged box: k_nee_tiles_grid / k_nee_env_tiles_grid retire tiles, and a
    tile retired at k samples holds render_nee's bits at k samples (36 x 20: ragged tiles on the right and at the bottom)"""
    from opencl_path_tracer_amd import scenes
    W, H = 36, 20

    def box():
        sc = TM.fog_box(api, W, H, sky)
        sc.set_medium_density(scenes.smoke_plume(8))
        return sc
    sc = box()
    thr = TI.threshold_of(sc)
    sc.render_adaptive(4, 16, thr, metric="half", path="nee", strategy="mis")
    assert (sc.stat("nee_family"), sc.stat("nee_form")) == (GRID_FAMILY, 2 | int(sky))
    counts = sc.sample_counts().reshape(-1)
    cols, rnds = sc.read_colors(), sc.read_rnds()
    seen = sorted(set(int(c) for c in np.unique(counts)))
    assert set(seen) <= {4, 8, 16} and len(seen) >= 2, seen
    for k in seen:
        fresh = box()
        fresh.render_nee(k, "mis")
        sel = counts == k
        assert same_bits(cols[sel, :3], fresh.read_colors()[sel, :3]) and np.array_equal(rnds[sel], fresh.read_rnds()[sel]), k
