"""-m gpu: smooth shading from vertex normals in Scene.render_nee (option smooth_normals; pt_smooth.hip, the smooth k_nee instances of
pt_nee.hip; include/pt_api.h pins the estimator).

  * the option without vertex normals (never set, or set and cleared) is a no-op bit for bit, in every node mode;
  * the interpolated normal of Scene.debug_shading_normals against numpy's float64 evaluation of the pinned formula;
  * the other render paths refuse while the option is on and render the oracle's bits once it is off again;
  * MIS frames, with and without an environment, against tests/smooth_ref.py (float64, brute force, same LCG and hashes);
  * adaptive NEE frames: a tile retired after k samples holds render_nee(k)'s bits; determinism."""

import numpy as np
import pytest

import smooth_ref as S

pytestmark = pytest.mark.gpu

CB_BOUNCES = 4
EYE_AT_ORIGIN = (-500.0, -500.0, 1299.0378)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def state(sc):
    rays = sc.read_rays()
    return sc.read_colors().copy(), sc.read_rnds().copy(), rays["P"][:, :3].copy(), rays["D"][:, :3].copy()


def same_state(a, b):
    return same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2]) and same_bits(a[3], b[3])


# ---------------------------------------------------------------------------- 1: no normals, no change
@pytest.mark.parametrize("lds,wide,mode", [(2, 1, 0), (0, 1, 1), (2, 2, 3)])
def test_option_without_normals_is_a_noop(api, oracle, cb_spec, cb_oracle_scene, lds, wide, mode):
    from opencl_path_tracer_amd import scenes
    W, H, spp = 64, 48, 3
    cam = oracle.make_camera(cb_spec.fov, cb_spec.yaw, cb_spec.pitch, cb_spec.shift, W, H)
    fr = oracle.OracleFrame(W, H)
    fr.render(cb_oracle_scene, cam, CB_BOUNCES, 0, spp, nthreads=16)

    def scene(smooth, set_and_clear=False):
        sc = api.Scene(W, H)
        sc.set_option("wide_nodes", wide)
        sc.load(cb_spec)
        sc.set_option("lds_scene", lds)
        assert sc.stat("node_mode") == mode
        if set_and_clear:
            sc.set_vertex_normals(scenes.uv_sphere_normals((250.0, 200.0, 300.0), 200.0), first=12)
            assert sc.debug_vertex_normals()[1].sum() == 960
            sc.clear_vertex_normals()
        sc.set_option("smooth_normals", smooth)
        sc.iterations = CB_BOUNCES
        return sc

    for strategy in ("bsdf", "mis"):
        off = scene(0)
        off.render_nee(spp, strategy)
        want = state(off)
        if strategy == "bsdf":
            assert same_bits(want[0][:, :3], fr.colors()[:, :3]) and np.array_equal(want[1], fr.rnds())
        for set_and_clear in (False, True):
            on = scene(1, set_and_clear)
            on.render_nee(spp, strategy)
            assert same_state(state(on), want), (strategy, set_and_clear)


# ---------------------------------------------------------------------------- 2: the interpolation
SPHERE_C, SPHERE_R = (0.5, -0.25, 6.0), 2.0


def sphere_in_walls(api):
    from opencl_path_tracer_amd import scenes
    mats = [((0.6, 0.6, 0.6), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0)]

    def quad(a, b, c, d):
        return [(a, b, c), (a, c, d)]
    x0, x1, y0, y1, z0, z1 = -6.0, 6.0, -4.0, 5.0, -2.0, 12.0
    walls = (quad((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)) + quad((x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)) +
             quad((x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)) + quad((x1, y0, z0), (x1, y1, z0), (x1, y1, z1), (x1, y0, z1)))
    sph = scenes.uv_sphere(SPHERE_C, SPHERE_R, 8, 4)
    spec = scenes.SceneSpec(materials=mats, shift=EYE_AT_ORIGIN, name="sphere_in_walls")
    spec.objects.append((np.asarray(walls, dtype=np.float32), np.zeros(len(walls), dtype=np.uint16)))
    spec.objects.append((sph, np.zeros(len(sph), dtype=np.uint16)))
    spec.normals = [None, scenes.uv_sphere_normals(SPHERE_C, SPHERE_R, 8, 4)]
    return spec


def hashed_rays(api, n):
    rng = np.random.default_rng(23)
    rays = np.zeros(n, dtype=api.RAY)
    P = rng.uniform(-0.5, 0.5, (n, 3)) + np.array([0.0, 0.5, 0.0])
    target = np.asarray(SPHERE_C) + rng.uniform(-2.2, 2.2, (n, 3))          # about half of the rays meet the sphere, the rest a wall or nothing
    D = target - P
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    rays["P"][:, :3] = P
    rays["D"][:, :3] = D
    return rays


@pytest.mark.parametrize("opts,mode", [({}, 0), ({"lds_scene": 0}, 1), ({"wide_nodes": 2}, 3)])
def test_interpolated_normal_matches_float64_formula(api, opts, mode):
    """Whole tree in LDS, nodes from global memory, 4-wide nodes (a treelet needs a tree too large for LDS: the adaptive test below)."""
    spec = sphere_in_walls(api)
    sc = api.Scene(32, 32)
    for k, v in opts.items():
        if k != "lds_scene":
            sc.set_option(k, v)
    sc.load(spec)
    if "lds_scene" in opts:
        sc.set_option("lds_scene", opts["lds_scene"])
    assert sc.stat("node_mode") == mode
    rays = hashed_rays(api, 4096)
    t_ref, tri_ref = sc.debug_closest_hit(rays)
    tri, ns = sc.debug_shading_normals(rays)
    assert np.array_equal(tri, tri_ref) and same_bits(ns[:, 3], t_ref)
    recs = api.triangles_from_vertices(np.concatenate([v for v, _ in spec.objects]), np.zeros(spec.ntris, dtype=np.uint16))
    nwall = spec.objects[0][0].shape[0]
    vn = np.zeros((spec.ntris, 3, 3), dtype=np.float32)
    vn[nwall:] = spec.normals[1]
    got_vn, has = sc.debug_vertex_normals()
    assert same_bits(got_vn, vn) and has[nwall:].all() and not has[:nwall].any()
    packed = S.unit64(vn[nwall:])
    verts = np.concatenate([v for v, _ in spec.objects]).astype(np.float64)
    worst, on_sphere, ang_s, ang_g = 0.0, 0, [], []
    for i in range(len(rays)):
        k = int(tri[i])
        if k < 0:                                             # through the open top or front: a miss
            assert same_bits(ns[i], np.array([0.0, 0.0, 0.0, -1.0], dtype=np.float32)), i
            continue
        P, D = rays["P"][i, :3].astype(np.float64), rays["D"][i, :3].astype(np.float64)
        N = recs["N"][k, :3]
        Ng32 = -N if np.float32(np.dot(D, N.astype(np.float64))) > 0 else N
        if k < nwall:                                         # a wall has no vertex normals: Ng's bits
            assert same_bits(ns[i, :3], Ng32), i
            continue
        hp = P + D * float(ns[i, 3])
        want, used, near = S.shading_normal(verts[k], N.astype(np.float64), packed[k - nwall], True, D, hp)
        if near or not used:
            continue
        on_sphere += 1
        worst = max(worst, float(np.abs(ns[i, :3].astype(np.float64) - want).max()))
        radial = (hp - np.asarray(SPHERE_C)) / np.linalg.norm(hp - np.asarray(SPHERE_C))
        dev = ns[i, :3].astype(np.float64)
        ang_s.append(np.degrees(np.arccos(np.clip(dev @ radial / np.linalg.norm(dev), -1, 1))))
        g = Ng32.astype(np.float64)
        ang_g.append(np.degrees(np.arccos(np.clip(g @ radial / np.linalg.norm(g), -1, 1))))
    print("largest |Ns - float64 formula| = %.3g over %d hits; mean angle to the radial direction: Ns %.3f deg, Ng %.3f deg"
          % (worst, on_sphere, np.mean(ang_s), np.mean(ang_g)))
    # measured on an MI355X: 1.53e-7 over 2,453 hits (a few ulp of a normalised component: the float32 rounding of t moves hp by up to
    # 2^-24 |hp|, the weights and the sum add a few roundings more); the bound is 4 x that
    assert on_sphere > 1000
    assert worst <= 6e-7
    assert np.mean(ang_s) < 0.25 * np.mean(ang_g)


# ---------------------------------------------------------------------------- 3: gating
def test_other_paths_refuse_while_the_option_is_on(api, oracle, cb_spec, cb_oracle_scene):
    W, H = 48, 32
    sc = api.Scene(W, H).load(cb_spec)
    sc.iterations = CB_BOUNCES
    sc.set_option("smooth_normals", 1)
    for call in (lambda: sc.render(1), lambda: sc.trace_rays(), lambda: sc.generate_rays(), lambda: sc.render_adaptive(2, 4, 0.1),
                 lambda: sc.render_adaptive(2, 4, 0.1, path="render")):
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_EINVAL and "smooth_normals" in str(e.value)
    sc.set_option("variant", 1)
    with pytest.raises(api.PtError) as e:
        sc.render(1)
    assert e.value.code == api.PT_EINVAL and "smooth_normals" in str(e.value)
    sc.set_option("variant", 0)
    sc.set_option("smooth_normals", 0)
    sc.render(2)
    cam = oracle.make_camera(cb_spec.fov, cb_spec.yaw, cb_spec.pitch, cb_spec.shift, W, H)
    fr = oracle.OracleFrame(W, H)
    fr.render(cb_oracle_scene, cam, CB_BOUNCES, 0, 2, nthreads=16)
    assert same_bits(sc.read_colors()[:, :3], fr.colors()[:, :3]) and np.array_equal(sc.read_rnds(), fr.rnds())


# ---------------------------------------------------------------------------- 4: the float64 model
REPLAY = dict(W=48, H=32, spp=2, bounces=4)
SPHERES = [((-2.6, -1.6, 7.0), 1.4, 0), ((0.3, -1.5, 9.6), 1.5, 5), ((2.7, -1.7, 6.2), 1.3, 6)]      # (centre, radius, material)


def replay_spec():
    """tests/test_gpu_nee.py's replay_spec (rebuilt here) plus three 8 x 4 spheres with analytic normals: diffuse, chromium, glass"""
    from opencl_path_tracer_amd import scenes
    mats = [
        ((0.6, 0.6, 0.6), (0.2, 0.2, 0.2), (0, 0, 0), (0, 0, 0), (0, 0, 0), 20.0, 0),      # 0 white, glossy lobe
        ((0.6, 0.1, 0.1), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),             # 1 red
        ((0.1, 0.6, 0.1), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),             # 2 green
        ((0, 0, 0), (0, 0, 0), (6.0, 5.0, 4.0), (0, 0, 0), (0, 0, 0), 0.0, 3),             # 3 lamp
        ((0, 0, 0), (0, 0, 0), (12.0, 4.0, 2.0), (0, 0, 0), (0, 0, 0), 0.0, 3),            # 4 small hot emitter
        scenes.BUILTIN_MATERIALS[scenes.CHROMIUM],                                           # 5 mirror
        scenes.BUILTIN_MATERIALS[scenes.GLASS],                                              # 6 glass
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
    spec = scenes.SceneSpec(materials=mats, name="smooth_replay", shift=EYE_AT_ORIGIN)
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.asarray(mo, dtype=np.uint16)))
    spec.normals = [None]
    for c, r, m in SPHERES:
        v = scenes.uv_sphere(c, r, 8, 4)
        spec.objects.append((v, np.full(len(v), m, dtype=np.uint16)))
        spec.normals.append(scenes.uv_sphere_normals(c, r, 8, 4))
    return spec


def replay_model(api, sc, spec, env=None):
    verts = np.concatenate([v for v, _ in spec.objects])
    mo = np.concatenate([m for _, m in spec.objects])
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    vn = np.concatenate([np.zeros(v.shape, dtype=np.float32) if n is None else n for (v, _), n in zip(spec.objects, spec.normals)])
    return S.SmoothModel(verts, recs["N"], mats, mo, sc.camera[0], vn, env=env, table=sc.debug_light_table())


@pytest.mark.parametrize("sky", [False, True])
def test_mis_matches_float64_model(api, sky):
    """Near-tie share of the model alone on these seeds, measured on the CPU before the first GPU run: 1.1 % without, 1.2 % with the
    sky (cap 10 %); events in the kept pixels without / with the sky: specular fall-backs 60 / 60, lobe terminations 9 / 10, light
    samples rejected by Ng alone 30 / 39."""
    from opencl_path_tracer_amd import scenes
    W, H, spp, bounces = REPLAY["W"], REPLAY["H"], REPLAY["spp"], REPLAY["bounces"]
    spec = replay_spec()
    sc = api.Scene(W, H).load(spec)
    env = None
    if sky:
        rgb = scenes.sun_and_sky()
        sc.set_environment(rgb)
        env = dict(rgb=rgb, tables=sc.debug_environment())
    sc.set_option("smooth_normals", 1)
    seeds = sc.read_rnds().copy()
    sc.iterations = bounces
    sc.render_nee(spp, "mis")
    model = replay_model(api, sc, spec, env)
    want, want_seeds, ties = model.render(seeds, bounces, spp, 2)
    got = sc.read_colors()[:, :3].astype(np.float64)
    keep = ~ties
    assert keep.mean() > 0.9, "too many near-tie pixels: %d" % int(ties.sum())
    for name, per_pixel in model.pixel_events.items():
        assert int(per_pixel[keep].sum()) > 0, name
    assert np.array_equal(sc.read_rnds()[keep], want_seeds[keep])
    scale = float(want[keep].max())
    err = np.abs(got[keep] - want[keep])
    bad = err > 2e-3 * np.abs(want[keep]) + 1e-6 * scale
    assert not bad.any(), "%d of %d pixel channels differ; worst %g" % (int(bad.sum()), bad.size, float((err / (np.abs(want[keep]) + 1e-6 * scale)).max()))
    assert float(want[keep].mean()) > 0.0
    # and the normals matter: the flat frame differs
    flat = api.Scene(W, H).load(spec)
    if sky:
        flat.set_environment(scenes.sun_and_sky())
    flat.iterations = bounces
    flat.render_nee(spp, "mis")
    assert not same_bits(flat.read_colors()[:, :3], sc.read_colors()[:, :3])


# ---------------------------------------------------------------------------- 5: adaptive NEE frames
@pytest.mark.parametrize("sky,opts,mode", [(False, {}, 0), (True, {}, 0), (True, {"lds_scene": 0}, 1), (True, {"treelet": 40, "wide_nodes": 1, "mesh": 1}, 2),
                                           (True, {"wide_nodes": 2}, 3)])
def test_adaptive_nee_tiles_hold_render_nee_bits(api, sky, opts, mode):
    """Without and with scenes.sun_and_sky() (k_nee_tiles_smooth / k_nee_env_tiles_smooth), the latter in every node mode; the treelet
    needs a tree too large for LDS: the 6,000-triangle mesh with computed vertex normals."""
    from opencl_path_tracer_amd import scenes
    W, H = 48, 32
    mesh = bool(opts.get("mesh"))
    spec = scenes.displaced_grid_mesh(6000) if mesh else replay_spec()

    def scene(smooth=1):
        c = api.Scene(W, H)
        for k, v in opts.items():
            if k not in ("lds_scene", "mesh"):
                c.set_option(k, v)
        c.load(spec)
        if "lds_scene" in opts:
            c.set_option("lds_scene", opts["lds_scene"])
        assert c.stat("node_mode") == mode
        if mesh:
            c.compute_vertex_normals(60.0, obj=1)
            assert c.debug_vertex_normals()[1][12:].all()
        if sky:
            c.set_environment(scenes.sun_and_sky())
        c.set_option("smooth_normals", smooth)
        return c
    sc = scene()
    sc.iterations = CB_BOUNCES
    # the threshold comes from the frame's own tile estimates: with threshold 0 nothing retires and tile_state() holds every tile's
    # estimate at the last decision (8 samples); their median retires about half of the tiles there and the quietest ones at 4
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
        fresh.iterations = CB_BOUNCES
        fresh.render_nee(k, "mis")
        sel = counts == k
        assert same_bits(cols[sel, :3], fresh.read_colors()[sel, :3]) and np.array_equal(rnds[sel], fresh.read_rnds()[sel]), k
    flat = scene(0)
    flat.iterations = CB_BOUNCES
    flat.render_nee(16, "mis")
    sel = counts == 16
    assert not same_bits(cols[sel, :3], flat.read_colors()[sel, :3])


# ---------------------------------------------------------------------------- 6: determinism
def test_determinism(api):
    W, H = 48, 32
    spec = replay_spec()
    a = api.Scene(W, H).load(spec)
    b = api.Scene(W, H).load(spec)
    for sc in (a, b):
        sc.set_option("smooth_normals", 1)
        sc.iterations = CB_BOUNCES
    a.render_nee(4, "mis")
    a.render_nee(4, "mis")
    b.render_nee(8, "mis")
    assert same_state(state(a), state(b))
