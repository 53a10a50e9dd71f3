"""-m gpu: albedo textures with uv coordinates in Scene.render_nee (option textures; pt_texture.hip, the textured k_nee instances of
pt_nee.hip; include/pt_api.h pins the lookup).

  * the option without textures, with a texture of exactly 1, and a constant texture against a scaled kd: no-ops bit for bit (colours,
    rnds, rays) in every node mode;
  * Scene.debug_albedo against numpy's float64 evaluation of the pinned lookup (tests/texture_ref.py), nearest exactly, bilinear to 1e-4;
  * MIS frames, with and without an environment, against tests/texture_ref.TextureModel;
  * rnds / rays do not depend on the textures; the preview of iterations == 1; the other render paths refuse while the option is on;
  * adaptive NEE frames hold render_nee's bits per retired tile; determinism."""

import os

import numpy as np
import pytest

import nee_ref as R
import texture_ref as T

pytestmark = pytest.mark.gpu

CB_BOUNCES = 4
EYE_AT_ORIGIN = (-500.0, -500.0, 1299.0378)
NODE_MODES = [(2, 1, 0), (0, 1, 1), (2, 2, 3)]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def state(sc):
    rays = sc.read_rays()
    return sc.read_colors().copy(), sc.read_rnds().copy(), rays["P"][:, :3].copy(), rays["D"][:, :3].copy()


def same_state(a, b):
    return same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2]) and same_bits(a[3], b[3])


def random_uvs(n, seed=3):
    return np.random.default_rng(seed).uniform(-2.0, 2.0, (n, 3, 2)).astype(np.float32)


# ---------------------------------------------------------------------------- 1: no-ops
@pytest.mark.parametrize("lds,wide,mode", NODE_MODES)
def test_option_without_textures_is_a_noop(api, oracle, cb_spec, cb_oracle_scene, lds, wide, mode):
    W, H, spp = 64, 48, 3
    cam = oracle.make_camera(cb_spec.fov, cb_spec.yaw, cb_spec.pitch, cb_spec.shift, W, H)
    fr = oracle.OracleFrame(W, H)
    fr.render(cb_oracle_scene, cam, CB_BOUNCES, 0, spp, nthreads=16)

    def scene(textures, uvs=False):
        sc = api.Scene(W, H)
        sc.set_option("wide_nodes", wide)
        sc.load(cb_spec)
        sc.set_option("lds_scene", lds)
        assert sc.stat("node_mode") == mode
        if uvs:                                                # uvs and a texture that no material is bound to
            sc.set_vertex_uvs(random_uvs(cb_spec.ntris))
            sc.add_texture(np.full((2, 2, 3), 0.25, dtype=np.float32))
        sc.set_option("textures", textures)
        sc.iterations = CB_BOUNCES
        return sc

    for strategy in ("bsdf", "mis"):
        off = scene(0)
        off.render_nee(spp, strategy)
        want = state(off)
        if strategy == "bsdf":
            assert same_bits(want[0][:, :3], fr.colors()[:, :3]) and np.array_equal(want[1], fr.rnds())
        for uvs in (False, True):
            on = scene(1, uvs)
            on.render_nee(spp, strategy)
            assert same_state(state(on), want), (strategy, uvs)


@pytest.mark.parametrize("lds,wide,mode", NODE_MODES)
@pytest.mark.parametrize("smooth", [0, 1])
def test_texture_of_one_is_a_noop(api, lds, wide, mode, smooth):
    """A 1 x 1 texture of exactly 1.0 bound to every material, uvs on every triangle: kd * 1 is kd.  With smooth_normals on the spheres
    carry their analytic normals, so the textured instances also run the interpolation of the smooth ones."""
    from opencl_path_tracer_amd import scenes
    W, H, spp = 64, 48, 3
    spec = scenes.cornell_box(smooth=bool(smooth))

    def scene(textures):
        sc = api.Scene(W, H)
        sc.set_option("wide_nodes", wide)
        sc.load(spec)
        sc.set_option("lds_scene", lds)
        assert sc.stat("node_mode") == mode
        if textures:
            t = sc.add_texture(np.ones((1, 1, 3), dtype=np.float32), filter=textures - 1)
            for m in range(len(spec.materials)):
                sc.set_material_texture(m, t)
            sc.set_vertex_uvs(random_uvs(spec.ntris))
            sc.set_option("textures", 1)
        sc.set_option("smooth_normals", smooth)
        sc.iterations = CB_BOUNCES
        return sc

    for strategy in ("bsdf", "mis"):
        off = scene(0)
        off.render_nee(spp, strategy)
        want = state(off)
        for filt in (1, 2):                                    # nearest, bilinear
            on = scene(filt)
            on.render_nee(spp, strategy)
            assert same_state(state(on), want), (strategy, filt)


@pytest.mark.parametrize("lds,wide,mode", NODE_MODES)
def test_constant_texture_equals_scaled_kd(api, lds, wide, mode):
    """kd = 1 with a constant-0.5 texture against an untextured kd = 0.5 (0.5 and 1 * 0.5 are exact; a bilinear blend of equal taps is the
    tap)."""
    from opencl_path_tracer_amd import scenes
    W, H, spp = 64, 48, 3

    def spec_with(kd):
        spec = scenes.cornell_box()
        m = list(spec.materials[scenes.WHITE_DIFFUSE])
        m[0] = (kd, kd, kd)
        spec.materials[scenes.WHITE_DIFFUSE] = tuple(m)
        return spec

    def scene(spec, textured):
        sc = api.Scene(W, H)
        sc.set_option("wide_nodes", wide)
        sc.load(spec)
        sc.set_option("lds_scene", lds)
        assert sc.stat("node_mode") == mode
        if textured:
            t = sc.add_texture(np.full((3, 2, 3), 0.5, dtype=np.float32), filter=textured - 1)
            sc.set_material_texture(scenes.WHITE_DIFFUSE, t)
            sc.set_vertex_uvs(random_uvs(spec.ntris))
            sc.set_option("textures", 1)
        sc.iterations = CB_BOUNCES
        return sc

    plain = scene(spec_with(0.5), 0)
    plain.render_nee(spp, "mis")
    want = state(plain)
    for filt in (1, 2):
        tex = scene(spec_with(1.0), filt)
        tex.render_nee(spp, "mis")
        assert same_state(state(tex), want), filt
    full = scene(spec_with(1.0), 0)
    full.render_nee(spp, "mis")
    assert not same_bits(state(full)[0], want[0])              # (and kd itself matters)


# ---------------------------------------------------------------------------- 2: the lookup
QUAD_UV = np.array([[(-0.7, -0.4), (2.3, -0.1), (2.6, 1.9)], [(-0.7, -0.4), (2.6, 1.9), (-0.5, 2.2)]], dtype=np.float32)
LOOKUP_KD = (0.8, 0.6, 0.4)


def lookup_spec():
    """a textured quad at z = 6 (uvs beyond [0, 1] and below 0) and three more triangles of bound materials that must keep their kd: a
    type-0 triangle without uvs, an emitter (type 3) and a mirror (type 1), both with uvs"""
    from opencl_path_tracer_amd import scenes
    mats = [
        (LOOKUP_KD, (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),
        ((0.3, 0.2, 0.1), (0, 0, 0), (5.0, 4.0, 3.0), (0, 0, 0), (0, 0, 0), 0.0, 3),
        ((0.15, 0.25, 0.35),) + tuple(scenes.BUILTIN_MATERIALS[scenes.CHROMIUM][1:]),
    ]
    a, b, c, d = (-2.0, -2.0, 6.0), (2.0, -2.0, 6.0), (2.0, 2.0, 6.0), (-2.0, 2.0, 6.0)
    tris = [(a, b, c), (a, c, d), ((3.0, -2.0, 6.0), (5.0, -2.0, 6.0), (4.0, 2.0, 6.0)), ((-5.0, -2.0, 6.0), (-3.0, -2.0, 6.0), (-4.0, 2.0, 6.0)),
            ((-2.0, 3.0, 6.0), (2.0, 3.0, 6.0), (0.0, 5.0, 6.0))]
    spec = scenes.SceneSpec(materials=mats, shift=EYE_AT_ORIGIN, name="lookup_quad")
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.asarray([0, 0, 0, 1, 2], dtype=np.uint16)))
    uv = np.full((5, 3, 2), np.nan, dtype=np.float32)
    uv[:2] = QUAD_UV
    uv[3] = uv[4] = QUAD_UV[0]
    spec.uvs = [uv]
    return spec


def lookup_rays(api, n=1000):
    rng = np.random.default_rng(29)
    rays = np.zeros(n, dtype=api.RAY)
    P = rng.uniform(-0.5, 0.5, (n, 3))
    target = np.stack([rng.uniform(-5.5, 5.5, n), rng.uniform(-2.5, 5.5, n), np.full(n, 6.0)], axis=1)
    target[:2 * n // 3, :2] = rng.uniform(-2.2, 2.2, (2 * n // 3, 2))              # two thirds at the quad and just around it
    D = target - P
    D /= np.linalg.norm(D, axis=1, keepdims=True)
    rays["P"][:, :3] = P
    rays["D"][:, :3] = D
    return rays


def lookup_texels():
    return np.random.default_rng(31).uniform(0.0, 1.0, (3, 5, 3)).astype(np.float32)            # 5 x 3: w = 5, h = 3


def lookup_model_hits(api, spec, rays, texels, filt):
    """per ray from the float64 model alone: (triangle or -1, tie in the intersection, kd' or None, near a lookup decision)"""
    verts = np.concatenate([v for v, _ in spec.objects])
    mo = np.concatenate([m for _, m in spec.objects])
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    model = R.Model(verts, recs["N"], mats, mo, api.Camera(spec.fov, spec.yaw, spec.pitch, spec.shift, 32, 32)[0])
    stored = texels.astype(np.float16).astype(np.float32)
    out = []
    for i in range(len(rays)):
        P, D = rays["P"][i, :3].astype(np.float64), rays["D"][i, :3].astype(np.float64)
        ti, t, tie = model.intersect(P, D)
        if ti < 0 or ti > 1:
            out.append((ti, tie, None, False))
            continue
        kd, near = T.albedo(np.asarray(LOOKUP_KD, dtype=np.float32), model.v[ti], model.n[ti], P + D * t, spec.uvs[0][ti], stored, filt)
        out.append((ti, tie, kd, near))
    return out


@pytest.mark.parametrize("opts,mode", [({}, 0), ({"lds_scene": 0}, 1), ({"wide_nodes": 2}, 3)])
@pytest.mark.parametrize("filt", [0, 1])
def test_albedo_matches_float64_formula(api, opts, mode, filt):
    """1,000 rays at the quad of lookup_spec under a random 5 x 3 texture.  Model-only figures, measured on the CPU before the first GPU
    run: 624 rays meet the quad, none with an intersection tie; under nearest filtering 0 of them (0 %; cap 5 %) are near a texel or
    wrap boundary (such rays would be left out), the others must equal kd * the stored texel bit for bit.  Bilinear: |kd' - model| <= 1e-4 (texels and
    kd are at most 1; px carries a few float32 ulps times w, under 1e-5, so the bound leaves a tenfold margin); measured maximum
    7.62e-7 (profiles/texture/README.md)."""
    spec = lookup_spec()
    sc = api.Scene(32, 32)
    for k, v in opts.items():
        if k != "lds_scene":
            sc.set_option(k, v)
    sc.load(spec)
    if "lds_scene" in opts:
        sc.set_option("lds_scene", opts["lds_scene"])
    assert sc.stat("node_mode") == mode
    texels = lookup_texels()
    t = sc.add_texture(texels, filter=filt)
    for m in range(3):
        sc.set_material_texture(m, t)
    stored, f = sc.debug_texture(t)
    assert f == filt and same_bits(stored, texels.astype(np.float16).astype(np.float32))
    rays = lookup_rays(api)
    t_ref, tri_ref = sc.debug_closest_hit(rays)
    tri, out = sc.debug_albedo(rays)                             # (the option is off: debug_albedo does not ask)
    assert np.array_equal(tri, tri_ref) and same_bits(out[:, 3], t_ref)
    hits = lookup_model_hits(api, spec, rays, texels, filt)
    kd_of = {2: spec.materials[0][0], 3: spec.materials[1][0], 4: spec.materials[2][0]}
    checked, near_n, worst, seen = 0, 0, 0.0, {2: 0, 3: 0, 4: 0}
    for i, (ti, tie, want, near) in enumerate(hits):
        if tie:
            continue
        assert int(tri[i]) == ti, i
        if ti < 0:
            assert same_bits(out[i], np.array([0.0, 0.0, 0.0, -1.0], dtype=np.float32)), i
        elif ti >= 2:                                            # no uvs / type 3 / type 1: the material's kd, the same bits
            assert same_bits(out[i, :3], np.asarray(kd_of[ti], dtype=np.float32)), (i, ti)
            seen[ti] += 1
        elif near and filt == 0:
            near_n += 1
        else:
            checked += 1
            if filt == 0:
                assert same_bits(out[i, :3], want.astype(np.float32)), (i, out[i], want)
            else:
                worst = max(worst, float(np.abs(out[i, :3].astype(np.float64) - want).max()))
    print("filter %d: %d quad hits checked, %d near-tie rays left out, largest |kd' - float64 formula| = %.3g; fall-back hits %s" % (filt, checked, near_n, worst, seen))
    assert checked > 300 and min(seen.values()) > 10
    assert near_n <= 0.05 * (checked + near_n)
    assert worst <= 1e-4
    # the texture matters, and so do the uvs: several distinct colours on the quad
    quad = np.array([h[0] in (0, 1) and not h[1] for h in hits])
    assert len(np.unique(out[quad, :3].round(4), axis=0)) > (10 if filt == 0 else 100)


def test_obj_map_kd_reaches_the_lookup(api, tmp_path):
    """pt_add_obj binds the map_Kd texture to the material it creates and records the vt: debug_albedo shows the picture's texels."""
    from opencl_path_tracer_amd import scenes
    d = str(tmp_path)
    px = bytes([255, 0, 0, 0, 255, 0, 0, 0, 255, 255, 255, 255])      # top row red, green; bottom row blue, white
    with open(os.path.join(d, "t.ppm"), "wb") as f:
        f.write(b"P6\n2 2\n255\n" + px)
    with open(os.path.join(d, "m.mtl"), "w") as f:
        f.write(scenes._mtl_block("a", ((0.5, 0.5, 0.5), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0)) + "map_Kd t.ppm\n")
    with open(os.path.join(d, "q.obj"), "w") as f:                     # (add_Obj negates x: the quad spans x in [-2, 2] either way)
        f.write("mtllib m.mtl\nv -2 -2 6\nv 2 -2 6\nv 2 2 6\nv -2 2 6\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nusemtl a\nf 1/1 2/2 3/3 4/4\n")
    sc = api.Scene(32, 32)
    sc.add_Obj(os.path.join(d, "q.obj"), (0, 0, 0), (1, 1, 1), 0.0, 0.0)
    sc.upload_Triangles()
    sc.upload_Materials()
    assert sc.stat("obj_textures_loaded") == 1
    sc.clear_textures()                                                 # nearest instead of the loader's bilinear: the texels themselves
    t = sc.add_texture(api.read_ppm(os.path.join(d, "t.ppm")), filter=0, srgb=1)
    sc.set_material_texture(0, t)
    rays = np.zeros(4, dtype=api.RAY)
    rays["D"][:, 2] = 1.0
    rays["P"][:, :2] = [(1.0, 0.5), (-1.0, 0.5), (1.0, -0.5), (-1.0, -0.7)]      # x is negated: u grows towards -x (all off the diagonal)
    tri, out = sc.debug_albedo(rays)
    assert (tri >= 0).all()
    want = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)], dtype=np.float32) * np.float32(0.5)
    assert same_bits(out[:, :3], want)


# ---------------------------------------------------------------------------- 3: the float64 model
REPLAY = dict(W=48, H=32, spp=2, bounces=4)
SPHERES = [((-2.6, -1.6, 7.0), 1.4, 7), ((0.3, -1.5, 9.6), 1.5, 5), ((2.7, -1.7, 6.2), 1.3, 6)]      # (centre, radius, material)


def replay_spec(textured=True):
    """tests/test_gpu_smooth.py's replay_spec (rebuilt here; the diffuse sphere has a material of its own, 7) with a bilinear checker on
    the floor (material 0, whose other surfaces have no uvs) and a nearest random 4 x 4 texture on the diffuse sphere"""
    from opencl_path_tracer_amd import scenes
    mats = [
        ((0.6, 0.6, 0.6), (0.2, 0.2, 0.2), (0, 0, 0), (0, 0, 0), (0, 0, 0), 20.0, 0),      # 0 white, glossy lobe
        ((0.6, 0.1, 0.1), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),             # 1 red
        ((0.1, 0.6, 0.1), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),             # 2 green
        ((0, 0, 0), (0, 0, 0), (6.0, 5.0, 4.0), (0, 0, 0), (0, 0, 0), 0.0, 3),             # 3 lamp
        ((0, 0, 0), (0, 0, 0), (12.0, 4.0, 2.0), (0, 0, 0), (0, 0, 0), 0.0, 3),            # 4 small hot emitter
        scenes.BUILTIN_MATERIALS[scenes.CHROMIUM],                                           # 5 mirror
        scenes.BUILTIN_MATERIALS[scenes.GLASS],                                              # 6 glass
        ((0.9, 0.8, 0.7), (0.2, 0.2, 0.2), (0, 0, 0), (0, 0, 0), (0, 0, 0), 20.0, 0),      # 7 the diffuse sphere
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
    spec = scenes.SceneSpec(materials=mats, name="texture_replay", shift=EYE_AT_ORIGIN)
    walls = np.asarray(tris, dtype=np.float32)
    spec.objects.append((walls, np.asarray(mo, dtype=np.uint16)))
    spec.normals = [None]
    uv = np.full((len(walls), 3, 2), np.nan, dtype=np.float32)
    uv[:2] = walls[:2][:, :, [0, 2]] / np.float32(3.0) + np.float32(0.21)          # the floor: (x, z) / 3, about four repeats each way
    spec.uvs = [uv]
    for c, r, m in SPHERES:
        v = scenes.uv_sphere(c, r, 8, 4)
        spec.objects.append((v, np.full(len(v), m, dtype=np.uint16)))
        spec.normals.append(scenes.uv_sphere_normals(c, r, 8, 4))
        spec.uvs.append(scenes.uv_sphere_uvs(rings=4, segments=8))
    if textured:
        spec.textures = [(scenes.checker_texture(4, (1.0, 0.9, 0.8), (0.15, 0.2, 0.3)), dict(filter=1)),
                         (np.random.default_rng(41).uniform(0.05, 1.0, (4, 4, 3)).astype(np.float32), dict(filter=0))]
        spec.material_textures = {0: 0, 7: 1}
    else:
        spec.uvs = []
    return spec


def replay_model(api, sc, spec, env=None, cam=None):
    verts = np.concatenate([v for v, _ in spec.objects])
    mo = np.concatenate([m for _, m in spec.objects])
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    vn = np.concatenate([np.zeros(v.shape, dtype=np.float32) if n is None else n for (v, _), n in zip(spec.objects, spec.normals)])
    uv = np.concatenate(spec.uvs)
    textures = [sc.debug_texture(k) for k in range(len(spec.textures))]
    return T.TextureModel(verts, recs["N"], mats, mo, sc.camera[0] if cam is None else cam, vn, uv, textures, spec.material_textures, env=env,
                          table=sc.debug_light_table())


@pytest.mark.parametrize("sky", [False, True])
def test_mis_matches_float64_model(api, sky):
    """The textured replay scene with smooth normals on.  Near-tie share of the model alone on these seeds, measured on the CPU before
    the first GPU run: 1.11 % without, 1.17 % with the sky (cap 10 %); textured type-0 vertices over the frame: 3,386 / 2,891."""
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
    sc.set_option("textures", 1)
    seeds = sc.read_rnds().copy()
    sc.iterations = bounces
    sc.render_nee(spp, "mis")
    model = replay_model(api, sc, spec, env)
    want, want_seeds, ties = model.render(seeds, bounces, spp, 2)
    got = sc.read_colors()[:, :3].astype(np.float64)
    keep = ~ties
    print("near-tie pixels: %d of %d; textured vertices: %d" % (int(ties.sum()), ties.size, model.textured_vertices))
    assert keep.mean() > 0.9, "too many near-tie pixels: %d" % int(ties.sum())
    assert model.textured_vertices > 500
    assert np.array_equal(sc.read_rnds()[keep], want_seeds[keep])
    scale = float(want[keep].max())
    err = np.abs(got[keep] - want[keep])
    bad = err > 2e-3 * np.abs(want[keep]) + 1e-6 * scale
    assert not bad.any(), "%d of %d pixel channels differ; worst %g" % (int(bad.sum()), bad.size, float((err / (np.abs(want[keep]) + 1e-6 * scale)).max()))
    assert float(want[keep].mean()) > 0.0
    # and the textures matter: the untextured frame differs
    flat = api.Scene(W, H).load(spec)
    if sky:
        flat.set_environment(scenes.sun_and_sky())
    flat.set_option("smooth_normals", 1)
    flat.iterations = bounces
    flat.render_nee(spp, "mis")
    assert not same_bits(flat.read_colors()[:, :3], sc.read_colors()[:, :3])


# ---------------------------------------------------------------------------- 4: the random streams do not see the textures
def test_rnds_and_rays_do_not_depend_on_the_textures(api):
    W = H = 32
    spec, twin = replay_spec(), replay_spec(textured=False)

    def scene(s, smooth, textures):
        sc = api.Scene(W, H).load(s)
        sc.set_option("smooth_normals", smooth)
        sc.set_option("textures", textures)
        sc.iterations = CB_BOUNCES
        return sc

    plain = scene(twin, 0, 0)
    plain.render(2, fused=False)                                # (generate_rays + trace_rays per sample: the launch that writes rays)
    want = state(plain)
    for strategy in ("bsdf", "light", "mis"):
        sc = scene(spec, 0, 1)
        sc.render_nee(2, strategy)
        got = state(sc)
        assert np.array_equal(got[1], want[1]) and same_bits(got[2], want[2]) and same_bits(got[3], want[3]), strategy
        assert not same_bits(got[0], want[0])
        smooth = scene(twin, 1, 0)
        smooth.render_nee(2, strategy)
        ws = state(smooth)
        sc = scene(spec, 1, 1)
        sc.render_nee(2, strategy)
        got = state(sc)
        assert np.array_equal(got[1], ws[1]) and same_bits(got[2], ws[2]) and same_bits(got[3], ws[3]), strategy
        assert not same_bits(got[0], ws[0])


# ---------------------------------------------------------------------------- 5: the preview
def test_preview_shows_kd_times_texel_plus_emission(api):
    """iterations == 1: every pixel whose four jitter corners read one texel of a nearest 3 x 3 texture shows kd * texel + emission."""
    from opencl_path_tracer_amd import scenes
    W = H = 32
    kd, em = np.array((0.8, 0.6, 0.4), dtype=np.float32), np.array((0.125, 0.25, 0.5), dtype=np.float32)
    mats = [(tuple(kd), (0, 0, 0), tuple(em), (0, 0, 0), (0, 0, 0), 1.0, 0)]
    a, b, c, d = (-4.0, -4.0, 6.0), (4.0, -4.0, 6.0), (4.0, 4.0, 6.0), (-4.0, 4.0, 6.0)
    spec = scenes.SceneSpec(materials=mats, shift=EYE_AT_ORIGIN, name="preview_quad")
    spec.objects.append((np.asarray([(a, b, c), (a, c, d)], dtype=np.float32), np.zeros(2, dtype=np.uint16)))
    spec.uvs = [np.asarray([[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)]], dtype=np.float32)]
    texels = np.random.default_rng(43).uniform(0.1, 1.0, (3, 3, 3)).astype(np.float32)
    spec.textures = [(texels, dict(filter=0))]
    spec.material_textures = {0: 0}
    sc = api.Scene(W, H).load(spec)
    sc.set_option("textures", 1)
    sc.iterations = 1
    sc.render_nee(1, "mis")
    got = sc.read_colors()[:, :3]
    stored = sc.debug_texture(0)[0]
    model = R.Model(spec.objects[0][0], api.triangles_from_vertices(*spec.objects[0])["N"], np.concatenate([api.Material(*mats[0])]), np.zeros(2, dtype=np.int64),
                    sc.camera[0])
    sure, cells = 0, set()
    for gid in range(W * H):
        cell = set()
        for r1, r2 in ((0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0)):
            P, D = model.camera_ray(gid, r1, r2)
            hp = P + D * ((6.0 - P[2]) / D[2])
            u, v = (hp[0] + 4.0) / 8.0, (hp[1] + 4.0) / 8.0
            ok = 0.0 < u < 1.0 and 0.0 < v < 1.0
            cell.add((min(2, int(u * 3)), min(2, int((1.0 - v) * 3))) if ok else None)
        if len(cell) != 1 or None in cell:
            continue
        x, y = next(iter(cell))
        assert same_bits(got[gid], kd * stored[y, x] + em), (gid, x, y)
        sure += 1
        cells.add((x, y))
    assert sure > W * H // 3 and len(cells) >= 5
    centre = [(H // 2 + dy) * W + W // 2 + dx for dy in (-1, 0) for dx in (-1, 0)]
    for gid in centre:
        assert same_bits(got[gid], kd * stored[1, 1] + em)
    off = api.Scene(W, H).load(spec)
    off.iterations = 1
    off.render_nee(1, "mis")
    assert same_bits(off.read_colors()[centre, :3], np.tile(kd + em, (4, 1)))


# ---------------------------------------------------------------------------- 6: gating
def test_other_paths_refuse_while_the_option_is_on(api, oracle, cb_spec, cb_oracle_scene):
    W, H = 48, 32
    calls = [lambda s: s.render(2), lambda s: s.trace_rays(), lambda s: s.generate_rays(), lambda s: s.render_adaptive(2, 4, 0.1),
             lambda s: s.render_adaptive(2, 4, 0.1, metric="half", path="render")]
    for k, call in enumerate(calls):
        sc = api.Scene(W, H).load(cb_spec)
        sc.iterations = CB_BOUNCES
        sc.set_option("textures", 1)
        with pytest.raises(api.PtError) as e:
            call(sc)
        assert e.value.code == api.PT_EINVAL and "textures" in str(e.value), k
        if k == 0:
            sc.set_option("variant", 1)
            with pytest.raises(api.PtError) as e:
                call(sc)
            assert e.value.code == api.PT_EINVAL and "textures" in str(e.value)
            sc.set_option("variant", 0)
        sc.set_option("textures", 0)
        call(sc)
        fresh = api.Scene(W, H).load(cb_spec)                  # a context that never had the option on
        fresh.iterations = CB_BOUNCES
        call(fresh)
        assert same_state(state(sc), state(fresh)), k
        if k == 0:
            cam = oracle.make_camera(cb_spec.fov, cb_spec.yaw, cb_spec.pitch, cb_spec.shift, W, H)
            fr = oracle.OracleFrame(W, H)
            fr.render(cb_oracle_scene, cam, CB_BOUNCES, 0, 2, nthreads=16)
            assert same_bits(sc.read_colors()[:, :3], fr.colors()[:, :3]) and np.array_equal(sc.read_rnds(), fr.rnds())


# ---------------------------------------------------------------------------- 7: adaptive NEE frames
@pytest.mark.parametrize("sky,opts,mode", [(False, {}, 0), (True, {"treelet": 40, "wide_nodes": 1, "mesh": 1}, 2)])
def test_adaptive_nee_tiles_hold_render_nee_bits(api, sky, opts, mode):
    """k_nee_tiles_tex on the textured replay scene, and k_nee_env_tiles_tex with a treelet (512-thread workgroups) on the 6,000-triangle
    mesh with computed vertex normals, random uvs and a texture on every material."""
    from opencl_path_tracer_amd import scenes
    W, H = 48, 32
    mesh = bool(opts.get("mesh"))
    spec = scenes.displaced_grid_mesh(6000) if mesh else replay_spec()

    def scene(textures=1):
        c = api.Scene(W, H)
        for k, v in opts.items():
            if k not in ("lds_scene", "mesh"):
                c.set_option(k, v)
        c.load(spec)
        assert c.stat("node_mode") == mode
        if mesh:
            c.compute_vertex_normals(60.0, obj=1)
            c.set_vertex_uvs(random_uvs(spec.ntris, seed=9))
            t = c.add_texture(np.random.default_rng(47).uniform(0.1, 1.0, (5, 7, 3)).astype(np.float32))
            for m in range(len(spec.materials)):
                c.set_material_texture(m, t)
        if sky:
            c.set_environment(scenes.sun_and_sky())
        c.set_option("smooth_normals", 1)
        c.set_option("textures", textures)
        return c
    sc = scene()
    sc.iterations = CB_BOUNCES
    # the threshold comes from the frame's own tile estimates, as in tests/test_gpu_smooth.py
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


# ---------------------------------------------------------------------------- 8: determinism
def test_determinism(api):
    W, H = 48, 32
    spec = replay_spec()
    a = api.Scene(W, H).load(spec)
    b = api.Scene(W, H).load(spec)
    for sc in (a, b):
        sc.set_option("smooth_normals", 1)
        sc.set_option("textures", 1)
        sc.iterations = CB_BOUNCES
    a.render_nee(4, "mis")
    a.render_nee(4, "mis")
    b.render_nee(8, "mis")
    assert same_state(state(a), state(b))
