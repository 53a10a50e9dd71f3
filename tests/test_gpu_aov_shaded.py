"""-m gpu: the shaded guide buffers (Scene.render_aovs(shading="shaded"), pt_render_aovs_ex with PT_AOV_SHADED; pinned in
include/pt_api.h) and their consumers.

  * with nothing to shade with they are pt_render_aovs's bits; the normal guide is the device's own shading normal, the albedo guide its
    own textured albedo (bit for bit, through pt_debug_shading_normal / pt_debug_albedo);
  * a specular chain under smooth normals against the float64 replay of tests/aov_shaded_ref.py;
  * the denoisers keep a texture they used to blur, temporal accumulation runs on the shaded guides, the authoring calls make shaded
    guides stale, a tiled rank renders its rows, two runs give the same bits."""
import ctypes as C

import numpy as np
import pytest

import aov_shaded_ref as A
import denoise_ref as DR
import temporal_ref as T
import texture_ref as TX

pytestmark = pytest.mark.gpu

EYE_AT_ORIGIN = (-500.0, -500.0, 1299.0378)
NODE_MODES = [(2, 1, 0), (0, 1, 1), (2, 2, 3)]          # the ones tests/test_gpu_texture.py parametrises over
F32 = np.float32


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def guides(sc, sub, depth, shading):
    sc.render_aovs(sub, depth, shading=shading)
    alb, nd = sc.read_aovs()
    return alb.copy(), nd.copy()


def pixel_rays(api, oracle, spec, W, H, r1, r2, ids=None):
    """the camera ray of every pixel at sub-pixel offset (r1, r2), by the oracle's camera_get_ray (the device's, bit for bit)"""
    cam = oracle.make_camera(spec.fov, spec.yaw, spec.pitch, spec.shift, W, H)
    ids = np.arange(W * H) if ids is None else ids
    rays = np.zeros(len(ids), dtype=api.RAY)
    one = np.zeros(1, dtype=oracle.RAY)
    L = oracle.lib()
    for k, gid in enumerate(ids):
        L.orc_camera_get_ray(one.ctypes.data_as(C.c_void_p), int(gid), cam.ctypes.data_as(C.c_void_p), float(r1), float(r2))
        rays["P"][k], rays["D"][k] = one["P"][0], one["D"][0]
    return rays


def normalised(sn):
    """the sum over one sub-pixel and the normalisation of pt_render_aovs in float32: s = 0 + n, then
    s * (1.0f / sqrtf((s.x s.x + s.y s.y) + s.z s.z)), 0 when s is 0"""
    sn = (np.zeros(3, dtype=F32) + np.asarray(sn, dtype=F32)).astype(F32)      # the running sum starts at +0: a component of -0 comes out +0
    l2 = (sn[:, 0] * sn[:, 0] + sn[:, 1] * sn[:, 1]) + sn[:, 2] * sn[:, 2]
    out = np.zeros_like(sn)
    nz = np.any(sn != 0, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F32(1.0) / np.sqrt(l2)
    out[nz] = sn[nz] * inv[nz, None]
    return out


# ---------------------------------------------------------------------------- scenes
SPHERE = ((0.2, -0.3, 6.0), 1.7)
CHECK_A, CHECK_B = (1.0, 0.9, 0.8), (0.15, 0.2, 0.3)


def sphere_spec():
    """a coarse diffuse uv_sphere (8 x 6) with its analytic normals and lat-long uvs over a floor, and a lamp (type 3) behind it"""
    from opencl_path_tracer_amd import scenes
    mats = [
        ((0.6, 0.6, 0.6), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),              # 0 floor
        ((0.9, 0.8, 0.7), (0.1, 0.1, 0.1), (0, 0, 0), (0, 0, 0), (0, 0, 0), 20.0, 0),       # 1 the sphere
        ((0.2, 0.1, 0.05), (0, 0, 0), (6.0, 5.0, 4.0), (0, 0, 0), (0, 0, 0), 0.0, 3),       # 2 lamp (a kd of its own: kd + emission)
    ]
    floor = [((-9.0, -2.0, 0.0), (9.0, -2.0, 0.0), (9.0, -2.0, 14.0)), ((-9.0, -2.0, 0.0), (9.0, -2.0, 14.0), (-9.0, -2.0, 14.0))]
    lamp = [((-3.0, 1.5, 11.0), (3.0, 1.5, 11.0), (3.0, 4.0, 11.0)), ((-3.0, 1.5, 11.0), (3.0, 4.0, 11.0), (-3.0, 4.0, 11.0))]
    spec = scenes.SceneSpec(materials=mats, shift=EYE_AT_ORIGIN, name="aov_sphere")
    walls = np.asarray(floor + lamp, dtype=np.float32)
    spec.objects.append((walls, np.asarray([0, 0, 2, 2], dtype=np.uint16)))
    c, r = SPHERE
    v = scenes.uv_sphere(c, r, 8, 6)
    spec.objects.append((v, np.full(len(v), 1, dtype=np.uint16)))
    spec.normals = [None, scenes.uv_sphere_normals(c, r, 8, 6)]
    spec.uvs = [np.full((len(walls), 3, 2), np.nan, dtype=np.float32), scenes.uv_sphere_uvs(rings=6, segments=8)]
    return spec


def textured_sphere(api, W, H, filt):
    from opencl_path_tracer_amd import scenes
    spec = sphere_spec()
    spec.textures = [(scenes.checker_texture(4, CHECK_A, CHECK_B), dict(filter=filt))]
    spec.material_textures = {1: 0, 2: 0}                  # (the binding on the lamp is ignored: type 3)
    sc = api.Scene(W, H).load(spec)
    sc.set_option("textures", 1)
    return sc, spec


# ---------------------------------------------------------------------------- 1: nothing to shade with
@pytest.mark.parametrize("lds,wide,mode", NODE_MODES)
def test_options_off_is_render_aovs(api, cb_spec, lds, wide, mode):
    W = H = 64
    sc = api.Scene(W, H)
    sc.set_option("wide_nodes", wide)
    sc.load(cb_spec)
    sc.set_option("lds_scene", lds)
    assert sc.stat("node_mode") == mode
    want = guides(sc, 2, 4, "geometric")
    assert (want[1][:, 3] > 0).any() and np.any((want[1][:, 3] > 0) & np.all(want[1][:, :3] == 0, axis=1))      # hits, and an escaping chain
    got = guides(sc, 2, 4, "shaded")
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    sc.set_option("smooth_normals", 1)                     # on, with nothing recorded or bound
    sc.set_option("textures", 1)
    got = guides(sc, 2, 4, "shaded")
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    p = api.AovParams(2, 4, api.PT_AOV_GEOMETRIC)          # GEOMETRIC through _ex
    sc._ck(api.LIB.pt_render_aovs_ex(sc._h, api._ptr(sc.camera), C.byref(p)))
    got = sc.read_aovs()
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    sc.close()


# ---------------------------------------------------------------------------- 2: the normal guide at primary hits
def test_normal_guide_is_the_shading_normal(api, oracle):
    """subpixels 1: the one sub-pixel ray is the pixel's centre ray, so the guide normal is pt_debug_shading_normal's Ns of that ray put
    through the pinned normalisation of pt_render_aovs (s * (1.0f / sqrtf(|s|^2)), restated in float32 here) and the depth is its t,
    bit for bit."""
    W = H = 48
    spec = sphere_spec()
    sc = api.Scene(W, H).load(spec)
    sc.set_option("smooth_normals", 1)
    alb, nd = guides(sc, 1, 4, "shaded")
    rays = pixel_rays(api, oracle, spec, W, H, F32(0.5), F32(0.5))
    tri, ns = sc.debug_shading_normals(rays)
    hit = tri >= 0
    assert hit.sum() > 0.5 * W * H and (~hit).any()
    assert same_bits(nd[:, 3], ns[:, 3])                                     # depth = t (-1 for a miss)
    assert same_bits(nd[:, :3], normalised(ns[:, :3]))
    assert np.all(nd[~hit, :3] == 0)
    geo = guides(sc, 1, 4, "geometric")
    assert same_bits(geo[1][:, 3], nd[:, 3]) and same_bits(geo[0], alb)      # same depth, same (untextured) albedo
    differ = np.any(geo[1][:, :3] != nd[:, :3], axis=1)
    on_sphere = alb[:, 3] == 1
    assert differ.sum() > 100 and not differ[~on_sphere].any()               # the facets are gone from the sphere, the rest is unchanged
    sc.close()


# ---------------------------------------------------------------------------- 3: the albedo guide
@pytest.mark.parametrize("filt", [0, 1])
def test_albedo_guide_is_the_textured_albedo(api, oracle, filt):
    W = H = 48
    sc, spec = textured_sphere(api, W, H, filt)
    emission = np.asarray([m[2] for m in spec.materials], dtype=F32)

    def terminal(r1, r2):
        """kd' + emission of each pixel's ray at that offset (0 for a miss) and its material (-1), float32"""
        tri, out = sc.debug_albedo(pixel_rays(api, oracle, spec, W, H, r1, r2))
        mo = np.concatenate([m for _, m in spec.objects])
        mat = np.where(tri >= 0, mo[np.maximum(tri, 0)].astype(np.int64), -1)
        a = (out[:, :3] + emission[np.maximum(mat, 0)]).astype(F32)
        a[tri < 0] = 0
        return a, mat

    a, mat = terminal(F32(0.5), F32(0.5))
    alb, _ = guides(sc, 1, 4, "shaded")
    assert same_bits(alb[:, :3], a) and np.array_equal(alb[:, 3], mat.astype(F32))
    assert (mat == 2).any() and (mat == 1).sum() > 200 and (mat == -1).any()
    flat, _ = guides(sc, 1, 4, "geometric")
    changed = np.any(flat[:, :3] != alb[:, :3], axis=1)
    assert changed[mat == 1].mean() > 0.9 and not changed[mat != 1].any()    # the texture shows on the sphere and nowhere else
    # subpixels 2: the float32 sum of the four sub-pixel values in raster order, / 4.0f
    total, first = np.zeros((W * H, 3), dtype=F32), None
    for k, (r1, r2) in enumerate(DR.subpixel_offsets(2)):
        a, mat = terminal(r1, r2)
        total = (total + a).astype(F32)
        first = mat if k == 0 else first
    alb2, _ = guides(sc, 2, 4, "shaded")
    assert same_bits(alb2[:, :3], total / F32(4.0)) and np.array_equal(alb2[:, 3], first.astype(F32))
    sc.close()


# ---------------------------------------------------------------------------- 4: a specular chain under smooth normals
CHAIN = dict(W=48, H=48, depth=4)


def chain_spec():
    """a smooth mirror sphere and a smooth glass sphere (coarse: 8 x 6, so that Ns and Ng disagree visibly) in front of a wall with a
    nearest-filtered checker, over a plain floor, under a lamp"""
    from opencl_path_tracer_amd import scenes
    mats = [
        ((0.8, 0.7, 0.6), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),              # 0 the textured wall
        ((0.5, 0.5, 0.5), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),              # 1 floor
        ((0.1, 0.1, 0.1), (0, 0, 0), (6.0, 5.0, 4.0), (0, 0, 0), (0, 0, 0), 0.0, 3),        # 2 lamp
        scenes.BUILTIN_MATERIALS[scenes.CHROMIUM],                                            # 3 mirror
        scenes.BUILTIN_MATERIALS[scenes.GLASS],                                               # 4 glass
    ]

    def quad(a, b, c, d):
        return [(a, b, c), (a, c, d)]
    wall = quad((-8.0, -2.0, 11.0), (8.0, -2.0, 11.0), (8.0, 7.0, 11.0), (-8.0, 7.0, 11.0))
    floor = quad((-8.0, -2.0, -1.0), (8.0, -2.0, -1.0), (8.0, -2.0, 11.0), (-8.0, -2.0, 11.0))
    lamp = quad((-2.0, 6.5, 4.0), (2.0, 6.5, 4.0), (2.0, 6.5, 8.0), (-2.0, 6.5, 8.0))
    walls = np.asarray(wall + floor + lamp, dtype=np.float32)
    spec = scenes.SceneSpec(materials=mats, shift=EYE_AT_ORIGIN, name="aov_chain")
    spec.objects.append((walls, np.asarray([0, 0, 1, 1, 2, 2], dtype=np.uint16)))
    uv = np.full((len(walls), 3, 2), np.nan, dtype=np.float32)
    uv[:2] = walls[:2][:, :, [0, 1]] / np.float32(4.0) + np.float32(0.13)
    spec.normals, spec.uvs = [None], [uv]
    for c, r, m in (((-1.75, -0.4, 6.6), 1.5, 3), ((1.7, -0.5, 6.0), 1.4, 4)):
        v = scenes.uv_sphere(c, r, 8, 6)
        spec.objects.append((v, np.full(len(v), m, dtype=np.uint16)))
        spec.normals.append(scenes.uv_sphere_normals(c, r, 8, 6))
        spec.uvs.append(np.full((len(v), 3, 2), np.nan, dtype=np.float32))
    spec.textures = [(scenes.checker_texture(4, CHECK_A, CHECK_B), dict(filter=0))]
    spec.material_textures = {0: 0}
    return spec


def chain_model(api, spec, textures, W, H):
    verts = np.concatenate([v for v, _ in spec.objects])
    mo = np.concatenate([m for _, m in spec.objects])
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    vn = np.concatenate([np.zeros(v.shape, dtype=np.float32) if n is None else n for (v, _), n in zip(spec.objects, spec.normals)])
    cam = api.Camera(spec.fov, spec.yaw, spec.pitch, spec.shift, W, H)[0]
    return TX.TextureModel(verts, recs["N"], mats, mo, cam, vn, np.concatenate(spec.uvs), textures, spec.material_textures)


def test_specular_chain_matches_float64_replay(api):
    """The float64 replay (tests/aov_shaded_ref.py) at subpixels 1, specular_depth 4.  Model-only figures, measured on the CPU before the
    first GPU run: 0 of the 2,304 pixels (0 %; cap 2 %) come within a margin of a decision (such pixels would be left out); 25 compared
    pixels took the Ng fall-back and 316 refracted; 150 chains escape and 10 end on the glass when the depth runs out.  Tolerance: |gpu - model| <= 2e-3 |model| + 1e-6 max|model| per buffer column group, the bound
    tests/test_gpu_smooth.py and tests/test_gpu_texture.py use for their float64 comparisons."""
    W, H, depth = CHAIN["W"], CHAIN["H"], CHAIN["depth"]
    spec = chain_spec()
    sc = api.Scene(W, H).load(spec)
    sc.set_option("smooth_normals", 1)
    sc.set_option("textures", 1)
    alb, nd = guides(sc, 1, depth, "shaded")
    model = chain_model(api, spec, [sc.debug_texture(0)], W, H)
    walb, wnd, near, fallback, refraction = A.replay(model, np.arange(W * H), [(0.5, 0.5)], depth)
    keep = ~near
    print("left out: %d of %d pixels; compared pixels with an Ng fall-back: %d, with a refraction: %d"
          % (int(near.sum()), near.size, int((fallback[keep] > 0).sum()), int((refraction[keep] > 0).sum())))
    assert near.mean() <= 0.02
    assert (fallback[keep] > 0).any() and (refraction[keep] > 0).any()
    assert np.array_equal(alb[keep, 3], walb[keep, 3].astype(F32))                      # the material index
    for what, got, want in (("albedo", alb[keep, :3], walb[keep, :3]), ("normal", nd[keep, :3], wnd[keep, :3]), ("depth", nd[keep, 3:], wnd[keep, 3:])):
        err = np.abs(got.astype(np.float64) - want)
        tol = 2e-3 * np.abs(want) + 1e-6 * float(np.abs(want).max())
        print("%s: worst |gpu - model| / tolerance = %.3g" % (what, float((err / tol).max())))
        assert np.all(err <= tol), "%s: %d values differ; worst %g of the tolerance" % (what, int((err > tol).sum()), float((err / tol).max()))
    # and both features matter here: the geometric guides differ
    galb, gnd = guides(sc, 1, depth, "geometric")
    assert not same_bits(galb, alb) and not same_bits(gnd, nd)
    sc.close()


# ---------------------------------------------------------------------------- 5: the denoiser keeps a texture
def wall_spec():
    from opencl_path_tracer_amd import scenes
    mats = [((0.8, 0.8, 0.8), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0)]
    a, b, c, d = (-6.3, -6.2, 6.0), (6.1, -6.2, 6.0), (6.1, 6.4, 6.0), (-6.3, 6.4, 6.0)      # (off centre: no pixel centre on the diagonal)
    v = np.asarray([(a, b, c), (a, c, d)], dtype=np.float32)
    spec = scenes.SceneSpec(materials=mats, shift=EYE_AT_ORIGIN, name="aov_wall")
    spec.objects.append((v, np.zeros(2, dtype=np.uint16)))
    spec.uvs = [v[:, :, [0, 1]] / np.float32(12.0) + np.float32(0.5)]
    spec.textures = [(scenes.checker_texture(8, CHECK_A, CHECK_B), dict(filter=0))]      # checks of 1.5 units, about 14 pixels
    spec.material_textures = {0: 0}
    return spec


def put_colors(api, sc, rgba):
    """overwrite the context's colors with a host frame (hipMemcpy through the library's own HIP runtime)"""
    sc.read_colors()                                        # (synchronises the context's stream)
    rgba = np.ascontiguousarray(rgba, dtype=np.float32)
    fn = api.LIB.hipMemcpy
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert fn(sc.device_colors(), rgba.ctypes.data, rgba.nbytes, 1) == 0
    assert same_bits(sc.read_colors(), rgba)


@pytest.mark.parametrize("which", ["denoise", "denoise_variance"])
def test_denoiser_keeps_the_texture(api, which):
    W = H = 64
    sc = api.Scene(W, H).load(wall_spec())
    sc.set_option("textures", 1)
    sc.set_option("moments", 1)
    sc.iterations = 2
    sc.render_nee(2, "bsdf")                                # a frame with valid moments for the variance filter; its colours are replaced
    alb, nd = guides(sc, 1, 4, "shaded")
    assert (nd[:, 3] > 0).all() and len(np.unique(alb[:, :3], axis=0)) == 2
    c = np.zeros((W * H, 4), dtype=F32)
    c[:, :3] = F32(0.7) * alb[:, :3]
    c[:, 3] = 4.0                                           # a second moment above the squared luminance: a finite positive variance
    put_colors(api, sc, c)
    inf = float("inf")
    if which == "denoise":
        run = lambda: sc.denoise(demodulate=1, sigma_color=inf, iterations=3)
    else:
        run = lambda: sc.denoise_variance(demodulate=1, sigma_luminance=inf, iterations=3)
    out = run()
    rel = np.abs(out[:, :3].astype(np.float64) - c[:, :3]) / c[:, :3]
    print("%s, shaded guides: worst relative change %.3g" % (which, float(rel.max())))
    assert rel.max() <= 1e-5
    sc.render_aovs(1, 4)                                    # geometric guides: the flat kd leaves the checker in the filtered signal
    out = run()
    contrast = 0.7 * 0.8 * (np.asarray(CHECK_A) - np.asarray(CHECK_B))
    worst = np.abs(out[:, :3].astype(np.float64) - c[:, :3]).max(axis=0)
    print("%s, geometric guides: worst change per channel %s of contrast %s" % (which, worst, contrast))
    assert np.all(worst > 0.1 * contrast)
    sc.close()


# ---------------------------------------------------------------------------- 6: temporal accumulation on shaded guides
def test_temporal_accumulate_uses_the_shaded_guides(api):
    """tests/test_gpu_temporal.py's moving-camera check (its tolerances, its exclusion rule: at least 99 % of the pixels compared) on
    the smooth sphere, NEE frames of 4 spp, shaded guides for both frames."""
    import opencl_path_tracer_amd.api as apimod
    W = H = 64
    spec = sphere_spec()
    sc = api.Scene(W, H).load(spec)
    sc.iterations = 4
    sc.set_option("moments", 1)
    sc.set_option("smooth_normals", 1)
    hist = None
    yaw, shift = spec.yaw, tuple(spec.shift)
    for i in range(2):
        if i:
            yaw += 0.5
            shift = apimod.camera_move(shift, yaw, spec.pitch, 0.0, 0.05, 0.0)
        sc.set_view(spec.fov, yaw, spec.pitch, shift)
        sc.current_sample = 0
        sc.render_nee(4, "mis")
        sc.render_aovs(1, 4, shading="shaded")
        sc.temporal_accumulate()
        alb, nd = sc.read_aovs()
        hist, info = T.accumulate(hist, sc.camera, sc.read_colors(), sc.sample_counts().reshape(-1), alb, nd, W, H, **api.temporal_defaults())
        rgbv, n = sc.read_temporal()
        ok = ~hist.bad
        assert ok.mean() >= 0.99, "frame %d: only %.4f of the pixels compared" % (i, ok.mean())
        err = np.abs(rgbv[ok, :3].astype(np.float64) - hist.c[ok]) - hist.tol_c[ok, None]
        assert np.all(err <= 0), "frame %d: colour, worst %r" % (i, err.max())
        assert np.all(np.abs(n[ok] - hist.n[ok]) <= 1e-5 * hist.n[ok])
        v, vm = rgbv[ok, 3].astype(np.float64), info["v"][ok]
        fin = np.isfinite(vm)
        assert np.array_equal(np.isfinite(v), fin)
        assert np.all(np.abs(v[fin] - vm[fin]) <= info["tol_v"][ok][fin])
    on_sphere = alb[:, 3] == 1
    print("pixels of the sphere that kept history: %.3f" % float(np.mean(n[on_sphere] > 4)))
    assert np.mean(n > 4) > 0.5
    sc.close()


# ---------------------------------------------------------------------------- 7: staleness
def test_authoring_calls_make_shaded_guides_stale(api, cb_spec):
    sc = api.Scene(32, 32).load(cb_spec)
    one_n, one_uv = np.ones((1, 3, 3), dtype=np.float32), np.zeros((1, 3, 2), dtype=np.float32)
    tex = np.ones((1, 1, 3), dtype=np.float32)
    sc.add_texture(tex)
    calls = [("set_vertex_normals", lambda: sc.set_vertex_normals(one_n)), ("clear_vertex_normals", sc.clear_vertex_normals),
             ("compute_vertex_normals", lambda: sc.compute_vertex_normals(30.0)), ("set_vertex_uvs", lambda: sc.set_vertex_uvs(one_uv)),
             ("clear_vertex_uvs", sc.clear_vertex_uvs), ("add_texture", lambda: sc.add_texture(tex)),
             ("set_material_texture", lambda: sc.set_material_texture(2, 0)), ("clear_textures", sc.clear_textures)]
    for name, call in calls:
        sc.render_aovs(1, 4, shading="shaded")
        sc.denoise()
        call()
        with pytest.raises(api.PtError) as e:
            sc.denoise()
        assert e.value.code == api.PT_EINVAL, name
        sc.render_aovs(1, 4, shading="shaded")              # rendering them again restores PT_OK
        sc.denoise()
    sc.add_texture(tex)
    for name, call in calls:                                # geometric guides do not read any of it
        sc.render_aovs(1, 4)
        call()
        sc.denoise()
    sc.render_aovs(1, 4, shading="shaded")                  # the two options do not invalidate guides
    sc.set_option("smooth_normals", 1)
    sc.set_option("textures", 1)
    sc.denoise()
    sc.upload_Materials()                                   # an upload still does
    with pytest.raises(api.PtError):
        sc.denoise()
    sc.close()


# ---------------------------------------------------------------------------- 8: a tiled rank
def test_tiled_rank_renders_its_rows(api):
    W = H = 48
    full, _ = textured_sphere(api, W, H, 1)
    full.set_option("smooth_normals", 1)
    want = guides(full, 2, 4, "shaded")
    full.close()
    spec = sphere_spec()
    from opencl_path_tracer_amd import scenes
    spec.textures = [(scenes.checker_texture(4, CHECK_A, CHECK_B), dict(filter=1))]
    spec.material_textures = {1: 0, 2: 0}
    sc = api.Scene(W, H, rank=1, world=2, rows_per_block=8).load(spec)
    sc.set_option("textures", 1)
    sc.set_option("smooth_normals", 1)
    ids = sc.local_pixel_ids()
    assert 0 < ids.size < W * H and ids.min() >= 8 * W
    got = guides(sc, 2, 4, "shaded")
    assert same_bits(got[0], want[0][ids]) and same_bits(got[1], want[1][ids])
    sc.close()


# ---------------------------------------------------------------------------- 9: determinism
def test_determinism(api):
    runs = []
    for _ in range(2):
        spec = chain_spec()
        sc = api.Scene(48, 48).load(spec)
        sc.set_option("smooth_normals", 1)
        sc.set_option("textures", 1)
        runs.append(guides(sc, 3, 4, "shaded"))
        runs.append(guides(sc, 3, 4, "shaded"))
        sc.close()
    for r in runs[1:]:
        assert same_bits(r[0], runs[0][0]) and same_bits(r[1], runs[0][1])
