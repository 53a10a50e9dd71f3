"""-m gpu: the rough metal of option glossy in Scene.render_nee (material type 4; pt_glossy.hip, the glossy k_nee instances of pt_nee.hip;
include/pt_api.h pins the vertex).

  * the option without a type-4 material, and a type-4 material without the option, change no bit;
  * the device functions of the vertex (Scene.debug_glossy) against numpy's float64 evaluation, and the sampler against the density;
  * a glossy quad under a constant sky against float64 quadrature in all three strategies; MIS beats both under a small bright light;
  * MIS frames, with and without an environment, against tests/glossy_ref.py (float64, brute force, same LCG and hashes);
  * the other render paths refuse while the option is on; adaptive NEE tiles hold render_nee's bits; determinism; shaded guides."""

import ctypes as C

import numpy as np
import pytest

import glossy_ref as G
import nee_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
CB_BOUNCES = 4
EYE_AT_ORIGIN = (-500.0, -500.0, 1299.0378)
STRATEGIES = ("bsdf", "light", "mis")


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def state(sc):
    rays = sc.read_rays()
    return sc.read_colors().copy(), sc.read_rnds().copy(), rays["P"][:, :3].copy(), rays["D"][:, :3].copy()


def same_state(a, b):
    return same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and same_bits(a[2], b[2]) and same_bits(a[3], b[3])


# ---------------------------------------------------------------------------- 1: no material or no option, no change
def test_option_without_the_material_and_material_without_the_option_are_noops(api, cb_spec):
    from opencl_path_tracer_amd import scenes
    W = H = 64
    spp = 4
    glossy_spec = scenes.cornell_box(glossy=True)

    def frame(spec, strategy, touch):
        sc = api.Scene(W, H).load(spec)
        touch(sc)
        sc.iterations = CB_BOUNCES
        sc.render_nee(spp, strategy)
        out = state(sc)
        sc.close()
        return out

    def on_and_off(sc):
        sc.set_option("glossy", 1)
        sc.set_option("glossy", 0)

    for strategy in STRATEGIES:
        want = frame(cb_spec, strategy, lambda sc: None)
        assert same_state(frame(cb_spec, strategy, lambda sc: sc.set_option("glossy", 1)), want), strategy
        # the material is inert until the option is on: the frame of a context that never touched the option
        inert = frame(glossy_spec, strategy, lambda sc: None)
        assert same_state(frame(glossy_spec, strategy, on_and_off), inert), strategy
        shaded = frame(glossy_spec, strategy, lambda sc: sc.set_option("glossy", 1))
        assert not same_bits(shaded[0], inert[0]), strategy


# ---------------------------------------------------------------------------- 2: the device functions
def glossy_inputs():
    """4,096 items: alpha in {0.03, 0.1, 0.5, 1} x 16 values of o.z from 1 down to 1e-3 x an 8 x 8 grid of (rnd1, rnd2) that holds 0 and
    1 - 2^-24.  o.z = 1 (D = -N) is given on axis-aligned normals only, where o comes out as (0, 0, 1) exactly and the tangent of the
    pinned sequence is its (1, 0, 0) branch in every precision; the other values of o.z turn over four normals, two of them tilted, one
    in each branch of the frame, at an azimuth that changes from item to item."""
    alphas = np.array([0.03, 0.1, 0.5, 1.0])
    oz = np.geomspace(1.0, 1e-3, 16)
    grid = np.array([0.0, 2.0 ** -24, 0.013, 0.25, 0.5, 0.77, 0.999, 1.0 - 2.0 ** -24])
    normals = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.48, -0.6, 0.64], [0.0006, 0.9999995, -0.0008]])
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    items = []
    k = 0
    for a in alphas:
        for iz, z in enumerate(oz):
            for r1 in grid:
                for r2 in grid:
                    N = normals[k % 2] if iz == 0 else normals[k % 4]
                    N32 = N.astype(np.float32).astype(np.float64)
                    X, Z = G.frame(N32[None])
                    phi = 2.399963 * k
                    s = np.sqrt(max(0.0, 1.0 - z * z))
                    D = -(X[0] * (s * np.cos(phi)) + Z[0] * (s * np.sin(phi)) + N32 * z)
                    items.append(np.concatenate([N, D / np.linalg.norm(D), [a, r1, r2]]))
                    k += 1
    return np.asarray(items, dtype=np.float32)


def float32_model_errors(items):
    """(float64 columns, float64 vertex, per-item errors (n, 6) of the pinned sequence restated in numpy float32 -- no fma, numpy's
    sin / cos rounded to float -- against the same sequence in float64), on the float32 inputs the device gets"""
    args = (items[:, 0:3], items[:, 3:6], items[:, 6], items[:, 7], items[:, 8], np.full(3, 0.04))
    v = G.vertex(*args, dtype=np.float64)
    want = G.debug_columns(v)
    low = G.debug_columns(G.vertex(*args, dtype=np.float32))
    return want, v, glossy_errors(low, want, v)


def glossy_errors(got, want, v):
    """glossy_ref.column_errors (relative errors), except that G1(w) is compared absolutely where w.z <= 1e-3: there G1 is proportional
    to w.z, whose size and sign are rounding noise of the reflection (5e8 relative between float32 and float64 on these inputs), and
    its absolute error is what factor_S sees"""
    e = G.column_errors(got, want)
    low = v["w"][:, 2] <= 1e-3
    e[low, 2] = np.abs(np.asarray(got, dtype=np.float64)[low, 4] - want[low, 4])
    return e


def test_device_functions_match_float64(api):
    """Tolerance: per column, 4 x the largest error of the float32 restatement against float64 (never below 4 x 2^-24, one rounding),
    once over all 4,096 inputs and once over the 3,584 inside the disc (rnd1 <= 0.999), where the sequence is well conditioned.
    Measured on the CPU, relative errors in the order direction (as a vector), p_b as sampled, G1(w), F.x, p_b evaluated again, o.z:
      all inputs   6.7e-3  6.6e-3  6.7e-4  1.6e-2  9.3e-2  3.1e-5
      inside       1.1e-4  6.3e-5  6.7e-4  4.7e-5  1.3e-3  3.1e-5
    The large values of the first row belong to the rim of the disc (rnd1 = 1 - 2^-24), where sqrtf(1 - t1^2 - t2^2) turns 1e-7 of
    rounding into 3e-4 of Nh, at alpha = 0.03, where D(h) doubles every relative error of h.x, h.y.  The sampled and the re-evaluated
    p_b of the float32 restatement differ by at most 1.7e-4 inside the disc."""
    items = glossy_inputs()
    assert items.shape == (4096, 9)
    want, v, cpu = float32_model_errors(items)
    inside = items[:, 7] <= np.float32(0.999)
    assert inside.sum() == 3584
    sc = api.Scene(8, 8)
    got = sc.debug_glossy(items).astype(np.float64)
    sc.close()
    assert np.isfinite(got).all()
    err = glossy_errors(got, want, v)
    bounds = {}
    for name, sel in (("all inputs", np.ones(len(items), dtype=bool)), ("inside", inside)):
        bounds[name] = 4.0 * np.maximum(cpu[sel].max(axis=0), 2.0 ** -24)
        print("%-10s float32 model vs float64: %s" % (name, cpu[sel].max(axis=0)))
        print("%-10s device vs float64:        %s" % (name, err[sel].max(axis=0)))
    for name, sel in (("all inputs", np.ones(len(items), dtype=bool)), ("inside", inside)):
        assert (err[sel].max(axis=0) <= bounds[name]).all(), (name, err[sel].max(axis=0), bounds[name])
    # the sampler and the density agree wherever the path goes on (the device's own w.z > 0): MIS breaks silently when they do not
    up = (got[:, :3] * items[:, 0:3].astype(np.float64)).sum(axis=1) > 0.0
    assert up.sum() > 3000
    rel = np.abs(got[:, 6] - got[:, 3]) / got[:, 3]
    print("largest |p_b again / p_b sampled - 1|: %.3g over %d items, %.3g over the %d inside the disc"
          % (rel[up].max(), up.sum(), rel[up & inside].max(), (up & inside).sum()))
    assert rel[up].max() <= max(bounds["all inputs"][1], bounds["all inputs"][4])
    assert rel[up & inside].max() <= max(bounds["inside"][1], bounds["inside"][4])


# ---------------------------------------------------------------------------- 3: quadrature
METAL = ((0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), (1, 1, 1))      # kd, ks, emission, N, K: F0 = (K^2 + 1) / (K^2 + 1) = 1


def quad(a, b, c, d):
    return [(a, b, c), (a, c, d)]


def tilted_quad_spec(shininess):
    """one type-4 quad that fills the 60-degree view from the origin, tilted so that o.z runs from head-on to 30 degrees off grazing"""
    from opencl_path_tracer_amd import scenes
    spec = scenes.SceneSpec(materials=[METAL + (shininess, 4)], shift=EYE_AT_ORIGIN, name="glossy_quad")
    tris = quad((-20.0, -3.0, 2.0), (20.0, -3.0, 2.0), (20.0, 8.0, 9.0), (-20.0, 8.0, 9.0))
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.zeros(2, dtype=np.uint16)))
    return spec


def quadrature(alpha, o, n_mu=96, n_phi=192):
    """integral over the upper hemisphere of g(w) p_b(w) for F0 = 1 and each o (n, 3): Gauss-Legendre in cos(theta), the midpoint rule
    in phi (exact for the trigonometric polynomials it can resolve; the integrand at alpha = 0.5 is smooth)"""
    x, wt = np.polynomial.legendre.leggauss(n_mu)
    mu, wt = 0.5 * (x + 1.0), 0.5 * wt
    phi = (np.arange(n_phi) + 0.5) * 2.0 * np.pi / n_phi
    s = np.sqrt(1.0 - mu * mu)
    w = np.stack([np.outer(s, np.cos(phi)), np.outer(s, np.sin(phi)), np.outer(mu, np.ones(n_phi))], -1).reshape(-1, 3)
    wq = np.outer(wt, np.full(n_phi, 2.0 * np.pi / n_phi)).reshape(-1)
    a = np.array([alpha])
    out = np.zeros(len(o))
    for i in range(len(o)):
        oo = np.broadcast_to(o[i], w.shape)
        pb, _ = G.ggx_pdf_of(a, oo, w)
        out[i] = float((G.ggx_G1(a, w) * pb * wq).sum())
    return out


def frame_mean_and_variance(api, spec, strategy, W, H, spp, sky):
    sc = api.Scene(W, H).load(spec)
    if sky is not None:
        sc.set_environment(sky)
    sc.set_option("glossy", 1)
    sc.set_option("moments", 1)
    sc.iterations = 2
    sc.render_nee(spp, strategy)
    cols = sc.read_colors()[:, :3].astype(np.float64)
    var = sc.read_variance().astype(np.float64).reshape(-1)
    sc.close()
    return cols, var


def test_glossy_quad_under_a_constant_sky_matches_quadrature(api):
    """Per pixel the lobe integral is I = the integral of g(w) p_b(w) over the hemisphere.  The estimator inherits the reference's bracket
    E (factor_L + factor_B) factor_S factor_R, and a path that met no diffuse vertex still has factor_L = factor_B = 1 (a mirror in front of
    a lamp shows twice the lamp's emission in every render path): under a sky of radiance 1 a sample is 2 g(w), so frame / 2 is the
    estimator of I with samples in [0, 1], and it is frame / 2 that is held to 6 x 0.5 / sqrt(pixels x spp)."""
    W = H = 32
    spp = 64
    spec = tilted_quad_spec(6.0)
    assert api.material_roughness(6.0) == 0.5
    sky = np.ones((1, 1, 3), dtype=np.float32)
    # the expected value per pixel, at the centre-of-pixel o
    verts, mo = spec.objects[0]
    recs = api.triangles_from_vertices(verts, mo)
    cam = api.Camera(spec.fov, spec.yaw, spec.pitch, spec.shift, W, H)
    model = R.Model(verts, recs["N"], np.concatenate([api.Material(*m) for m in spec.materials]), mo, cam[0])
    o = np.zeros((W * H, 3))
    for gid in range(W * H):
        P, D = model.camera_ray(gid, 0.5, 0.5)
        ti, _, _ = model.intersect(P, D)
        assert ti >= 0, gid                                   # the quad fills the view
        N = model.n[ti] / np.linalg.norm(model.n[ti])
        N = -N if D @ N > 0 else N
        X, Z = G.frame(N[None])
        o[gid] = G.local(-D[None], X, Z, N[None])[0]
    assert o[:, 2].min() > 0.3 and o[:, 2].max() > 0.95
    want = quadrature(0.5, o)
    assert 0.5 < want.min() and want.max() < 1.0
    frames = {s: frame_mean_and_variance(api, spec, s, W, H, spp, sky) for s in STRATEGIES}
    bracket = 2.0                                             # factor_L + factor_B of a path without a diffuse vertex
    means = {s: float(frames[s][0][:, 0].mean()) / bracket for s in STRATEGIES}
    # (grey everywhere: F0 = 1 and a white sky; the variance read-out is that of the luminance, which is the grey value: 0.2126 + 0.7152 + 0.0722 = 1)
    se = {s: float(np.sqrt(frames[s][1].sum()) / (W * H)) / bracket for s in STRATEGIES}
    print("quadrature mean %.6f; frame means %s; standard errors %s" % (want.mean(), means, se))
    assert abs(means["bsdf"] - want.mean()) <= 6.0 * 0.5 / np.sqrt(W * H * spp)
    for s in ("light", "mis"):
        assert abs(means[s] - means["bsdf"]) <= 6.0 * np.sqrt(se[s] ** 2 + se["bsdf"] ** 2), s


def highlight_spec():
    """a rough-metal floor (shininess 200: alpha 0.1) under one bright triangle light that hangs 0.6 above it: below the light the lobe is
    far narrower than the light (light sampling is the noisy one), further out the light is a speck in the lobe (BSDF sampling is)"""
    from opencl_path_tracer_amd import scenes
    mats = [METAL + (200.0, 4), ((0, 0, 0), (0, 0, 0), (60.0, 60.0, 60.0), (0, 0, 0), (0, 0, 0), 0.0, 3)]
    spec = scenes.SceneSpec(materials=mats, shift=EYE_AT_ORIGIN, name="glossy_highlight")
    tris = quad((-30.0, -1.5, 0.5), (30.0, -1.5, 0.5), (30.0, -1.5, 60.0), (-30.0, -1.5, 60.0))
    tris.append(((-0.9, -0.9, 5.0), (0.9, -0.9, 5.0), (0.0, -0.9, 6.6)))
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.asarray([0, 0, 1], dtype=np.uint16)))
    return spec


def test_mis_has_the_lowest_variance_under_a_small_bright_light(api):
    W = H = 32
    spec = highlight_spec()
    total = {s: float(frame_mean_and_variance(api, spec, s, W, H, 64, None)[1].sum()) for s in STRATEGIES}
    print("summed variance of the pixel means:", total)
    assert total["mis"] < total["bsdf"] and total["mis"] < total["light"], total


# ---------------------------------------------------------------------------- 4: the float64 model
REPLAY = dict(W=48, H=32, spp=2, bounces=4)
SPHERES = [((-2.6, -1.6, 7.0), 1.4, 0), ((0.3, -1.5, 9.6), 1.5, 5), ((2.7, -1.7, 6.2), 1.3, 6), ((1.6, 1.7, 8.2), 1.0, 8)]


def replay_spec():
    """tests/test_gpu_smooth.py's replay scene (rebuilt here) with the floor a rough metal of shininess 30 (material 7) and a fourth 8 x 4
    sphere of shininess 198 (alpha 0.1, material 8)"""
    from opencl_path_tracer_amd import scenes
    chromium = scenes.BUILTIN_MATERIALS[scenes.CHROMIUM]
    mats = [
        ((0.6, 0.6, 0.6), (0.2, 0.2, 0.2), (0, 0, 0), (0, 0, 0), (0, 0, 0), 20.0, 0),      # 0 white, glossy lobe
        ((0.6, 0.1, 0.1), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),             # 1 red
        ((0.1, 0.6, 0.1), (0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 0, 0), 1.0, 0),             # 2 green
        ((0, 0, 0), (0, 0, 0), (6.0, 5.0, 4.0), (0, 0, 0), (0, 0, 0), 0.0, 3),             # 3 lamp
        ((0, 0, 0), (0, 0, 0), (12.0, 4.0, 2.0), (0, 0, 0), (0, 0, 0), 0.0, 3),            # 4 small hot emitter
        chromium,                                                                            # 5 mirror
        scenes.BUILTIN_MATERIALS[scenes.GLASS],                                              # 6 glass
        tuple(chromium[:5]) + (30.0, 4),                                                     # 7 rough metal, alpha 0.25
        tuple(scenes.BUILTIN_MATERIALS[scenes.GOLD][:5]) + (198.0, 4),                     # 8 rough gold, alpha 0.1
    ]
    x0, x1, y0, y1, z0, z1 = -5.0, 5.0, -3.0, 5.0, -1.0, 12.0
    tris, mo = [], []
    for q, m in ((quad((x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)), 7),      # floor
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
    spec = scenes.SceneSpec(materials=mats, name="glossy_replay", shift=EYE_AT_ORIGIN)
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.asarray(mo, dtype=np.uint16)))
    spec.normals = [None]
    for c, r, m in SPHERES:
        v = scenes.uv_sphere(c, r, 8, 4)
        spec.objects.append((v, np.full(len(v), m, dtype=np.uint16)))
        spec.normals.append(scenes.uv_sphere_normals(c, r, 8, 4))
    return spec


def replay_model(api, sc, spec, env=None, table=None, smooth=True):
    verts = np.concatenate([v for v, _ in spec.objects])
    mo = np.concatenate([m for _, m in spec.objects])
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    vn = np.concatenate([np.zeros(v.shape, dtype=np.float32) if n is None or not smooth else n for (v, _), n in zip(spec.objects, spec.normals)])
    return G.GlossyModel(verts, recs["N"], mats, mo, sc.camera[0], vn, env=env, table=table)


def replay_scene(api, spec, sky, W, H, smooth=True, device=0):
    from opencl_path_tracer_amd import scenes
    sc = api.Scene(W, H, device=device).load(spec)
    env = None
    if sky:
        rgb = scenes.sun_and_sky()
        sc.set_environment(rgb)
        env = dict(rgb=rgb, tables=sc.debug_environment())
    sc.set_option("smooth_normals", 1 if smooth else 0)
    sc.set_option("glossy", 1)
    return sc, env


@pytest.mark.parametrize("sky,smooth", [(False, True), (True, True), (False, False)])
def test_mis_matches_float64_model(api, sky, smooth):
    """Near-tie share of the model alone on these seeds, measured on the CPU before the first GPU run: 0.9 % without, 1.0 % with the sky, 0.8 % without the sky
    and with smooth_normals off (cap 10 %); events
    in the kept pixels without / with the sky: glossy vertices 1,967 / 1,969, paths ended by w.z <= 0 103 / 102,
    by Ng 21 / 21, light samples taken at a glossy vertex 751 / 393, emitter hits after one with W_b < 1 24 / 24, sky misses after one
    - / 151.  With smooth_normals off (the glossy instances handed no vertex normals): 1,936 vertices, 103 ended by w.z <= 0, none by Ng
    (Ns = Ng there), 758 light samples, 24 emitter hits."""
    W, H, spp, bounces = REPLAY["W"], REPLAY["H"], REPLAY["spp"], REPLAY["bounces"]
    spec = replay_spec()
    sc, env = replay_scene(api, spec, sky, W, H, smooth)
    seeds = sc.read_rnds().copy()
    sc.iterations = bounces
    sc.render_nee(spp, "mis")
    model = replay_model(api, sc, spec, env, table=sc.debug_light_table(), smooth=smooth)
    want, want_seeds, ties = model.render(seeds, bounces, spp, 2)
    got = sc.read_colors()[:, :3].astype(np.float64)
    keep = ~ties
    print("near ties: %.2f %%; events in the kept pixels: %s" % (100.0 * ties.mean(), {k: int(v[keep].sum()) for k, v in model.pixel_events.items()}))
    assert keep.mean() > 0.9, "too many near-tie pixels: %d" % int(ties.sum())
    # (without vertex normals Ns = Ng: a direction with w.z > 0 is above the geometric surface)
    for name in ("glossy_vertex", "glossy_end_wz", "glossy_light", "glossy_emitter_wb") + (("glossy_end_ng",) if smooth else ()) + (("glossy_sky",) if sky else ()):
        assert int(model.pixel_events[name][keep].sum()) > 0, name
    assert np.array_equal(sc.read_rnds()[keep], want_seeds[keep])
    scale = float(want[keep].max())
    err = np.abs(got[keep] - want[keep])
    bad = err > 2e-3 * np.abs(want[keep]) + 1e-6 * scale
    assert not bad.any(), "%d of %d pixel channels differ; worst %g" % (int(bad.sum()), bad.size, float((err / (np.abs(want[keep]) + 1e-6 * scale)).max()))
    assert float(want[keep].mean()) > 0.0
    # and the material matters: with the option off the frame differs
    off, _ = replay_scene(api, spec, sky, W, H, smooth)
    off.set_option("glossy", 0)
    off.iterations = bounces
    off.render_nee(spp, "mis")
    assert not same_bits(off.read_colors()[:, :3], sc.read_colors()[:, :3])


def test_glossy_with_textures_keeps_the_random_streams(api):
    """The glossy instances with a real texture view (option textures on, smooth_normals off): the checker floor of
    scenes.cornell_box(textured=True) next to the rough sphere.  A texture changes no LCG draw and no pt_nee_rand value (the pinned rule of
    option textures), so rnds and rays are those of the same frame without textures, bit for bit, while the colours differ; pixels that
    show the floor directly carry the texel in the preview colour of iterations == 1, the metal its F0."""
    from opencl_path_tracer_amd import scenes
    W = H = 64
    spec = scenes.cornell_box(textured=True, glossy=True)
    g = len(spec.materials) - 1

    def frame(textures, iterations, spp):
        sc = api.Scene(W, H).load(spec)
        sc.set_option("glossy", 1)
        sc.set_option("textures", textures)
        sc.iterations = iterations
        sc.render_nee(spp, "mis")
        out = state(sc)
        sc.close()
        return out
    plain, tex, again = frame(0, CB_BOUNCES, 4), frame(1, CB_BOUNCES, 4), frame(1, CB_BOUNCES, 4)
    assert same_state(tex, again)
    assert np.array_equal(tex[1], plain[1]) and same_bits(tex[2], plain[2]) and same_bits(tex[3], plain[3])
    assert not same_bits(tex[0], plain[0])
    # the preview: kd' + emission on the floor, F0 + emission on the metal
    pre_plain, pre_tex = frame(0, 1, 1)[0][:, :3], frame(1, 1, 1)[0][:, :3]
    F0 = api.Material(*spec.materials[g])["F0"][0, :3]
    metal = (pre_tex.view(np.uint32) == F0.view(np.uint32)).all(axis=1)
    assert metal.sum() > 50 and same_bits(pre_plain[metal], pre_tex[metal])
    white = np.asarray(spec.materials[scenes.WHITE_DIFFUSE][0], dtype=np.float32)
    dark = (pre_tex.view(np.uint32) == (white * F32(0.25)).view(np.uint32)).all(axis=1)
    assert dark.sum() > 50 and (pre_plain[dark].view(np.uint32) == white.view(np.uint32)).all()


# ---------------------------------------------------------------------------- 5: gating
def test_other_paths_refuse_while_the_option_is_on(api, oracle, cb_spec, cb_oracle_scene):
    W, H = 48, 32
    sc = api.Scene(W, H).load(cb_spec)
    sc.iterations = CB_BOUNCES
    sc.set_option("glossy", 1)
    for call in (lambda: sc.render(1), lambda: sc.trace_rays(), lambda: sc.generate_rays(), lambda: sc.render_adaptive(2, 4, 0.1),
                 lambda: sc.render_adaptive(2, 4, 0.1, path="render")):
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_EINVAL and "glossy" in str(e.value)
    sc.set_option("variant", 1)
    with pytest.raises(api.PtError) as e:
        sc.render(1)
    assert e.value.code == api.PT_EINVAL and "glossy" in str(e.value)
    sc.set_option("variant", 0)
    sc.set_option("glossy", 0)
    sc.render(2)
    cam = oracle.make_camera(cb_spec.fov, cb_spec.yaw, cb_spec.pitch, cb_spec.shift, W, H)
    fr = oracle.OracleFrame(W, H)
    fr.render(cb_oracle_scene, cam, CB_BOUNCES, 0, 2, nthreads=16)
    assert same_bits(sc.read_colors()[:, :3], fr.colors()[:, :3]) and np.array_equal(sc.read_rnds(), fr.rnds())


# ---------------------------------------------------------------------------- 6: adaptive NEE frames
@pytest.mark.parametrize("sky,opts,mode", [(False, {}, 0), (True, {}, 0), (True, {"wide_nodes": 2}, 3)])
def test_adaptive_nee_tiles_hold_render_nee_bits(api, sky, opts, mode):
    """k_nee_tiles_glossy / k_nee_env_tiles_glossy against k_nee_glossy / k_nee_env_glossy on the replay scene"""
    from opencl_path_tracer_amd import scenes
    W, H = 48, 32
    spec = replay_spec()

    def scene(glossy=1):
        c = api.Scene(W, H)
        for k, v in opts.items():
            c.set_option(k, v)
        c.load(spec)
        assert c.stat("node_mode") == mode
        if sky:
            c.set_environment(scenes.sun_and_sky())
        c.set_option("smooth_normals", 1)
        c.set_option("glossy", glossy)
        return c
    sc = scene()
    sc.iterations = CB_BOUNCES
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
    inert = scene(0)
    inert.iterations = CB_BOUNCES
    inert.render_nee(16, "mis")
    sel = counts == 16
    assert not same_bits(cols[sel, :3], inert.read_colors()[sel, :3])


# ---------------------------------------------------------------------------- 7: determinism
def test_determinism(api):
    W, H = 48, 32
    spec = replay_spec()
    a, _ = replay_scene(api, spec, True, W, H)
    b, _ = replay_scene(api, spec, True, W, H)
    for sc in (a, b):
        sc.iterations = CB_BOUNCES
    a.render_nee(4, "mis")
    a.render_nee(4, "mis")
    b.render_nee(8, "mis")
    assert same_state(state(a), state(b))


# ---------------------------------------------------------------------------- 8: guides
def pixel_rays(api, oracle, spec, W, H):
    """the centre ray of every pixel, by the oracle's camera_get_ray (the device's, bit for bit)"""
    cam = oracle.make_camera(spec.fov, spec.yaw, spec.pitch, spec.shift, W, H)
    rays = np.zeros(W * H, dtype=api.RAY)
    one = np.zeros(1, dtype=oracle.RAY)
    L = oracle.lib()
    for gid in range(W * H):
        L.orc_camera_get_ray(one.ctypes.data_as(C.c_void_p), int(gid), cam.ctypes.data_as(C.c_void_p), 0.5, 0.5)
        rays["P"][gid], rays["D"][gid] = one["P"][0], one["D"][0]
    return rays


def test_shaded_guides_show_the_metal(api, oracle):
    from opencl_path_tracer_amd import scenes
    W = H = 48
    spec = scenes.cornell_box(smooth=True, glossy=True)
    g = len(spec.materials) - 1
    sc = api.Scene(W, H).load(spec)
    sc.set_option("smooth_normals", 1)

    def guides(shading):
        sc.render_aovs(1, 4, shading=shading)
        alb, nd = sc.read_aovs()
        return alb.copy(), nd.copy()
    off_shaded, off_geo = guides("shaded"), guides("geometric")
    sc.set_option("glossy", 1)
    alb, nd = guides("shaded")
    geo = guides("geometric")
    assert same_bits(geo[0], off_geo[0]) and same_bits(geo[1], off_geo[1])            # geometric guides do not follow the option
    metal = alb[:, 3] == g
    assert metal.sum() > 50 and np.array_equal(metal, off_shaded[0][:, 3] == g)
    F0 = api.Material(*spec.materials[g])["F0"][0, :3]
    assert same_bits(alb[metal, :3], np.broadcast_to(F0, (int(metal.sum()), 3)))       # tint (1, 1, 1) x F0
    assert not off_shaded[0][metal, :3].any()                                          # option off: kd + emission of the inert material, 0
    assert same_bits(alb[~metal], off_shaded[0][~metal]) and same_bits(nd, off_shaded[1])
    sc.set_option("glossy", 0)
    again = guides("shaded")
    assert same_bits(again[0], off_shaded[0]) and same_bits(again[1], off_shaded[1])   # and off again: the buffers they were
    sc.set_option("glossy", 1)
    # the normal of a pixel whose centre ray meets the metal first (not through the glass sphere) is that ray's shading normal, put through
    # the pinned normalisation of pt_render_aovs
    tri, ns = sc.debug_shading_normals(pixel_rays(api, oracle, spec, W, H))
    first = 12
    direct = metal & (tri >= first) & (tri < first + spec.objects[1][0].shape[0])
    assert direct.sum() > 50
    s = (np.zeros(3, dtype=F32) + ns[direct, :3]).astype(F32)
    l2 = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
    assert same_bits(nd[direct, :3], s * (F32(1.0) / np.sqrt(l2))[:, None])
    sc.close()
