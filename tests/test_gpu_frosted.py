"""-m gpu: the rough dielectric of option frosted in Scene.render_nee (material type 6; the frosted k_nee instances of pt_nee.hip,
k_debug_frosted of pt_glossy.hip; include/pt_api.h pins the vertex).

  1 the option without a type-6 material, and a type-6 material without the option, change no bit, with glossy, coated or a lens on;
  2 the device functions of the vertex (Scene.debug_frosted) against numpy's float64 evaluation, and the sampler against the evaluator;
  3 a frosted quad under a constant sky against float64 quadrature over both hemispheres in all three strategies;
  4 MIS frames with a frosted sphere behind a frosted pane against tests/frosted_ref.py (float64, brute force, same LCG and hashes);
  5 adaptive NEE tiles hold render_nee's bits; 6 determinism, and types 4, 5, 6 with a lens in one frame; 7 shaded guides."""

import numpy as np
import pytest

import frosted_ref as F
import glossy_ref as G
import nee_ref as R
import test_gpu_coated as TC
import test_gpu_glossy as TG

pytestmark = pytest.mark.gpu

F32 = np.float32
CB_BOUNCES = 4
STRATEGIES = ("bsdf", "light", "mis")
same_bits, state, same_state = TG.same_bits, TG.state, TG.same_state


def frosted(shininess, n=1.5):
    return ((0, 0, 0), (0, 0, 0), (0, 0, 0), (n, n, n), (0, 0, 0), float(shininess), 6)


# ---------------------------------------------------------------------------- 1: no material or no option, no change
def test_noops_are_bit_exact(api):
    from opencl_path_tracer_amd import scenes
    W = H = 32
    spp = 16

    def frame(spec, strategy, touch):
        sc = api.Scene(W, H).load(spec)
        touch(sc)
        sc.iterations = CB_BOUNCES
        sc.render_nee(spp, strategy)
        out = state(sc)
        sc.close()
        return out

    def on_and_off(sc):
        sc.set_option("frosted", 1)
        sc.set_option("frosted", 0)

    def lens(sc):
        sc.set_lens(20.0, 900.0)

    others = {"plain": (scenes.cornell_box(), lambda sc: None),
              "glossy": (scenes.cornell_box(glossy=True), lambda sc: sc.set_option("glossy", 1)),
              "coated": (scenes.cornell_box(coated=True), lambda sc: sc.set_option("coated", 1)),
              "lens": (scenes.cornell_box(), lens)}
    frosted_spec = scenes.cornell_box(frosted=True)
    for strategy in STRATEGIES:
        for name, (spec, other) in others.items():
            want = frame(spec, strategy, other)

            def both(sc):
                other(sc)
                sc.set_option("frosted", 1)
            assert same_state(frame(spec, strategy, both), want), (strategy, name)       # the option without a type-6 material
        plain = others["plain"][0]
        assert not same_state(frame(plain, strategy, lens), frame(plain, strategy, lambda sc: None))      # (the lens is a lens)
        # the material is inert until the option is on: the frame of a context that never touched the option
        inert = frame(frosted_spec, strategy, lambda sc: None)
        assert same_state(frame(frosted_spec, strategy, on_and_off), inert), strategy
        shaded = frame(frosted_spec, strategy, lambda sc: sc.set_option("frosted", 1))
        assert not same_bits(shaded[0], inert[0]), strategy


# ---------------------------------------------------------------------------- 2: the device functions
ETAS = (F32(1.5), F32(1.0) / F32(1.5))
U_SEL = (0.03, 0.35, 0.8, 0.97)


def frosted_inputs():
    """test_gpu_glossy.glossy_inputs()'s 4,096 items (alpha in {0.03, 0.1, 0.5, 1} x 16 values of o.z from head-on to 1e-3 x an 8 x 8 grid
    of (rnd1, rnd2) with the centre and the rim of the disc) as items of pt_debug_frosted: F0 = 0.04, eta alternating 1.5 and 1 / 1.5 every
    four items, and u_sel cycling through 0.03 (below Fm at every angle: F0 is 0.04), 0.35, 0.8 and 0.97, which fall on either side of Fm
    as o.h moves it from 0.04 head-on to 1 at grazing and inside the cone of total internal reflection"""
    g = TG.glossy_inputs()
    n = len(g)
    k = np.arange(n)
    items = np.zeros((n, 12), dtype=np.float32)
    items[:, 0:7] = g[:, 0:7]
    items[:, 7] = 0.04
    items[:, 8] = np.where((k // 4) % 2 == 0, ETAS[0], ETAS[1])
    items[:, 9:11] = g[:, 7:9]
    items[:, 11] = np.array(U_SEL)[k % 4]
    return items


def model_columns(items, dtype):
    v = F.vertex(items[:, 0:3], items[:, 3:6], items[:, 6], items[:, 7:8] * np.ones(3), items[:, 8], items[:, 9], items[:, 10], items[:, 11], dtype=dtype)
    return F.debug_columns(v), v


def frosted_errors(got, want, v):
    """frosted_ref.column_errors (relative errors), except that the two g columns are compared absolutely where |w.z| <= 1e-3: there g is
    proportional to G1 of w (mirrored for a refraction) and so to |w.z|, whose size and sign are rounding noise of the direction (as for
    G1(w) in test_gpu_glossy), and the absolute error is what factor_R sees"""
    e = F.column_errors(got, want)
    low = np.abs(v["w"][:, 2]) <= 1e-3
    got = np.asarray(got, dtype=np.float64)
    for k, c in ((3, 6), (5, 8)):
        e[low, k] = np.abs(got[low, c] - want[low, c])
    return e


def float32_restatement(items):
    """(float64 columns, float64 vertex, float32 columns, the items left out, the restatement's largest error of Fm and of disc inside the
    disc).  Left out: |u_sel - Fm| within the restatement's own largest error of Fm outside total internal reflection (the lobe is a coin
    toss), or |disc| within its largest error of disc (reflection or refraction, Fm = 1 or not, is one).  The errors are taken over the
    item's own region, inside the disc (rnd1 <= 0.999) or on its rim, the two regions the tolerances are taken over: on the rim of
    alpha = 0.03 the half vector, and Fm with it, is three orders of magnitude less certain than inside."""
    want, v = model_columns(items, np.float64)
    low, vl = model_columns(items, np.float32)
    assert (v["tir"] == vl["tir"]).all()
    inside = items[:, 9] <= np.float32(0.999)
    fe = np.abs(low[:, 3].astype(np.float64) - want[:, 3])
    de = np.abs(vl["disc"].astype(np.float64) - v["disc"])
    near = np.zeros(len(items), dtype=bool)
    for sel in (inside, ~inside):
        near |= sel & (((np.abs(items[:, 11].astype(np.float64) - want[:, 3]) <= fe[sel].max()) & ~v["tir"]) | (np.abs(v["disc"]) <= de[sel].max()))
    return want, v, low, near, float(fe[inside].max()), float(de[inside].max())


def test_device_functions_match_float64(api):
    """Tolerance: per column, 4 x the largest error of the float32 restatement against float64 (never below 4 x 2^-24), once over all kept
    inputs and once over those inside the disc (rnd1 <= 0.999), as in test_gpu_coated.  Items whose |u_sel - Fm| is within the
    restatement's own error of Fm (1.4e-5 inside the disc, 1.6e-2 on its rim), or whose |disc| is within its error of disc (5.1e-5, 1.5e-4),
    are left out: 2 of the 4,096 are, both on the rim; 63 % of the kept items reflect, 1,503 of them by total internal reflection.
    Measured on the CPU (float32 restatement against float64), relative errors in the order direction (as a vector), Fm, p_b sampled, g.x
    sampled, p_b again, g.x again, o.z:
      all inputs   6.7e-3  1.6e-2  1.6e-2  4.4e-4  9.8e-2  2.8e-4  3.1e-5
      inside       3.0e-5  4.7e-5  6.3e-5  4.4e-4  1.2e-3  2.8e-4  3.1e-5
    Measured on the device: see profiles/frosted/README.md.
    The large values belong to alpha = 0.03 (D(h) doubles every relative error of h.x, h.y) and to the rim of the disc, as for type 4."""
    items = frosted_inputs()
    assert items.shape == (4096, 12)
    want, v, low, near, fm_err, disc_err = float32_restatement(items)
    print("left out: %d of %d (restatement's error of Fm %.3g, of disc %.3g)" % (int(near.sum()), len(items), fm_err, disc_err))
    assert near.sum() < 0.01 * len(items)
    keep = ~near
    assert (low[keep, 4] == want[keep, 4]).all()                       # the restatement chooses the float64 lobes on the kept items
    assert 0.25 < want[keep, 4].mean() < 0.75                          # and both lobes make up 25-75 % of the items
    cpu = frosted_errors(low, want, v)
    inside = items[:, 9] <= np.float32(0.999)
    assert inside.sum() == 3584
    sc = api.Scene(8, 8)
    got = sc.debug_frosted(items).astype(np.float64)
    sc.close()
    assert np.isfinite(got).all()
    assert (got[keep, 4] == want[keep, 4]).all()                       # the lobe choice
    err = frosted_errors(got, want, v)
    bounds = {}
    for name, sel in (("all inputs", keep), ("inside", keep & inside)):
        bounds[name] = 4.0 * np.maximum(cpu[sel].max(axis=0), 2.0 ** -24)
        print("%-10s float32 model vs float64: %s" % (name, cpu[sel].max(axis=0)))
        print("%-10s device vs float64:        %s" % (name, err[sel].max(axis=0)))
    for name, sel in (("all inputs", keep), ("inside", keep & inside)):
        assert (err[sel].max(axis=0) <= bounds[name]).all(), (name, err[sel].max(axis=0), bounds[name])
    # beyond the critical angle of eta = 1 / 1.5 every item reflects, with Fm = 1
    cone = keep & v["tir"]
    assert cone.sum() > 500 and (items[cone, 8] == ETAS[1]).all()
    assert (got[cone, 4] == 1.0).all() and (got[cone, 3] == 1.0).all()
    refr = keep & (got[:, 4] == 0.0)
    assert (got[refr, 5] == 0.0).all() and (got[refr, 7] == 0.0).all() and (got[refr, 8] == 0.0).all()
    # the sampler and the evaluator agree for the reflected items wherever the path goes on (the device's own w.z > 0): MIS breaks
    # silently when they do not
    wz = (got[:, :3] * items[:, 0:3].astype(np.float64)).sum(axis=1) / np.linalg.norm(got[:, :3], axis=1)
    up = keep & (got[:, 4] == 1.0) & (wz > 0.0)
    assert up.sum() > 1000
    rel_pb = np.abs(got[:, 7] - got[:, 5]) / np.where(got[:, 5] != 0, got[:, 5], 1.0)
    dg = np.abs(got[:, 8] - got[:, 6])
    rel_g = np.where(wz <= 1e-3, dg, dg / np.where(got[:, 6] != 0, np.abs(got[:, 6]), 1.0))      # (the metric of frosted_errors)
    for name, sel in (("all inputs", up), ("inside", up & inside)):
        print("%-10s largest |p_b again / p_b sampled - 1| %.3g, |g.x again / g.x sampled - 1| %.3g over %d items"
              % (name, rel_pb[sel].max(), rel_g[sel].max(), sel.sum()))
        assert rel_pb[sel].max() <= max(bounds[name][2], bounds[name][4])
        assert rel_g[sel].max() <= max(bounds[name][3], bounds[name][5])


# ---------------------------------------------------------------------------- 3: quadrature
def frosted_quadrature(alpha, o, F0, eta, n_mu=96, n_phi=192):
    """per o (n, 3): I = I_r + I_t, the integral over the sphere of g(w) p(w) (the reflection lobe above, the refraction lobe below the
    surface), and V = the integral of g^2 p minus I^2, the variance of one sample g(w) of the BSDF strategy (a sample that leaves its
    hemisphere counts 0); Gauss-Legendre in cos(theta) x midpoint in phi, as test_gpu_coated.coated_quadrature, on each hemisphere"""
    x, wt = np.polynomial.legendre.leggauss(n_mu)
    mu, wt = 0.5 * (x + 1.0), 0.5 * wt
    phi = (np.arange(n_phi) + 0.5) * 2.0 * np.pi / n_phi
    s = np.sqrt(1.0 - mu * mu)
    up = np.stack([np.outer(s, np.cos(phi)), np.outer(s, np.sin(phi)), np.outer(mu, np.ones(n_phi))], -1).reshape(-1, 3)
    w = np.concatenate([up, up * np.array([1.0, 1.0, -1.0])])
    wq = np.tile(np.outer(wt, np.full(n_phi, 2.0 * np.pi / n_phi)).reshape(-1), 2)
    a, e = np.array([alpha]), np.array([eta])
    F0v = np.full(w.shape, F0)
    I, V = np.zeros(len(o)), np.zeros(len(o))
    for i in range(len(o)):
        p, g = F.evaluate_of(a, F0v, e, np.broadcast_to(o[i], w.shape), w)
        gx = np.where(p > 0, g[:, 0], 0.0)
        I[i] = float((gx * p * wq).sum())
        V[i] = float((gx ** 2 * p * wq).sum()) - I[i] ** 2
    return I, V


def frosted_frame(api, spec, strategy, W, H, spp, sky):
    sc = api.Scene(W, H).load(spec)
    if sky is not None:
        sc.set_environment(sky)
    sc.set_option("frosted", 1)
    sc.set_option("moments", 1)
    sc.iterations = 2
    sc.render_nee(spp, strategy)
    cols = sc.read_colors()[:, :3].astype(np.float64)
    var = sc.read_variance().astype(np.float64).reshape(-1)
    sc.close()
    return cols, var


def test_frosted_quad_under_a_constant_sky_matches_quadrature(api):
    """The tilted quad of test_gpu_glossy as type 6, shininess 6 (alpha 0.5), N = 1.5, under a sky of radiance 1, iterations = 2: a path
    with no diffuse vertex has bracket factor_L + factor_B = 2, and both the reflected and the refracted direction leave the lone quad
    for the sky, so frame / 2 estimates I_r(o) + I_t(o).  BSDF within 6 standard errors of the quadrature mean, the standard error from
    the MODEL's own variance (the integral of g^2 p minus I^2 per pixel, at the centre-of-pixel o), not from the frame; LIGHT and MIS
    within 6 combined standard errors (read_variance) of BSDF: a wrong weight after a refraction would bias LIGHT, whose reflected sky
    hits count 0 and whose refracted ones count 1."""
    W = H = 32
    spp = 64
    spec = TG.tilted_quad_spec(6.0)
    spec.materials = [frosted(6.0)]
    assert api.material_roughness(6.0) == 0.5
    sky = np.ones((1, 1, 3), dtype=np.float32)
    verts, mo = spec.objects[0]
    recs = api.triangles_from_vertices(verts, mo)
    cam = api.Camera(spec.fov, spec.yaw, spec.pitch, spec.shift, W, H)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    assert np.allclose(mats["F0"][0, :3], 0.04, rtol=1e-6) and float(mats["n"][0]) == 1.5
    model = R.Model(verts, recs["N"], mats, mo, cam[0])
    o = np.zeros((W * H, 3))
    for gid in range(W * H):
        P, D = model.camera_ray(gid, 0.5, 0.5)
        ti, _, _ = model.intersect(P, D)
        assert ti >= 0, gid
        N = model.n[ti] / np.linalg.norm(model.n[ti])
        N = -N if D @ N > 0 else N
        X, Z = G.frame(N[None])
        o[gid] = G.local(-D[None], X, Z, N[None])[0]
    I, V = frosted_quadrature(0.5, o, float(mats["F0"][0, 0]), 1.5)
    assert (V > 0).all() and I.max() < 1.0
    se_model = float(np.sqrt(V.sum() / spp)) / (W * H)
    frames = {s: frosted_frame(api, spec, s, W, H, spp, sky) for s in STRATEGIES}
    bracket = 2.0
    means = {s: float(frames[s][0][:, 0].mean()) / bracket for s in STRATEGIES}
    se = {s: float(np.sqrt(frames[s][1].sum()) / (W * H)) / bracket for s in STRATEGIES}
    print("quadrature mean %.6f, model standard error %.3g; frame means %s; standard errors %s" % (I.mean(), se_model, means, se))
    assert abs(means["bsdf"] - I.mean()) <= 6.0 * se_model
    for s in ("light", "mis"):
        assert abs(means[s] - means["bsdf"]) <= 6.0 * np.sqrt(se[s] ** 2 + se["bsdf"] ** 2), s


# ---------------------------------------------------------------------------- 4: the float64 model
REPLAY = dict(W=32, H=24, spp=4, bounces=4)
FROSTED = 10


def replay_spec():
    """test_gpu_coated.replay_spec (a rough-metal floor, a mirror, a type-5 plastic, a glass and a rough-gold type-4 sphere in a box) with
    its glass sphere a type-6 rough dielectric of shininess 30 (alpha 0.25, N = 1.5): material 10, and in front of the spheres one
    triangle of the same material, a pane with a single face: a path that refracts through it stays `inside`, so it meets the sphere with
    eta = 1 / 1.5, where total internal reflection occurs, and leaves every refraction along -Ng"""
    from opencl_path_tracer_amd import scenes
    spec = TC.replay_spec()
    spec.materials.append(tuple(scenes.BUILTIN_MATERIALS[scenes.GLASS][:5]) + (30.0, 6))
    assert len(spec.materials) - 1 == FROSTED
    v, m = spec.objects[3]
    assert (m == 6).all()
    spec.objects[3] = (v, np.full(len(v), FROSTED, dtype=np.uint16))
    pane = np.asarray([((-0.4, -2.9, 3.6), (4.6, -2.9, 4.4), (2.0, 1.2, 4.0))], dtype=np.float32)
    spec.objects.append((pane, np.full(1, FROSTED, dtype=np.uint16)))
    spec.normals.append(None)
    spec.name = "frosted_replay"
    return spec


def replay_scene(api, spec, sky, W, H, smooth=True, device=0):
    sc, env = TC.replay_scene(api, spec, sky, W, H, smooth, device)     # (options glossy and coated on)
    sc.set_option("frosted", 1)
    return sc, env


def replay_model(api, cam, spec, env=None, table=None, smooth=True, ps_margin=1e-5, fm_margin=1e-5):
    verts = np.concatenate([v for v, _ in spec.objects])
    mo = np.concatenate([m for _, m in spec.objects])
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    vn = np.concatenate([np.zeros(v.shape, dtype=np.float32) if n is None or not smooth else n for (v, _), n in zip(spec.objects, spec.normals)])
    return F.FrostedModel(verts, recs["N"], mats, mo, cam, vn, env=env, table=table, ps_margin=ps_margin, fm_margin=fm_margin)


REPLAY_EVENTS = ("frosted_reflect", "frosted_refract", "frosted_tir", "frosted_inside", "frosted_light", "coated_coat", "glossy_vertex")


@pytest.mark.parametrize("sky,smooth", [(False, True), (True, True), (False, False)])
def test_mis_matches_float64_model(api, sky, smooth):
    """Tolerance 2e-3 |want| + 1e-6 scale, the glossy and the coated replay's, by their method: the float32 restatement's largest relative
    error of g inside the disc at alpha 0.1 to 0.5 (this scene's frosted material has alpha 0.25) is 1.9e-4 per vertex and that of p_b
    8.1e-5 (test_device_functions_match_float64 prints the columns), and a path of 4 bounces multiplies at most 4 such factors and one MIS weight:
    4 x 1.9e-4 + 2 x 8.1e-5 = 9.2e-4 < 2e-3.  A pixel is a near tie by CoatedModel's margins, or when |u_sel - Fm| or |disc| at a type-6
    vertex is below the restatement's error of Fm or of disc.  rnds are equal bit for bit in the kept pixels.  The near-tie share and
    the events of the run on the device are in profiles/frosted/README.md."""
    W, H, spp, bounces = REPLAY["W"], REPLAY["H"], REPLAY["spp"], REPLAY["bounces"]
    spec = replay_spec()
    _, _, _, _, ps_err = TC.float32_restatement(TC.coated_inputs())
    _, _, _, _, fm_err, disc_err = float32_restatement(frosted_inputs())
    sc, env = replay_scene(api, spec, sky, W, H, smooth)
    seeds = sc.read_rnds().copy()
    sc.iterations = bounces
    sc.render_nee(spp, "mis")
    model = replay_model(api, sc.camera[0], spec, env, table=sc.debug_light_table(), smooth=smooth, ps_margin=ps_err, fm_margin=max(fm_err, disc_err))
    want, want_seeds, ties = model.render(seeds, bounces, spp, 2)
    got = sc.read_colors()[:, :3].astype(np.float64)
    keep = ~ties
    print("near ties: %.2f %%; events in the kept pixels: %s" % (100.0 * ties.mean(), {k: int(v[keep].sum()) for k, v in model.pixel_events.items()}))
    assert keep.mean() > 0.9, "too many near-tie pixels: %d" % int(ties.sum())
    for name in REPLAY_EVENTS + (("frosted_end_ng",) if smooth else ()):
        assert int(model.pixel_events[name][keep].sum()) > 0, name
    if sky:         # a sky miss right after a type-6 vertex, reflected (W_b from its p_b) or refracted (weight 1)
        assert int(model.pixel_events["frosted_sky"][keep].sum()) + int(model.pixel_events["frosted_through_sky"][keep].sum()) > 0
    assert np.array_equal(sc.read_rnds()[keep], want_seeds[keep])
    scale = float(want[keep].max())
    err = np.abs(got[keep] - want[keep])
    bad = err > 2e-3 * np.abs(want[keep]) + 1e-6 * scale
    print("worst error / bound: %.3g" % float((err / (2e-3 * np.abs(want[keep]) + 1e-6 * scale)).max()))
    assert not bad.any(), "%d of %d pixel channels differ; worst %g" % (int(bad.sum()), bad.size, float((err / (np.abs(want[keep]) + 1e-6 * scale)).max()))
    assert float(want[keep].mean()) > 0.0
    off, _ = replay_scene(api, spec, sky, W, H, smooth)
    off.set_option("frosted", 0)
    off.iterations = bounces
    off.render_nee(spp, "mis")
    assert not same_bits(off.read_colors()[:, :3], sc.read_colors()[:, :3])


# ---------------------------------------------------------------------------- 5: adaptive NEE frames
@pytest.mark.parametrize("sky,opts,mode", [(False, {}, 0), (True, {}, 0), (True, {"wide_nodes": 2}, 3)])
def test_adaptive_nee_tiles_hold_render_nee_bits(api, sky, opts, mode):
    """k_nee_tiles_frosted / k_nee_env_tiles_frosted against k_nee_frosted / k_nee_env_frosted on the replay scene, 16 x 16"""
    from opencl_path_tracer_amd import scenes
    W = H = 16
    spec = replay_spec()

    def scene(on=1):
        c = api.Scene(W, H)
        for k, v in opts.items():
            c.set_option(k, v)
        c.load(spec)
        assert c.stat("node_mode") == mode
        if sky:
            c.set_environment(scenes.sun_and_sky())
        c.set_option("smooth_normals", 1)
        c.set_option("glossy", 1)
        c.set_option("coated", 1)
        c.set_option("frosted", on)
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


# ---------------------------------------------------------------------------- 6: determinism
def test_determinism_and_every_lobe_material_with_a_lens(api):
    W, H = 32, 24
    spec = replay_spec()

    def scene():
        sc, _ = replay_scene(api, spec, True, W, H)
        sc.set_lens(0.2, 7.0)
        sc.iterations = CB_BOUNCES
        return sc
    a, b = scene(), scene()
    a.render_nee(4, "mis")
    a.render_nee(4, "mis")
    b.render_nee(8, "mis")
    assert same_state(state(a), state(b))
    cols = a.read_colors()[:, :3]
    assert np.isfinite(cols).all() and float(cols.mean()) > 0.0
    # (types 4, 5 and 6 are all in the frame, and the lens moved it)
    c, _ = replay_scene(api, spec, True, W, H)
    c.iterations = CB_BOUNCES
    c.render_nee(8, "mis")
    assert np.isfinite(c.read_colors()[:, :3]).all() and not same_bits(c.read_colors()[:, :3], cols)
    assert {4, 5, 6} <= {int(m[6]) for m in spec.materials}


# ---------------------------------------------------------------------------- 7: guides
def test_shaded_guides_show_the_frosted_glass(api, oracle):
    from opencl_path_tracer_amd import scenes
    W = H = 32
    spec = scenes.cornell_box(smooth=True, frosted=True)
    p = len(spec.materials) - 1
    sc = api.Scene(W, H).load(spec)
    sc.set_option("smooth_normals", 1)

    def guides(shading):
        sc.render_aovs(1, 4, shading=shading)
        alb, nd = sc.read_aovs()
        return alb.copy(), nd.copy()
    off_shaded, off_geo = guides("shaded"), guides("geometric")
    sc.set_option("frosted", 1)
    alb, nd = guides("shaded")
    geo = guides("geometric")
    assert same_bits(geo[0], off_geo[0]) and same_bits(geo[1], off_geo[1])            # geometric guides do not follow the option
    fr = alb[:, 3] == p
    assert fr.sum() > 30 and np.array_equal(fr, off_shaded[0][:, 3] == p)             # a terminal hit with or without the option
    # pixels that see the sphere directly (tint 1): albedo 1, as a terminal dielectric
    tri, ns = sc.debug_shading_normals(TG.pixel_rays(api, oracle, spec, W, H))
    first = 12 + spec.objects[1][0].shape[0]
    direct = fr & (tri >= first) & (tri < first + spec.objects[2][0].shape[0])
    assert direct.sum() > 30
    assert same_bits(alb[direct, :3], np.ones((int(direct.sum()), 3), dtype=F32))
    kd_em = (np.asarray(spec.materials[p][0], dtype=F32) + np.asarray(spec.materials[p][2], dtype=F32))
    assert same_bits(off_shaded[0][direct, :3], np.broadcast_to(kd_em, (int(direct.sum()), 3)))      # option off: kd + emission of the inert material
    assert same_bits(alb[~fr], off_shaded[0][~fr]) and same_bits(nd, off_shaded[1])
    s = (np.zeros(3, dtype=F32) + ns[direct, :3]).astype(F32)
    l2 = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
    assert same_bits(nd[direct, :3], s * (F32(1.0) / np.sqrt(l2))[:, None])            # Ns, through the pinned normalisation of pt_render_aovs
    sc.set_option("frosted", 0)
    again = guides("shaded")
    assert same_bits(again[0], off_shaded[0]) and same_bits(again[1], off_shaded[1])   # and off again: the buffers they were
    sc.close()
