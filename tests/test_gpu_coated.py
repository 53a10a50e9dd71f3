"""-m gpu: the coated diffuse of option coated in Scene.render_nee (material type 5; the coated k_nee instances of pt_nee.hip,
k_debug_coated of pt_glossy.hip; include/pt_api.h pins the vertex).

  1 the option without a type-5 material, and a type-5 material without the option, change no bit; only glossy on: the glossy kernels' bits;
  2 the device functions of the vertex (Scene.debug_coated) against numpy's float64 evaluation, and the sampler against the evaluator;
  3 a coated quad under a constant sky against float64 quadrature in all three strategies;
  4 MIS beats both other strategies under a small bright light;
  5 MIS frames with a type-5 and a type-4 sphere against tests/coated_ref.py (float64, brute force, same LCG and hashes);
  6 a texture on the plastic changes no random stream; 7 adaptive NEE tiles hold render_nee's bits; 8 determinism; 9 shaded guides."""

import numpy as np
import pytest

import coated_ref as K
import glossy_ref as G
import nee_ref as R
import test_gpu_glossy as TG

pytestmark = pytest.mark.gpu

F32 = np.float32
CB_BOUNCES = 4
STRATEGIES = ("bsdf", "light", "mis")
DIELECTRIC = ((1.5, 1.5, 1.5), (0, 0, 0))      # N, K: F0 = 0.04
same_bits, state, same_state = TG.same_bits, TG.state, TG.same_state


def plastic(kd, shininess):
    return (tuple(kd), (0, 0, 0), (0, 0, 0)) + DIELECTRIC + (float(shininess), 5)


# ---------------------------------------------------------------------------- 1: no material or no option, no change
def test_noops_are_bit_exact(api, cb_spec):
    from opencl_path_tracer_amd import scenes
    W = H = 32
    spp = 4
    coated_spec = scenes.cornell_box(coated=True)
    both_spec = scenes.cornell_box(glossy=True, coated=True)

    def frame(spec, strategy, touch):
        sc = api.Scene(W, H).load(spec)
        touch(sc)
        sc.iterations = CB_BOUNCES
        sc.render_nee(spp, strategy)
        out = state(sc)
        sc.close()
        return out

    def on_and_off(sc):
        sc.set_option("coated", 1)
        sc.set_option("coated", 0)

    for strategy in STRATEGIES:
        want = frame(cb_spec, strategy, lambda sc: None)
        assert same_state(frame(cb_spec, strategy, lambda sc: sc.set_option("coated", 1)), want), strategy
        inert = frame(coated_spec, strategy, lambda sc: None)
        assert same_state(frame(coated_spec, strategy, on_and_off), inert), strategy
        shaded = frame(coated_spec, strategy, lambda sc: sc.set_option("coated", 1))
        assert not same_bits(shaded[0], inert[0]), strategy
    # types 4 and 5 with only glossy on: the glossy kernels' frame, rendered by a context before option coated is ever set, and the same
    # bits again from that context after the option went on and off, and from a context that switched it on and off before rendering
    sc = api.Scene(W, H).load(both_spec)
    sc.set_option("glossy", 1)
    sc.iterations = CB_BOUNCES
    sc.render_nee(spp, "mis")
    before = state(sc)
    on_and_off(sc)
    sc.current_sample = 0
    sc.seed_default()
    sc.render_nee(spp, "mis")
    assert same_state(state(sc), before)
    sc.set_option("coated", 1)
    sc.current_sample = 0
    sc.seed_default()
    sc.render_nee(spp, "mis")
    assert not same_bits(state(sc)[0], before[0])
    sc.close()

    def glossy_then_toggle(c):
        on_and_off(c)
        c.set_option("glossy", 1)
    assert same_state(frame(both_spec, "mis", glossy_then_toggle), before)
    # and glossy stays a run-time matter inside the coated kernels: coated on, glossy off leaves type 4 inert (its frame differs from both)
    only_coated = frame(both_spec, "mis", lambda c: c.set_option("coated", 1))
    assert not same_bits(only_coated[0], before[0])


# ---------------------------------------------------------------------------- 2: the device functions
def coated_inputs():
    """test_gpu_glossy.glossy_inputs()'s 4,096 items (alpha in {0.03, 0.1, 0.5, 1} x 16 values of o.z from head-on to 1e-3 x an 8 x 8 grid
    of (rnd1, rnd2) with the centre and the rim of the disc) as items of pt_debug_coated: F0 = 0.04, kd alternating 0.8 / 0.2, and u_sel
    cycling through 0.05 (below the lower clamp of ps: always the coat), 0.95 (above the upper: always the base), 0.2 and 0.6, which fall
    on either side of ps as o.z moves it from 0.1 head-on to 0.9 at grazing"""
    g = TG.glossy_inputs()
    n = len(g)
    k = np.arange(n)
    items = np.zeros((n, 12), dtype=np.float32)
    items[:, 0:7] = g[:, 0:7]
    items[:, 7] = 0.04
    items[:, 8] = np.where((k // 4) % 2 == 0, 0.8, 0.2)
    items[:, 9:11] = g[:, 7:9]
    items[:, 11] = np.array([0.05, 0.95, 0.2, 0.6])[k % 4]
    return items


def model_columns(items, dtype):
    v = K.vertex(items[:, 0:3], items[:, 3:6], items[:, 6], items[:, 7:8] * np.ones(3), items[:, 8:9] * np.ones(3), items[:, 9], items[:, 10],
                 items[:, 11], dtype=dtype)
    return K.debug_columns(v), v


def coated_errors(got, want, v):
    """coated_ref.column_errors (relative errors), except that the two g columns are compared absolutely where w.z <= 1e-3: there spec is
    proportional to G1(w) and so to w.z, whose size and sign are rounding noise of the reflection (as for G1(w) in test_gpu_glossy), and the
    absolute error is what factor_S sees"""
    e = K.column_errors(got, want)
    low = v["w"][:, 2] <= 1e-3
    got = np.asarray(got, dtype=np.float64)
    for k, c in ((3, 6), (5, 8)):
        e[low, k] = np.abs(got[low, c] - want[low, c])
    return e


def float32_restatement(items):
    """(float64 columns, float64 vertex, errors (n, 7) of the float32 restatement against float64, the items whose lobe choice is a near tie:
    |u_sel - ps| within the restatement's own largest error of ps)"""
    want, v = model_columns(items, np.float64)
    low, _ = model_columns(items, np.float32)
    ps_err = float(np.abs(low[:, 3].astype(np.float64) - want[:, 3]).max())
    near = np.abs(items[:, 11].astype(np.float64) - want[:, 3]) <= ps_err
    return want, v, low, near, ps_err


def test_device_functions_match_float64(api):
    """Tolerance: per column, 4 x the largest error of the float32 restatement against float64 (never below 4 x 2^-24), once over all kept
    inputs and once over those inside the disc (rnd1 <= 0.999), as in test_gpu_glossy.  Items whose |u_sel - ps| is within the
    restatement's own error of ps are left out (their lobe is a coin toss); none of the 4,096 is.
    Measured on the CPU (float32 restatement against float64), relative errors in the order direction (as a vector), ps, p_b sampled, g.x
    sampled, p_b again, g.x again, o.z:
      all inputs   6.7e-3  3.1e-7  4.1e-3  9.5e-4  9.3e-2  9.5e-4  3.1e-5
      inside       3.0e-5  2.9e-7  5.6e-4  9.5e-4  1.3e-3  9.5e-4  3.1e-5
    The large values belong to alpha = 0.03 (D(h) doubles every relative error of h.x, h.y) and to the rim of the disc, as for type 4; at
    alpha >= 0.1 inside the disc every column is below 2e-4 but g at alpha = 1 and o.z = 1e-3 (6.6e-4).
    Measured on the device: see profiles/coated/README.md."""
    items = coated_inputs()
    assert items.shape == (4096, 12)
    want, v, low, near, ps_err = float32_restatement(items)
    print("near ties of the lobe choice: %d of %d (restatement's error of ps %.3g)" % (int(near.sum()), len(items), ps_err))
    assert near.sum() < 0.01 * len(items)
    keep = ~near
    assert (low[keep, 4] == want[keep, 4]).all()                       # the restatement chooses the float64 lobes on the kept items
    assert 0.25 < want[keep, 4].mean() < 0.75                          # and both lobes are well represented
    cpu = coated_errors(low, want, v)
    inside = items[:, 9] <= np.float32(0.999)
    assert inside.sum() == 3584
    sc = api.Scene(8, 8)
    got = sc.debug_coated(items).astype(np.float64)
    sc.close()
    assert np.isfinite(got).all()
    assert (got[keep, 4] == want[keep, 4]).all()                       # the lobe choice
    err = coated_errors(got, want, v)
    bounds = {}
    for name, sel in (("all inputs", keep), ("inside", keep & inside)):
        bounds[name] = 4.0 * np.maximum(cpu[sel].max(axis=0), 2.0 ** -24)
        print("%-10s float32 model vs float64: %s" % (name, cpu[sel].max(axis=0)))
        print("%-10s device vs float64:        %s" % (name, err[sel].max(axis=0)))
    for name, sel in (("all inputs", keep), ("inside", keep & inside)):
        assert (err[sel].max(axis=0) <= bounds[name]).all(), (name, err[sel].max(axis=0), bounds[name])
    # the sampler and the evaluator agree wherever the path goes on (the device's own w.z > 0): MIS breaks silently when they do not
    wz = (got[:, :3] * items[:, 0:3].astype(np.float64)).sum(axis=1) / np.linalg.norm(got[:, :3], axis=1)
    up = keep & (wz > 0.0)
    assert up.sum() > 3000
    rel_pb = np.abs(got[:, 7] - got[:, 5]) / got[:, 5]
    dg = np.abs(got[:, 8] - got[:, 6])
    rel_g = np.where(wz <= 1e-3, dg, dg / np.where(got[:, 6] != 0, np.abs(got[:, 6]), 1.0))      # (the metric of coated_errors)
    for name, sel in (("all inputs", up), ("inside", up & inside)):
        print("%-10s largest |p_b again / p_b sampled - 1| %.3g, |g.x again / g.x sampled - 1| %.3g over %d items"
              % (name, rel_pb[sel].max(), rel_g[sel].max(), sel.sum()))
        assert rel_pb[sel].max() <= max(bounds[name][2], bounds[name][4])
        assert rel_g[sel].max() <= max(bounds[name][3], bounds[name][5])


# ---------------------------------------------------------------------------- 3: quadrature
def coated_quadrature(alpha, o, F0, kd, n_mu=96, n_phi=192):
    """per o (n, 3): I = the integral over the upper hemisphere of spec + diff, and V = the integral of g^2 p_b minus I^2, the variance of
    one sample g(w) of the BSDF strategy (a sample that leaves the hemisphere counts 0); Gauss-Legendre in cos(theta) x midpoint in phi"""
    x, wt = np.polynomial.legendre.leggauss(n_mu)
    mu, wt = 0.5 * (x + 1.0), 0.5 * wt
    phi = (np.arange(n_phi) + 0.5) * 2.0 * np.pi / n_phi
    s = np.sqrt(1.0 - mu * mu)
    w = np.stack([np.outer(s, np.cos(phi)), np.outer(s, np.sin(phi)), np.outer(mu, np.ones(n_phi))], -1).reshape(-1, 3)
    wq = np.outer(wt, np.full(n_phi, 2.0 * np.pi / n_phi)).reshape(-1)
    a = np.array([alpha])
    F0v, kdv = np.full(w.shape, F0), np.full(w.shape, kd)
    I, V = np.zeros(len(o)), np.zeros(len(o))
    for i in range(len(o)):
        pb, g, spec, diff = K.evaluate_of(a, F0v, kdv, np.broadcast_to(o[i], w.shape), w)
        I[i] = float(((spec + diff)[:, 0] * wq).sum())
        V[i] = float((g[:, 0] ** 2 * pb * wq).sum()) - I[i] ** 2
    return I, V


def coated_frame(api, spec, strategy, W, H, spp, sky):
    sc = api.Scene(W, H).load(spec)
    if sky is not None:
        sc.set_environment(sky)
    sc.set_option("coated", 1)
    sc.set_option("moments", 1)
    sc.iterations = 2
    sc.render_nee(spp, strategy)
    cols = sc.read_colors()[:, :3].astype(np.float64)
    var = sc.read_variance().astype(np.float64).reshape(-1)
    sc.close()
    return cols, var


def test_coated_quad_under_a_constant_sky_matches_quadrature(api):
    """The tilted quad of test_gpu_glossy as type 5, grey kd 0.8, shininess 6 (alpha 0.5), under a sky of radiance 1, iterations = 2: a path
    with no diffuse vertex has bracket factor_L + factor_B = 2, so frame / 2 estimates I(o) = the integral of spec + diff.  BSDF within 6
    standard errors of the quadrature mean, the standard error from the MODEL's own variance (the integral of g^2 p_b minus I^2 per pixel,
    at the centre-of-pixel o), not from the frame; LIGHT and MIS within 6 combined standard errors (read_variance) of BSDF."""
    W = H = 32
    spp = 64
    spec = TG.tilted_quad_spec(6.0)
    spec.materials = [plastic((0.8, 0.8, 0.8), 6.0)]
    assert api.material_roughness(6.0) == 0.5
    sky = np.ones((1, 1, 3), dtype=np.float32)
    verts, mo = spec.objects[0]
    recs = api.triangles_from_vertices(verts, mo)
    cam = api.Camera(spec.fov, spec.yaw, spec.pitch, spec.shift, W, H)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    assert np.allclose(mats["F0"][0, :3], 0.04, rtol=1e-6)
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
    I, V = coated_quadrature(0.5, o, float(mats["F0"][0, 0]), float(F32(0.8)))
    assert (V > 0).all() and I.max() < 1.0
    se_model = float(np.sqrt(V.sum() / spp)) / (W * H)
    frames = {s: coated_frame(api, spec, s, W, H, spp, sky) for s in STRATEGIES}
    bracket = 2.0
    means = {s: float(frames[s][0][:, 0].mean()) / bracket for s in STRATEGIES}
    se = {s: float(np.sqrt(frames[s][1].sum()) / (W * H)) / bracket for s in STRATEGIES}
    print("quadrature mean %.6f, model standard error %.3g; frame means %s; standard errors %s" % (I.mean(), se_model, means, se))
    assert abs(means["bsdf"] - I.mean()) <= 6.0 * se_model
    for s in ("light", "mis"):
        assert abs(means[s] - means["bsdf"]) <= 6.0 * np.sqrt(se[s] ** 2 + se["bsdf"] ** 2), s


# ---------------------------------------------------------------------------- 4: MIS pays
def test_mis_has_the_lowest_variance_under_a_small_bright_light(api):
    """test_gpu_glossy.highlight_spec's floor as type 5, shininess 200 (alpha 0.1), white kd"""
    W = H = 32
    spec = TG.highlight_spec()
    spec.materials[0] = plastic((1.0, 1.0, 1.0), 200.0)
    total = {s: float(coated_frame(api, spec, s, W, H, 64, None)[1].sum()) for s in STRATEGIES}
    print("summed variance of the pixel means:", total)
    assert total["mis"] < total["bsdf"] and total["mis"] < total["light"], total


# ---------------------------------------------------------------------------- 5: the float64 model
REPLAY = dict(W=32, H=24, spp=4, bounces=4)
PLASTIC = 9


def replay_spec():
    """test_gpu_glossy.replay_spec (a rough-metal floor, a mirror, a glass and a rough-gold type-4 sphere) with its first sphere, the white
    one, a type-5 plastic of shininess 20 (alpha 0.30): material 9"""
    spec = TG.replay_spec()
    spec.materials.append(plastic((0.6, 0.15, 0.1), 20.0))
    assert len(spec.materials) - 1 == PLASTIC
    v, m = spec.objects[1]
    spec.objects[1] = (v, np.full(len(v), PLASTIC, dtype=np.uint16))
    spec.name = "coated_replay"
    return spec


def replay_scene(api, spec, sky, W, H, smooth=True, device=0):
    sc, env = TG.replay_scene(api, spec, sky, W, H, smooth, device)     # (option glossy on)
    sc.set_option("coated", 1)
    return sc, env


def replay_model(api, cam, spec, env=None, table=None, smooth=True, ps_margin=1e-5):
    verts = np.concatenate([v for v, _ in spec.objects])
    mo = np.concatenate([m for _, m in spec.objects])
    recs = api.triangles_from_vertices(verts, mo)
    mats = np.concatenate([api.Material(*m) for m in spec.materials])
    vn = np.concatenate([np.zeros(v.shape, dtype=np.float32) if n is None or not smooth else n for (v, _), n in zip(spec.objects, spec.normals)])
    return K.CoatedModel(verts, recs["N"], mats, mo, cam, vn, env=env, table=table, ps_margin=ps_margin)


REPLAY_EVENTS = ("coated_coat", "coated_base", "coated_end_wz", "coated_light", "coated_emitter_wb", "glossy_vertex")


@pytest.mark.parametrize("sky,smooth", [(False, True), (True, True), (False, False)])
def test_mis_matches_float64_model(api, sky, smooth):
    """Tolerance 2e-3 |want| + 1e-6 scale, the glossy replay's.  Confirmed on the CPU: the float32 restatement's largest relative error of
    g inside the disc at the roughnesses of this scene (alpha 0.1 to 0.5) is 1.9e-4 per vertex and that of p_b 1.9e-4
    (test_device_functions_match_float64 prints them), and a path of 4 bounces multiplies at most 4 such factors and one MIS weight:
    4 x 1.9e-4 + 2 x 1.9e-4 = 1.2e-3 < 2e-3, so the mixture needs no more.  A pixel is a near tie by GlossyModel's margins or when
    |u_sel - ps| is below the restatement's error of ps (2.4e-7).  Near-tie share of the model alone without the sky, measured on the CPU
    before the first GPU run: 2.6 % with smooth_normals, 2.0 % without (cap 10 %); events in the kept pixels there: coat lobe 130 / 125, base
    lobe 412 / 479, ended by w.z <= 0 3 / 5, by Ng 20 / -, light samples at a type-5 vertex 179 / 233, emitter hits after one with W_b < 1
    4 / 3.  On the device: profiles/coated/README.md."""
    W, H, spp, bounces = REPLAY["W"], REPLAY["H"], REPLAY["spp"], REPLAY["bounces"]
    spec = replay_spec()
    _, _, _, _, ps_err = float32_restatement(coated_inputs())
    sc, env = replay_scene(api, spec, sky, W, H, smooth)
    seeds = sc.read_rnds().copy()
    sc.iterations = bounces
    sc.render_nee(spp, "mis")
    model = replay_model(api, sc.camera[0], spec, env, table=sc.debug_light_table(), smooth=smooth, ps_margin=ps_err)
    want, want_seeds, ties = model.render(seeds, bounces, spp, 2)
    got = sc.read_colors()[:, :3].astype(np.float64)
    keep = ~ties
    print("near ties: %.2f %%; events in the kept pixels: %s" % (100.0 * ties.mean(), {k: int(v[keep].sum()) for k, v in model.pixel_events.items()}))
    assert keep.mean() > 0.9, "too many near-tie pixels: %d" % int(ties.sum())
    for name in REPLAY_EVENTS + (("coated_end_ng",) if smooth else ()) + (("coated_sky",) if sky else ()):
        assert int(model.pixel_events[name][keep].sum()) > 0, name
    assert np.array_equal(sc.read_rnds()[keep], want_seeds[keep])
    scale = float(want[keep].max())
    err = np.abs(got[keep] - want[keep])
    bad = err > 2e-3 * np.abs(want[keep]) + 1e-6 * scale
    print("worst error / bound: %.3g" % float((err / (2e-3 * np.abs(want[keep]) + 1e-6 * scale)).max()))
    assert not bad.any(), "%d of %d pixel channels differ; worst %g" % (int(bad.sum()), bad.size, float((err / (np.abs(want[keep]) + 1e-6 * scale)).max()))
    assert float(want[keep].mean()) > 0.0
    off, _ = replay_scene(api, spec, sky, W, H, smooth)
    off.set_option("coated", 0)
    off.iterations = bounces
    off.render_nee(spp, "mis")
    assert not same_bits(off.read_colors()[:, :3], sc.read_colors()[:, :3])


# ---------------------------------------------------------------------------- 6: random streams
def textured_plastic_spec(kd=None, colours=((1.0, 1.0, 1.0), (0.25, 0.25, 0.25))):
    """scenes.cornell_box(coated=True) with lat-long uvs on the plastic sphere and an 8 x 8 checker of `colours`, nearest filtering, bound to
    its material (kd: another albedo for it)"""
    from opencl_path_tracer_amd import scenes
    spec = scenes.cornell_box(coated=True)
    p = len(spec.materials) - 1
    if kd is not None:
        spec.materials[p] = (tuple(kd),) + tuple(spec.materials[p][1:])
    spec.uvs = [None, None, scenes.uv_sphere_uvs(16, 32)]
    spec.textures = [(scenes.checker_texture(8, *colours), dict(filter=0, srgb=0))]
    spec.material_textures = {p: 0}
    return spec


def test_a_texture_on_the_plastic_keeps_the_random_streams(api):
    """A texture draws nothing and changes no pt_nee_rand value, and a type-5 vertex draws its two LCG values whatever its albedo.  What a
    texture on a type-5 material CAN change is the lobe choice, because ps is pinned on kd' (km is the mean of kd'): another lobe, another
    direction, another path.  So the frame keeps rnds and rays bit for bit exactly when the texture leaves km alone, and that is the
    texture used here: grey kd 0.25 under a checker of (2, 1, 0) and (0, 1, 2), whose kd' (0.5, 0.25, 0) and (0, 0.25, 0.5) sum to
    0.75 like kd itself, exactly in float32 in the pinned order.  The colours differ.  With the 1 / 0.25 checker of the guides test
    (which moves km by a factor of 4) 20 of 1,024 pixels end on another LCG state at 4 spp, as measured on the device."""
    W = H = 32
    spec = textured_plastic_spec(kd=(0.25, 0.25, 0.25), colours=((2.0, 1.0, 0.0), (0.0, 1.0, 2.0)))

    def frame(textures):
        sc = api.Scene(W, H).load(spec)
        sc.set_option("coated", 1)
        sc.set_option("textures", textures)
        sc.iterations = CB_BOUNCES
        sc.render_nee(4, "mis")
        out = state(sc)
        sc.close()
        return out
    plain, tex = frame(0), frame(1)
    assert np.array_equal(tex[1], plain[1]) and same_bits(tex[2], plain[2]) and same_bits(tex[3], plain[3])
    assert not same_bits(tex[0], plain[0])


# ---------------------------------------------------------------------------- 7: adaptive NEE frames
@pytest.mark.parametrize("sky,opts,mode", [(False, {}, 0), (True, {}, 0), (True, {"wide_nodes": 2}, 3)])
def test_adaptive_nee_tiles_hold_render_nee_bits(api, sky, opts, mode):
    """k_nee_tiles_coated / k_nee_env_tiles_coated against k_nee_coated / k_nee_env_coated on the replay scene, 16 x 16"""
    from opencl_path_tracer_amd import scenes
    W = H = 16
    spec = replay_spec()

    def scene(coated=1):
        c = api.Scene(W, H)
        for k, v in opts.items():
            c.set_option(k, v)
        c.load(spec)
        assert c.stat("node_mode") == mode
        if sky:
            c.set_environment(scenes.sun_and_sky())
        c.set_option("smooth_normals", 1)
        c.set_option("glossy", 1)
        c.set_option("coated", coated)
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


# ---------------------------------------------------------------------------- 8: determinism
def test_determinism(api):
    W, H = 32, 24
    spec = replay_spec()
    a, _ = replay_scene(api, spec, True, W, H)
    b, _ = replay_scene(api, spec, True, W, H)
    for sc in (a, b):
        sc.iterations = CB_BOUNCES
    a.render_nee(4, "mis")
    a.render_nee(4, "mis")
    b.render_nee(8, "mis")
    assert same_state(state(a), state(b))


# ---------------------------------------------------------------------------- 9: guides
def test_shaded_guides_show_the_plastic(api, oracle):
    from opencl_path_tracer_amd import scenes
    W = H = 32
    spec = textured_plastic_spec()
    spec.normals = scenes.cornell_box(smooth=True).normals
    p = len(spec.materials) - 1
    sc = api.Scene(W, H).load(spec)
    sc.set_option("smooth_normals", 1)

    def guides(shading):
        sc.render_aovs(1, 4, shading=shading)
        alb, nd = sc.read_aovs()
        return alb.copy(), nd.copy()
    off_shaded, off_geo = guides("shaded"), guides("geometric")
    sc.set_option("coated", 1)
    alb, nd = guides("shaded")
    geo = guides("geometric")
    assert same_bits(geo[0], off_geo[0]) and same_bits(geo[1], off_geo[1])            # geometric guides do not follow the option
    pl = alb[:, 3] == p
    assert pl.sum() > 30 and np.array_equal(pl, off_shaded[0][:, 3] == p)
    kd = np.asarray(spec.materials[p][0], dtype=F32)
    # pixels that see the plastic directly (tint 1): kd' = kd without textures
    tri, ns = sc.debug_shading_normals(TG.pixel_rays(api, oracle, spec, W, H))
    first = 12 + spec.objects[1][0].shape[0]
    direct = pl & (tri >= first) & (tri < first + spec.objects[2][0].shape[0])
    assert direct.sum() > 30
    assert same_bits(alb[direct, :3], np.broadcast_to(kd, (int(direct.sum()), 3)))
    assert not off_shaded[0][pl, :3].any()                                             # option off: kd + emission of the inert material is not read: 0
    assert same_bits(alb[~pl], off_shaded[0][~pl]) and same_bits(nd, off_shaded[1])
    s = (np.zeros(3, dtype=F32) + ns[direct, :3]).astype(F32)
    l2 = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
    assert same_bits(nd[direct, :3], s * (F32(1.0) / np.sqrt(l2))[:, None])            # Ns, through the pinned normalisation of pt_render_aovs
    # with option textures the albedo is kd times the checker's texel
    sc.set_option("textures", 1)
    tex, _ = guides("shaded")
    light, dark = kd * F32(1.0), kd * F32(0.25)
    is_light = (tex[direct, :3].view(np.uint32) == light.view(np.uint32)).all(axis=1)
    is_dark = (tex[direct, :3].view(np.uint32) == dark.view(np.uint32)).all(axis=1)
    assert (is_light | is_dark).all() and is_light.any() and is_dark.any()
    sc.set_option("textures", 0)
    sc.set_option("coated", 0)
    again = guides("shaded")
    assert same_bits(again[0], off_shaded[0]) and same_bits(again[1], off_shaded[1])   # and off again: the buffers they were
    sc.close()
