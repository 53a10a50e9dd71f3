"""-m gpu: temporal accumulation with reprojection (Scene.temporal_accumulate, pt_temporal_accumulate; pinned in include/pt_api.h).

  * a camera at rest: K frames of k samples accumulate to one frame of K k samples (the same LCG stream), n = K k;
  * max_history = 0 gives the frame's own bits; a moving camera, a disocclusion and adaptive frames match the float64 model
    (tests/temporal_ref.py) away from its decision boundaries;
  * the refusals, determinism, pt_denoise_temporal against the variance filter's model, and the quality of a panning camera."""

import numpy as np
import pytest

import temporal_ref as T
import variance_ref as V

pytestmark = pytest.mark.gpu


def _params(api, **kw):
    return dict(api.temporal_defaults(), **kw)


def _frame(sc, k):
    """One frame of k samples started at current_sample 0 with moments on, and its guides."""
    sc.current_sample = 0
    sc.render(k)
    sc.render_aovs(1, 4)


def _model(api, sc, hist, W, H, **kw):
    alb, nd = sc.read_aovs()
    return T.accumulate(hist, sc.camera, sc.read_colors(), sc.sample_counts().reshape(-1), alb, nd, W, H, **_params(api, **kw))


def _check(sc, hist, info, what):
    """The device's last accumulate against the model, where the model has no pixel near a decision (and no tainted history)."""
    rgbv, n = sc.read_temporal()
    ok = ~hist.bad
    assert ok.mean() >= 0.99, "%s: only %.4f of the pixels compared" % (what, ok.mean())
    c, m = rgbv[ok, :3].astype(np.float64), hist.c[ok]
    err = np.abs(c - m) - hist.tol_c[ok, None]
    w = np.unravel_index(np.argmax(err), err.shape)[0]
    assert np.all(err <= 0), "%s: colour, worst %r at %r: %r vs %r" % (what, np.max(err), w, c[w], m[w])
    assert np.all(np.abs(n[ok] - hist.n[ok]) <= 1e-5 * hist.n[ok]), what
    v, vm = rgbv[ok, 3].astype(np.float64), info["v"][ok]
    fin = np.isfinite(vm)
    assert np.array_equal(np.isfinite(v), fin), what
    tol = info["tol_v"][ok][fin]
    w = int(np.argmax(np.abs(v[fin] - vm[fin]) - tol))
    assert np.all(np.abs(v[fin] - vm[fin]) <= tol), "%s: variance %r vs %r (tol %r)" % (what, v[fin][w], vm[fin][w], tol[w])
    return rgbv, n


def _moving_views(spec, steps):
    """(fov, yaw, pitch, shift) per frame: the scene's view, then each step (dfov, dyaw, dpitch, forward, rightward, upward) applied."""
    import opencl_path_tracer_amd.api as api
    fov, yaw, pitch, shift = spec.fov, spec.yaw, spec.pitch, tuple(spec.shift)
    views = [(fov, yaw, pitch, shift)]
    for dfov, dyaw, dpitch, fwd, rgt, upw in steps:
        fov, yaw, pitch = fov + dfov, yaw + dyaw, pitch + dpitch
        shift = api.camera_move(shift, yaw, pitch, fwd, rgt, upw)
        views.append((fov, yaw, pitch, shift))
    return views


def _scene(api, spec, W, H, bounces=4):
    sc = api.Scene(W, H).load(spec)
    sc.iterations = bounces
    sc.set_option("moments", 1)
    return sc


# ---- 1. a camera at rest: four frames of 4 samples are one frame of 16
def test_still_camera_is_one_long_frame(api, cb_spec):
    W, H = 64, 48
    a = _scene(api, cb_spec, W, H)
    a.seed_default()
    for _ in range(4):
        _frame(a, 4)
        a.temporal_accumulate(max_history=64)
    rgbv, n = a.read_temporal()
    _, nd = a.read_aovs()
    a.close()
    b = _scene(api, cb_spec, W, H)
    b.seed_default()
    b.render(16)
    ref, vref = b.read_colors(), b.read_variance().reshape(-1)
    b.close()
    hit = nd[:, 3] >= 0
    assert hit.mean() > 0.9
    assert np.all(n[hit] == 16) and np.all(n[~hit] == 4)
    assert np.allclose(rgbv[hit, :3], ref[hit, :3], rtol=1e-4, atol=1e-6)
    m2 = ref[hit, 3].astype(np.float64)
    assert np.all(np.abs(rgbv[hit, 3] - vref[hit]) <= 1e-4 * vref[hit] + 1e-5 * m2 / 15 + 1e-12)


# ---- 2. max_history = 0 restarts: the frame's own bits, n = k
def test_max_history_zero_is_the_frame(api, cb_spec):
    W, H = 48, 32
    sc = _scene(api, cb_spec, W, H)
    _frame(sc, 4)
    sc.temporal_accumulate()
    _frame(sc, 3)
    rgbv = sc.temporal_accumulate(max_history=0)
    _, n = sc.read_temporal()
    cols = sc.read_colors()
    assert np.array_equal(rgbv[:, :3].view(np.uint32), cols[:, :3].view(np.uint32))
    assert np.array_equal(rgbv[:, 3].view(np.uint32), sc.read_variance().reshape(-1).view(np.uint32))
    assert np.all(n == 3)
    sc.close()


# ---- 3. a moving camera against the model
def test_moving_camera_matches_model(api, cb_spec):
    W, H = 96, 64
    sc = _scene(api, cb_spec, W, H)
    hist = None
    for i, view in enumerate(_moving_views(cb_spec, [(0.5, 0.4, -0.3, 3.0, 2.0, -1.0), (-0.8, -0.6, 0.5, -4.0, -3.0, 2.0)])):
        sc.set_view(*view)
        _frame(sc, 4)
        sc.temporal_accumulate()
        hist, info = _model(api, sc, hist, W, H)
        rgbv, n = _check(sc, hist, info, "frame %d" % i)
    assert np.mean(n > 4) > 0.5                                 # most pixels found history
    sc.close()


# ---- 4. disocclusion: pixels with no valid tap start over
def test_disocclusion(api, cb_spec):
    W, H = 96, 64
    sc = _scene(api, cb_spec, W, H)
    hist = None
    for view in _moving_views(cb_spec, [(0.0, 0.0, 0.0, 0.0, 60.0, 0.0)]):
        sc.set_view(*view)
        _frame(sc, 4)
        sc.temporal_accumulate()
        hist, info = _model(api, sc, hist, W, H)
    rgbv, n = _check(sc, hist, info, "disocclusion")
    fresh = info["no_tap"] & ~hist.bad
    assert 0 < fresh.sum() < (~hist.bad).sum()
    assert np.all(n[fresh] == 4)
    sc.close()


# ---- 5. adaptive frames: k per pixel from the tile counts
def test_adaptive_frames(api, cb_spec):
    W, H = 96, 64
    sc = _scene(api, cb_spec, W, H)
    hist = None
    varied = False
    for view in _moving_views(cb_spec, [(0.0, 0.3, 0.2, 2.0, 1.0, 0.0)]):
        sc.set_view(*view)
        sc.current_sample = 0
        sc.render_adaptive(4, 16, 0.5)
        sc.render_aovs(1, 4)
        varied |= len(set(sc.sample_counts().reshape(-1).tolist())) > 1
        sc.temporal_accumulate()
        hist, info = _model(api, sc, hist, W, H)
        _check(sc, hist, info, "adaptive")
    assert varied
    sc.close()


# ---- 6. refusals
def _einval(api, fn):
    with pytest.raises(api.PtError) as e:
        fn()
    assert e.value.code == api.PT_EINVAL
    return str(e.value)


def test_refusals(api, cb_spec):
    W, H = 32, 24
    sc = _scene(api, cb_spec, W, H)
    sc.render(2)
    sc.render_aovs(1, 4)
    _einval(api, sc.denoise_temporal)                            # before any accumulate
    sc.temporal_accumulate()
    sc.denoise_temporal()
    assert "already" in _einval(api, sc.temporal_accumulate)     # the same frame twice
    sc.render_aovs(1, 4)
    _einval(api, sc.denoise_temporal)                            # new guides
    views = _moving_views(cb_spec, [(0.0, 1.0, 0.0, 0.0, 0.0, 0.0)])
    sc.current_sample = 0
    sc.render(2)
    sc.set_view(*views[1])
    sc.render_aovs(1, 4)
    assert "camera" in _einval(api, sc.temporal_accumulate)      # guides of another camera
    sc.render(2)                                                 # the same frame goes on through the second camera
    assert "camera" in _einval(api, sc.temporal_accumulate)
    sc.set_option("moments", 0)
    _frame(sc, 2)
    assert "moments" in _einval(api, sc.temporal_accumulate)
    sc.set_option("moments", 1)
    _frame(sc, 2)
    sc.temporal_accumulate()
    assert np.any(sc.read_temporal()[1] > 2)                     # the history carried on through the refusals
    sc.upload_Materials()                                        # drops the history
    _frame(sc, 2)
    sc.temporal_accumulate()
    assert np.all(sc.read_temporal()[1] == 2)
    sc.close()
    tiled = api.Scene(W, H, rank=0, world=2).load(cb_spec)
    tiled.set_option("moments", 1)
    tiled.render(2)
    tiled.render_aovs(1, 4)
    assert "world" in _einval(api, tiled.temporal_accumulate)
    tiled.close()


# ---- 7. determinism
def test_determinism(api, cb_spec):
    W, H = 64, 48
    out = []
    for _ in range(2):
        sc = _scene(api, cb_spec, W, H)
        for view in _moving_views(cb_spec, [(0.3, 0.5, -0.2, 2.0, 3.0, 1.0), (0.0, -0.4, 0.1, 1.0, -2.0, 0.0)]):
            sc.set_view(*view)
            _frame(sc, 3)
            sc.temporal_accumulate()
        out.append(sc.read_temporal())
        sc.close()
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))


# ---- 8. pt_denoise_temporal is the variance filter on the accumulated colour and variance
def test_denoise_temporal_matches_variance_model(api, cb_spec):
    W, H = 96, 64
    sc = _scene(api, cb_spec, W, H)
    for view in _moving_views(cb_spec, [(0.0, 0.5, 0.0, 0.0, 3.0, 0.0)]):
        sc.set_view(*view)
        _frame(sc, 4)
        sc.temporal_accumulate()
    rgbv, _ = sc.read_temporal()
    alb, nd = sc.read_aovs()
    for kw in ({}, {"demodulate": 1, "iterations": 3}):
        out = sc.denoise_temporal(**kw)
        model = V.variance_atrous_model(rgbv, rgbv[:, 3], alb, nd, W, H, **dict(api.denoise_variance_defaults(), **kw))
        err = np.abs(out.astype(np.float64) - model) - (2e-5 + 1e-4 * np.abs(model))
        assert np.all(err <= 0), (kw, np.max(err))
    sc.close()


# ---- 9. quality of a moving camera
def _quality(api, cb_spec, step, label):
    W = H = 128
    B, K, k = 4, 16, 4
    views = _moving_views(cb_spec, [step] * (K - 1))
    ref = api.Scene(W, H).load(cb_spec)
    ref.iterations = B
    ref.set_view(*views[-1])
    ref.upload_seeds(np.random.default_rng(12345).integers(1, 2 ** 31 - 1, W * H, dtype=np.int64).astype(np.int32))
    ref.render(2048)
    gt = ref.read_colors()[:, :3].astype(np.float64)
    ref.close()
    sc = _scene(api, cb_spec, W, H, B)
    for view in views:
        sc.set_view(*view)
        _frame(sc, k)
        tv = sc.temporal_accumulate()
    raw = sc.read_colors()
    dt = sc.denoise_temporal()
    dv = sc.denoise_variance()
    _, n = sc.read_temporal()
    sc.close()

    def rmse(a):
        d = a[:, :3].astype(np.float64) - gt
        return float(np.sqrt(np.mean(d * d)))
    r = {"raw": rmse(raw), "temporal": rmse(tv), "denoise_temporal": rmse(dt), "denoise_variance": rmse(dv),
         "mean_ref": float(gt.mean()), "mean_temporal": float(tv[:, :3].astype(np.float64).mean()), "n_mean": float(n.mean())}
    print("[quality] %s 128x128 %d frames of %d spp: raw %.4g, temporal %.4g (%.3fx), denoise_temporal %.4g (%.3fx), denoise_variance "
          "%.4g (%.3fx), mean %.4g vs %.4g, mean n %.1f" % (label, K, k, r["raw"], r["temporal"], r["temporal"] / r["raw"],
                                                             r["denoise_temporal"], r["denoise_temporal"] / r["raw"], r["denoise_variance"],
                                                             r["denoise_variance"] / r["raw"], r["mean_temporal"], r["mean_ref"], r["n_mean"]))
    return r


@pytest.mark.parametrize("label", ["pan", "sideways"])
def test_quality_moving_camera(api, cb_spec, label):
    # half a pixel per frame: by yaw, or sideways by half the footprint of a pixel at the back of the box (~1,300 units away)
    step = (0.0, 0.5 * cb_spec.fov / 128.0, 0.0, 0.0, 0.0, 0.0) if label == "pan" else \
        (0.0, 0.0, 0.0, 0.0, 0.5 * 2.0 * 1300.0 * np.tan(np.radians(cb_spec.fov / 2.0)) / 128.0, 0.0)
    r = _quality(api, cb_spec, step, label)
    assert r["temporal"] <= 0.6 * r["raw"], r
    assert r["denoise_temporal"] < r["denoise_variance"], r
    assert abs(r["mean_temporal"] - r["mean_ref"]) <= 0.03 * r["mean_ref"], r
