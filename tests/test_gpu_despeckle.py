"""-m gpu: the variance-gated firefly filter (Scene.despeckle, pt_despeckle; pinned in include/pt_api.h).

  * the kernel, through pt_debug_despeckle, on the authored frames of tests/despeckle_ref.py: flags equal to the float64 model's,
    values within 1e-5 of the largest term of each sum, +inf variances and pixels that are not live exact; two runs give the same
    bits; with spread on the frame's sum is kept;
  * a rendered frame (source FRAME) and a temporal result (source TEMPORAL); colors, rnds and the variance read-out stay as they were;
  * the chain into the variance-guided filter (pt_denoise_despeckled) against that filter's float64 model, and when it refuses;
  * quality at the setting of the denoisers' tests, printed as [quality].

Measured on an MI355X (256x256 Cornell box, 16 spp, trial defaults): see profiles/despeckle/README.md."""
import numpy as np
import pytest

import despeckle_ref as D
import variance_ref as V

pytestmark = pytest.mark.gpu

CASES = D.authored()
RTOL = 1e-5          # of the largest magnitude among the terms of each sum: at most 49 additions at 2^-24 each (despeckle_ref.py)


@pytest.fixture(scope="module")
def ctx(api, cb_spec):
    sc = api.Scene(8, 8).load(cb_spec)
    yield sc
    sc.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check_against(name, frame, got, flags, want):
    """got / flags from the device against a model dict (despeckle or replay) for the input `frame`."""
    live = want["live"]
    assert np.array_equal(flags == 2, ~live), name
    assert np.array_equal(_bits(got)[~live], _bits(frame)[~live]), "%s: a pixel that is not live was not copied through" % name
    assert not np.isnan(got[live]).any(), "%s: NaN in a live pixel" % name
    assert np.array_equal(np.isinf(got[..., 3]) & live, np.isinf(want["v"]) & live), "%s: +inf variances differ" % name
    ratio, at = D.check_values(got, want, RTOL)
    print("[despeckle] %-46s flagged %4d  worst error / tolerance %.3f at %s" % (name, int((flags == 1).sum()), ratio, at))
    assert ratio <= 1.0, (name, ratio, at, got[at[:2]], want["c"][at[:2]], want["v"][at[:2]])


# ---------------------------------------------------------------------------------------------------------- 1. authored frames
@pytest.mark.parametrize("k", range(len(CASES)), ids=[n for n, _, _ in CASES])
def test_authored_frame(ctx, k):
    name, frame, params = CASES[k]
    want = D.despeckle(frame, **params)
    got, flags = ctx.debug_despeckle(frame, **params)
    assert flags.shape == frame.shape[:2] and got.shape == frame.shape
    assert np.array_equal(flags, want["flags"]), (name, np.argwhere(flags != want["flags"])[:8])
    _check_against(name, frame, got, flags, want)


# ---------------------------------------------------------------------------------------------------------- 2. determinism
def test_two_runs_same_bits(ctx):
    name, frame, params = next(c for c in CASES if c[0] == D.LARGEST)
    a, fa = ctx.debug_despeckle(frame, **params)
    b, fb = ctx.debug_despeckle(frame, **params)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(fa, fb)


# ---------------------------------------------------------------------------------------------------------- 3. energy
def test_spread_keeps_the_sum(ctx):
    checked = 0
    for name, frame, params in CASES:
        if not params["spread"] or not np.isfinite(frame[..., :3]).all():
            continue
        got, flags = ctx.debug_despeckle(frame, **params)
        before = frame[..., :3].astype(np.float64).sum(axis=(0, 1))
        after = got[..., :3].astype(np.float64).sum(axis=(0, 1))
        assert np.all(np.abs(after - before) <= 1e-5 * np.abs(before)), (name, before, after)
        checked += 1
    assert checked >= 15


# ---------------------------------------------------------------------------------------------------------- 4. a rendered frame
W = H = 64


@pytest.fixture(scope="module")
def rendered(api, cb_spec):
    """The Cornell box with the glass and chrome spheres, 64 x 64, 8 bounces, 16 spp, moments on, default seeds."""
    sc = api.Scene(W, H).load(cb_spec)
    sc.set_option("moments", 1)
    sc.iterations = 8
    sc.render(16)
    yield sc
    sc.close()


def test_rendered_frame(api, rendered):
    sc = rendered
    params = dict(D.DEFAULTS)
    before = (sc.read_colors(), sc.read_rnds(), sc.read_variance())
    assert sc.device_despeckled() is None
    rgbv, flags = sc.despeckle(source=api.PT_DESPECKLE_FRAME, **params)
    after = (sc.read_colors(), sc.read_rnds(), sc.read_variance())
    assert np.array_equal(_bits(before[0]), _bits(after[0])) and np.array_equal(before[1], after[1])
    assert np.array_equal(_bits(before[2]), _bits(after[2]))
    assert sc.device_despeckled()
    again = sc.read_despeckled()
    assert np.array_equal(_bits(again[0]), _bits(rgbv)) and np.array_equal(again[1], flags)
    frame = np.concatenate([before[0][:, :3], before[2].reshape(-1, 1)], axis=1).reshape(H, W, 4)
    got, flags = rgbv.reshape(H, W, 4), flags.reshape(H, W)
    want = D.despeckle(frame, **params)
    close = want["margin"] < 1e-5
    print("[despeckle] rendered 64x64: flagged %d, pixels with a decision margin under 1e-5: %d" % (int((flags == 1).sum()), int(close.sum())))
    assert close.mean() <= 0.005                               # the model alone: does not depend on the kernel
    differ = flags != want["flags"]
    assert not (differ & ~close).any(), np.argwhere(differ & ~close)[:8]
    assert (flags == 1).sum() >= 1
    _check_against("rendered 64x64", frame, got, flags, D.replay(frame, flags, **params))
    # the same frame through the debug entry: the same kernel, the same bits
    dbg, dflags = sc.debug_despeckle(frame, **params)
    assert np.array_equal(_bits(dbg), _bits(got)) and np.array_equal(dflags, flags)


def test_frame_source_needs_valid_moments(api, cb_spec):
    sc = api.Scene(16, 16).load(cb_spec)
    sc.iterations = 4
    sc.render(2)                                               # moments off
    with pytest.raises(api.PtError) as e:
        sc.despeckle()
    assert e.value.code == api.PT_EINVAL and "moments" in str(e.value)
    with pytest.raises(api.PtError) as e:
        sc.read_despeckled()
    assert e.value.code == api.PT_EINVAL
    sc.close()


# ---------------------------------------------------------------------------------------------------------- 5. temporal source
def test_temporal_source(api, cb_spec):
    sc = api.Scene(W, H).load(cb_spec)
    sc.set_option("moments", 1)
    sc.iterations = 8
    sc.render(4)
    sc.render_aovs(1, 4)
    with pytest.raises(api.PtError) as e:
        sc.despeckle(source=api.PT_DESPECKLE_TEMPORAL)
    assert e.value.code == api.PT_EINVAL
    sc.temporal_accumulate()
    sc.current_sample = 0
    sc.render(4)
    sc.render_aovs(1, 4)
    sc.temporal_accumulate()
    trgbv, n = sc.read_temporal()
    assert n.max() == 8.0                                      # (a camera at rest: every hit pixel has both frames behind it)
    rgbv, flags = sc.despeckle(source="temporal")
    want, wflags = sc.debug_despeckle(trgbv.reshape(H, W, 4))
    assert np.array_equal(_bits(rgbv.reshape(H, W, 4)), _bits(want)) and np.array_equal(flags.reshape(H, W), wflags)
    again, _ = sc.read_temporal()
    assert np.array_equal(_bits(again), _bits(trgbv))
    # the chain runs on it, and a newer accumulate makes it stale
    out = sc.denoise_despeckled()
    assert np.all(np.isfinite(out[:, :3]))
    sc.current_sample = 0
    sc.render(4)
    sc.render_aovs(1, 4)
    with pytest.raises(api.PtError) as e:
        sc.denoise_despeckled()                                # a frame has started
    assert e.value.code == api.PT_EINVAL
    sc.close()


# ---------------------------------------------------------------------------------------------------------- 6. chain
def _einval(api, call, **kw):
    with pytest.raises(api.PtError) as e:
        call(**kw)
    assert e.value.code == api.PT_EINVAL
    return str(e.value)


def test_chain_matches_filter_model(api, cb_spec):
    """denoise_despeckled against the float64 model of the variance-guided filter (variance_ref.variance_atrous_model, which builds
    on denoise_ref.py) run on read_despeckled(), at test_gpu_denoise_variance.py's tolerance for the same filter."""
    w, h = 96, 64
    sc = api.Scene(w, h).load(cb_spec)
    sc.set_option("moments", 1)
    sc.iterations = 8
    sc.render(16)
    sc.despeckle()
    assert "guides" in _einval(api, sc.denoise_despeckled)                 # without guides
    sc.render_aovs(2, 4)
    rgbv, flags = sc.read_despeckled()
    assert (flags == 1).sum() >= 1
    alb, nd = sc.read_aovs()
    for extra in ({}, {"demodulate": 1, "iterations": 3}):
        params = dict(api.denoise_variance_defaults(), **extra)
        out = sc.denoise_despeckled(**extra)
        model = V.variance_atrous_model(rgbv, rgbv[:, 3], alb, nd, w, h, **params)
        err = np.abs(out.astype(np.float64) - model)
        tol = 2e-5 + 1e-4 * np.abs(model)
        worst = np.unravel_index(np.argmax(err - tol), err.shape)
        assert np.all(err <= tol), "params %s: worst %s gpu %r model %r" % (params, worst, out[worst[0]], model[worst[0]])
    assert not np.array_equal(out, sc.denoise_variance(**extra))           # (the same buffers; not the same input)
    assert np.array_equal(_bits(sc.denoise_despeckled(**extra)), _bits(out))
    _einval(api, sc.denoise_despeckled, iterations=0)
    sc.render(2)                                                          # samples were added: the result is stale
    assert "stale" in _einval(api, sc.denoise_despeckled)
    sc.despeckle()
    sc.denoise_despeckled()
    sc.upload_Materials()                                                 # the scene was uploaded
    _einval(api, sc.denoise_despeckled)
    sc.render_aovs(2, 4)                                                  # fresh guides do not bring the old result back
    assert "has not run" in _einval(api, sc.denoise_despeckled)
    sc.despeckle()
    sc.denoise_despeckled()
    sc.close()


# ---------------------------------------------------------------------------------------------------------- 7. quality
def test_quality(api, cb_spec):
    """The setting of the denoisers' quality tests: 256 x 256, 8 bounces, 16 spp, render_aovs(2, 4), against 4,096 spp.  Only what
    the construction promises is asserted; whether 0.5 x raw is reached is a finding (profiles/despeckle/README.md)."""
    w = h = 256
    ref = api.Scene(w, h, device=0).load(cb_spec)
    ref.iterations = 8
    ref.render(4096)
    gt = ref.read_colors()[:, :3].astype(np.float64)
    ref.close()
    sc = api.Scene(w, h, device=0).load(cb_spec)
    sc.set_option("moments", 1)
    sc.iterations = 8
    sc.render(16)
    raw = sc.read_colors()[:, :3].astype(np.float64)
    sc.render_aovs(2, 4)
    dv = sc.denoise_variance()[:, :3].astype(np.float64)
    rgbv, flags = sc.despeckle()
    ds = rgbv[:, :3].astype(np.float64)
    dd = sc.denoise_despeckled()[:, :3].astype(np.float64)
    sc.close()

    def rmse(a):
        return float(np.sqrt(np.mean((a - gt) ** 2)))
    r_raw, r_ds, r_dv, r_dd = rmse(raw), rmse(ds), rmse(dv), rmse(dd)
    print("[quality] 256x256 16 spp: RMSE raw %.5g, despeckled %.5g (%.3f x raw), denoise_variance %.5g (%.3f), denoise_despeckled %.5g (%.3f); "
          "flagged %d" % (r_raw, r_ds, r_ds / r_raw, r_dv, r_dv / r_raw, r_dd, r_dd / r_raw, int((flags == 1).sum())))
    print("[quality] frame means: reference %.6g, raw %.6g, despeckled %.6g, denoise_variance %.6g, denoise_despeckled %.6g"
          % (gt.mean(), raw.mean(), ds.mean(), dv.mean(), dd.mean()))
    assert r_ds < r_raw, (r_raw, r_ds)
    assert r_dd <= r_dv, (r_dv, r_dd)
    assert abs(ds.mean() - raw.mean()) <= 1e-4 * raw.mean(), (raw.mean(), ds.mean())
