"""-m "not gpu": the second-moment option and the variance read-out without a device -- option and argument checks on a host-only
context, and self-checks of the float32 statements the GPU tests compare against (tests/variance_ref.py)."""
import numpy as np
import pytest

import variance_ref as V


def test_exports_name_the_new_entry_points(api):
    for name in ("pt_read_variance", "pt_device_variance"):
        assert name in api.EXPORTS
        assert hasattr(api.LIB, name)


def test_moments_option(api, cb_spec):
    sc = api.Scene(16, 12, device=None).load(cb_spec)
    sc.set_option("moments", 1)
    sc.set_option("moments", 0)
    for bad in (2, -1, 7):
        assert api.LIB.pt_set_option(sc._h, b"moments", bad) == api.PT_EINVAL
        assert b"moments" in api.LIB.pt_last_error(sc._h)


def test_read_variance_host_only(api, cb_spec):
    sc = api.Scene(16, 12, device=None).load(cb_spec)
    sc.set_option("moments", 1)
    with pytest.raises(api.PtError) as e:
        sc.read_variance()
    assert e.value.code == api.PT_ENODEVICE
    out = np.empty(16 * 12, np.float32)
    assert api.LIB.pt_read_variance(sc._h, api._ptr(out), out.size) == api.PT_ENODEVICE
    assert api.LIB.pt_device_variance(sc._h) is None
    assert api.LIB.pt_read_variance(None, api._ptr(out), out.size) == api.PT_EINVAL
    assert api.LIB.pt_device_variance(None) is None


def test_luminance_pins():
    c = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [0, 0, 0]], np.float32)
    l = V.luminance(c)
    assert l[0] == np.float32(0.2126) and l[1] == np.float32(0.7152) and l[2] == np.float32(0.0722)
    assert abs(float(l[3]) - 1.0) < 1e-6 and l[4] == 0


def test_fold_moment_is_the_running_mean_of_squares():
    rng = np.random.default_rng(3)
    xs = rng.random((40, 5, 3), dtype=np.float32) * 4
    m2 = np.zeros(5, np.float32)
    for s in range(xs.shape[0]):
        m2 = V.fold_moment(m2, xs[s], s)
    want = np.mean(V.luminance(xs.reshape(-1, 3)).astype(np.float64).reshape(40, 5) ** 2, axis=0)
    assert np.allclose(m2, want, rtol=1e-5)
    one = V.fold_moment(np.full(5, 123.0, np.float32), xs[0], 0)        # sample 0 starts from 0 whatever is in .w
    assert np.array_equal(one, V.luminance(xs[0]) * V.luminance(xs[0]))


def test_variance_formula():
    rng = np.random.default_rng(5)
    x = (rng.random((64, 10, 3)) * 2).astype(np.float32)
    mean = np.zeros((10, 3), np.float32)
    m2 = np.zeros(10, np.float32)
    for s in range(x.shape[0]):
        mean = ((mean * np.float32(s)) + x[s]) / np.float32(s + 1)
        m2 = V.fold_moment(m2, x[s], s)
    colors = np.concatenate([mean, m2[:, None]], axis=1)
    v = V.variance(colors, 64)
    l = V.luminance(x.reshape(-1, 3)).astype(np.float64).reshape(64, 10)
    assert np.allclose(v, np.var(l, axis=0, ddof=0) / 63, rtol=1e-3, atol=1e-9)
    assert np.all(np.isinf(V.variance(colors, 1))) and np.all(np.isinf(V.variance(colors, 0)))
    assert np.all(V.variance(np.array([[1, 1, 1, 0.5]], np.float32), 4) == 0)     # m2 < mu^2 (rounding): clamped at 0


# ---- the variance-guided filter: defaults, argument checks, and the float64 model's own sanity
def test_denoise_variance_defaults(api):
    d = api.denoise_variance_defaults()
    assert d["iterations"] == 2 and d["demodulate"] == 0
    assert d["sigma_luminance"] == np.float32(4.0)
    assert d["sigma_normal"] == np.float32(8.0) and d["sigma_depth"] == np.float32(0.05)
    nd = api.denoise_defaults()
    assert (d["sigma_normal"], d["sigma_depth"]) == (nd["sigma_normal"], nd["sigma_depth"])


@pytest.mark.parametrize("kw", [
    {"iterations": 0}, {"iterations": 11}, {"sigma_luminance": -1.0}, {"sigma_normal": -0.5}, {"sigma_depth": -1e-9},
    {"sigma_luminance": float("nan")}, {"sigma_normal": float("nan")}, {"sigma_depth": float("nan")},
])
def test_denoise_variance_bad_arguments(api, cb_spec, kw):
    import ctypes as C
    sc = api.Scene(16, 12, device=None).load(cb_spec)
    p = api.DenoiseVarianceParams(**dict(api.denoise_variance_defaults(), **kw))
    assert api.LIB.pt_denoise_variance(sc._h, C.byref(p)) == api.PT_EINVAL
    assert b"pt_denoise_variance" in api.LIB.pt_last_error(sc._h)


def test_denoise_variance_without_guides_or_device(api, cb_spec):
    import ctypes as C
    sc = api.Scene(16, 12, device=None).load(cb_spec)
    with pytest.raises(api.PtError) as e:
        sc.denoise_variance()
    assert e.value.code == api.PT_EINVAL and "guides" in str(e.value)
    assert api.LIB.pt_denoise_variance(sc._h, None) == api.PT_EINVAL
    tiled = api.Scene(16, 16, device=None, rank=0, world=2).load(cb_spec)
    p = api.DenoiseVarianceParams(**api.denoise_variance_defaults())
    assert api.LIB.pt_denoise_variance(tiled._h, C.byref(p)) == api.PT_EINVAL
    assert b"world" in api.LIB.pt_last_error(tiled._h)
    with pytest.raises(api.PtError) as e:
        sc.device_variance()
    assert e.value.code == api.PT_ENODEVICE


def _guides(W, H, rng):
    alb = np.zeros((W * H, 4), np.float32)
    alb[:, :3] = rng.random((W * H, 3)) * 0.8 + 0.1
    nd = np.zeros((W * H, 4), np.float32)
    n = rng.normal(size=(W * H, 3))
    nd[:, :3] = n / np.linalg.norm(n, axis=1, keepdims=True)
    nd[:, 3] = rng.random(W * H) * 10 + 1
    return alb, nd


def test_model_constant_frame_stays_constant():
    W, H = 23, 17
    rng = np.random.default_rng(1)
    alb, nd = _guides(W, H, rng)
    c = np.tile(np.array([[0.3, 1.2, 2.5, 0]], np.float32), (W * H, 1))
    v = rng.random(W * H).astype(np.float32)
    out = V.variance_atrous_model(c, v, alb, nd, W, H, demodulate=0)
    assert np.allclose(out[:, :3], c[:, :3], rtol=1e-12)


def test_model_infinite_sigma_is_the_bspline_average():
    import denoise_ref as R
    W, H = 29, 21
    rng = np.random.default_rng(2)
    alb, nd = _guides(W, H, rng)
    nd[:, 3] = 5.0                                          # every pixel a hit: no hit / miss edges
    c = rng.random((W * H, 4)).astype(np.float32)
    v = rng.random(W * H).astype(np.float32)
    for L in (1, 3):
        out = V.variance_atrous_model(c, v, alb, nd, W, H, iterations=L, sigma_luminance=np.inf, sigma_normal=0.0,
                                      sigma_depth=np.inf, demodulate=0)
        assert np.allclose(out[:, :3], R.b3_blur(c, W, H, L), rtol=1e-12, atol=1e-14)


def test_model_zero_variance_stays_zero():
    W, H = 19, 13
    rng = np.random.default_rng(3)
    alb, nd = _guides(W, H, rng)
    c = rng.random((W * H, 4)).astype(np.float32)
    for dm in (0, 1):
        out = V.variance_atrous_model(c, np.zeros(W * H, np.float32), alb, nd, W, H, iterations=3, sigma_luminance=np.inf, demodulate=dm)
        assert np.all(out[:, 3] == 0)
    # and positive variance shrinks: a weighted mean of independent pixels has at most the largest input variance
    v = rng.random(W * H).astype(np.float32)
    out = V.variance_atrous_model(c, v, alb, nd, W, H, iterations=3, demodulate=0)
    assert np.all(out[:, 3] >= 0) and out[:, 3].mean() < v.mean()
