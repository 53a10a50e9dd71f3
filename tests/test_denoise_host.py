"""-m "not gpu": guide buffers and the a-trous denoiser without a device -- argument checking on a host-only context, the
defaults, and self-checks of the float64 filter model the GPU tests compare against (tests/denoise_ref.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import denoise_ref as R


def _params(api, **kw):
    p = api.DenoiseParams(**api.denoise_defaults())
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("sub,depth", [(0, 4), (9, 4), (-1, 0), (1, -1), (1, 17), (2, 1000)])
def test_render_aovs_bad_arguments(api, cb_spec, sub, depth):
    sc = api.Scene(16, 12, device=None).load(cb_spec)
    assert api.LIB.pt_render_aovs(sc._h, api._ptr(sc.camera), sub, depth) == api.PT_EINVAL
    assert b"pt_render_aovs" in api.LIB.pt_last_error(sc._h)


def test_render_aovs_host_only(api, cb_spec):
    """Valid arguments on a host-only context: refused like every other render call (no CPU path)."""
    sc = api.Scene(16, 12, device=None).load(cb_spec)
    with pytest.raises(api.PtError) as e:
        sc.render_aovs(2, 4)
    assert e.value.code == api.PT_ENODEVICE
    with pytest.raises(api.PtError):
        sc.read_aovs()
    with pytest.raises(api.PtError):
        sc.read_denoised()
    assert sc.device_denoised() is None


@pytest.mark.parametrize("kw", [
    {"iterations": 0}, {"iterations": 11}, {"iterations": -3},
    {"sigma_color": -1.0}, {"sigma_normal": -0.5}, {"sigma_depth": -1e-9},
    {"sigma_color": float("nan")}, {"sigma_normal": float("nan")}, {"sigma_depth": float("nan")},
    {"sigma_color": -float("inf")},
])
def test_denoise_bad_arguments(api, cb_spec, kw):
    sc = api.Scene(16, 12, device=None).load(cb_spec)
    assert api.LIB.pt_denoise(sc._h, C.byref(_params(api, **kw))) == api.PT_EINVAL
    assert b"pt_denoise" in api.LIB.pt_last_error(sc._h)


def test_denoise_without_guides(api, cb_spec):
    sc = api.Scene(16, 12, device=None).load(cb_spec)
    with pytest.raises(api.PtError) as e:
        sc.denoise()
    assert e.value.code == api.PT_EINVAL and "guides" in str(e.value)
    assert api.LIB.pt_denoise(sc._h, None) == api.PT_EINVAL
    tiled = api.Scene(16, 16, device=None, rank=0, world=2).load(cb_spec)
    assert api.LIB.pt_denoise(tiled._h, C.byref(_params(api))) == api.PT_EINVAL
    assert b"world" in api.LIB.pt_last_error(tiled._h)


def test_defaults_fill_every_field(api):
    p = api.DenoiseParams(-7, float("nan"), float("nan"), float("nan"), -7)
    api.LIB.pt_denoise_defaults(C.byref(p))
    assert 1 <= p.iterations <= 10
    for s in (p.sigma_color, p.sigma_normal, p.sigma_depth):
        assert s >= 0 and not math.isnan(s)
    assert p.demodulate in (0, 1)
    assert api.denoise_defaults() == p.as_dict()


# ---- the float64 model (what the GPU filter is compared against)
def _frame(W, H, seed=3):
    rng = np.random.RandomState(seed)
    colors = np.zeros((W * H, 4), dtype=np.float32)
    colors[:, :3] = rng.gamma(1.5, 0.6, size=(W * H, 3))
    albedo = np.zeros((W * H, 4), dtype=np.float32)
    albedo[:, :3] = rng.uniform(0.0, 0.9, size=(W * H, 3))
    nd = np.zeros((W * H, 4), dtype=np.float32)
    n = rng.normal(size=(W * H, 3))
    nd[:, :3] = n / np.linalg.norm(n, axis=1, keepdims=True)
    nd[:, 3] = rng.uniform(100.0, 900.0, size=W * H)
    return colors, albedo, nd


@pytest.mark.parametrize("W,H,L", [(23, 17, 1), (40, 24, 3), (64, 48, 5)])
def test_model_all_terms_off_is_b3(W, H, L):
    colors, albedo, nd = _frame(W, H)
    out = R.atrous_model(colors, albedo, nd, W, H, iterations=L, sigma_color=np.inf, sigma_normal=0.0, sigma_depth=np.inf, demodulate=0)
    assert np.allclose(out[:, :3], R.b3_blur(colors, W, H, L), rtol=1e-13, atol=0)
    assert np.all(out[:, 3] == 1.0)
    # sigma_normal = +inf turns the normal term off as well
    out2 = R.atrous_model(colors, albedo, nd, W, H, iterations=L, sigma_normal=np.inf)
    assert np.array_equal(out, out2)


def test_b3_blur_by_hand():
    """One interior pixel of one iteration against the 25-tap sum written out."""
    W, H = 9, 9
    colors, _, _ = _frame(W, H, seed=5)
    x = colors[:, :3].astype(np.float64).reshape(H, W, 3)
    want = np.zeros(3)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            want += R.KERNEL[dx + 2] * R.KERNEL[dy + 2] * x[4 + dy, 4 + dx]
    assert np.allclose(R.b3_blur(colors, W, H, 1).reshape(H, W, 3)[4, 4], want, rtol=1e-14)


@pytest.mark.parametrize("demod", [0, 1])
def test_model_constant_stays_constant(demod):
    W, H = 40, 24
    _, albedo, nd = _frame(W, H)
    nd[::7, 3] = -1.0                      # some misses
    nd[::7, :3] = 0.0
    colors = np.zeros((W * H, 4), dtype=np.float32)
    colors[:, :3] = (0.25, 1.5, 3.0)
    if demod:
        albedo[:, :3] = (0.5, 0.25, 0.75)   # constant albedo: the demodulated frame is constant too
    out = R.atrous_model(colors, albedo, nd, W, H, iterations=4, sigma_color=0.5, sigma_normal=64.0, sigma_depth=0.5, demodulate=demod)
    assert np.allclose(out[:, :3], colors[:, :3], rtol=1e-14)


def test_model_no_weight_across_hit_miss():
    """A frame whose left half hits and right half misses: no colour crosses the boundary, with every other term off."""
    W, H = 32, 16
    colors, albedo, nd = _frame(W, H)
    nd = nd.reshape(H, W, 4)
    nd[:, W // 2:, 3] = -1.0
    nd[:, W // 2:, :3] = 0.0
    nd = nd.reshape(-1, 4)
    c = colors.reshape(H, W, 4).copy()
    c[:, W // 2:, :3] = 1000.0
    out = R.atrous_model(c.reshape(-1, 4), albedo, nd, W, H, iterations=5).reshape(H, W, 4)
    left = R.b3_blur(c[:, :W // 2].reshape(-1, 4), W // 2, H, 5).reshape(H, W // 2, 3)
    assert np.allclose(out[:, :W // 2, :3], left, rtol=1e-12)
    assert np.allclose(out[:, W // 2:, :3], 1000.0, rtol=1e-14)


def test_model_depth_weight():
    """Two hit pixels one step apart: wz = exp(-|dz| / (sigma_z * z_p)); checked on a 2x1 frame, one iteration."""
    W, H = 2, 1
    colors = np.zeros((2, 4), dtype=np.float32)
    colors[:, :3] = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]
    albedo = np.ones((2, 4), dtype=np.float32)
    nd = np.zeros((2, 4), dtype=np.float32)
    nd[:, 3] = [100.0, 150.0]
    sz = 0.5
    out = R.atrous_model(colors, albedo, nd, W, H, iterations=1, sigma_depth=sz)
    wz = math.exp(-50.0 / (sz * 100.0))
    h = R.KERNEL[2] * R.KERNEL[3]
    want = h * wz / (9.0 / 64.0 + h * wz)
    assert np.allclose(out[0, :3], want, rtol=1e-14)


def test_subpixel_offsets():
    assert R.subpixel_offsets(1) == [(0.5, 0.5)]
    o = R.subpixel_offsets(3)
    assert len(o) == 9 and o[1][0] > o[0][0] and o[1][1] == o[0][1]      # i inner
    assert all(isinstance(a, np.float32) for pair in o for a in pair)
