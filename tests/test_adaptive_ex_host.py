"""-m "not gpu": pt_render_adaptive_ex without a device -- the defaults, argument checking on a host-only context (before the device
is asked for), the butterfly sum of the variance metric's replay (tests/adaptive_variance_ref.py), and the Python entry's dispatch."""
import ctypes as C

import numpy as np
import pytest

import adaptive_variance_ref as AV


def params(api, **kw):
    p = api.AdaptiveParams(**api.adaptive_defaults())
    p.min_spp, p.max_spp, p.threshold = 4, 16, 0.1
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_defaults(api):
    d = api.adaptive_defaults()
    assert (d["min_spp"], d["max_spp"]) == (16, 1024)
    assert d["metric"] == api.PT_ADAPT_VARIANCE == 1 and d["path"] == api.PT_ADAPT_PATH_RENDER == 0
    assert d["strategy"] == api.PT_NEE_MIS and d["tonemapped"] == 1
    assert d["threshold"] > 0 and np.isfinite(d["threshold"])
    assert (api.PT_ADAPT_HALF, api.PT_ADAPT_PATH_NEE) == (0, 1)
    assert C.sizeof(api.AdaptiveParams) == 28
    api.LIB.pt_adaptive_defaults(None)                      # a null pointer is ignored


@pytest.mark.parametrize("kw", [
    {"metric": 2}, {"metric": -1}, {"path": 2}, {"path": -1},
    {"path": 1, "strategy": 3}, {"path": 1, "strategy": -1},
    {"min_spp": 0}, {"min_spp": 1}, {"min_spp": 5}, {"min_spp": 8, "max_spp": 4}, {"min_spp": -2},
    {"threshold": -1.0}, {"threshold": float("nan")}, {"threshold": -float("inf")},
])
def test_invalid_arguments_host_only(api, cb_spec, kw):
    sc = api.Scene(16, 16, device=None).load(cb_spec)
    p = params(api, **kw)
    assert api.LIB.pt_render_adaptive_ex(sc._h, api._ptr(sc.camera), 4, C.byref(p)) == api.PT_EINVAL
    assert b"pt_render_adaptive_ex" in api.LIB.pt_last_error(sc._h)
    sc.close()


def test_null_params_and_bad_iterations(api, cb_spec):
    sc = api.Scene(16, 16, device=None).load(cb_spec)
    assert api.LIB.pt_render_adaptive_ex(sc._h, api._ptr(sc.camera), 4, None) == api.PT_EINVAL
    assert b"pt_render_adaptive_ex" in api.LIB.pt_last_error(sc._h)
    p = params(api)
    assert api.LIB.pt_render_adaptive_ex(sc._h, api._ptr(sc.camera), -1, C.byref(p)) == api.PT_EINVAL
    assert api.LIB.pt_render_adaptive_ex(None, api._ptr(sc.camera), 4, C.byref(p)) == api.PT_EINVAL
    sc.close()


def test_check_order_is_pt_render_adaptives(api, cb_spec):
    """The first thing wrong is the one reported: bounds, threshold, iterations, then metric / path / strategy; all before the device."""
    sc = api.Scene(16, 16, device=None).load(cb_spec)
    cam = api._ptr(sc.camera)

    def msg(it, **kw):
        p = params(api, **kw)
        assert api.LIB.pt_render_adaptive_ex(sc._h, cam, it, C.byref(p)) == api.PT_EINVAL
        return api.LIB.pt_last_error(sc._h)

    assert b"min_spp" in msg(-1, min_spp=3, threshold=-1.0, metric=7)
    assert b"threshold" in msg(-1, threshold=-1.0, metric=7)
    assert b"iterations" in msg(-1, metric=7)
    assert b"metric" in msg(4, metric=7, path=7)
    assert b"path" in msg(4, path=7, strategy=7)
    assert b"strategy" in msg(4, path=1, strategy=7)
    p = params(api, strategy=7)                              # path RENDER ignores the strategy
    assert api.LIB.pt_render_adaptive_ex(sc._h, cam, 4, C.byref(p)) == api.PT_ENODEVICE
    sc.close()


@pytest.mark.parametrize("kw", [{}, {"metric": 0}, {"path": 1}, {"path": 1, "strategy": 0}, {"tonemapped": 0}, {"threshold": float("inf")},
                                {"threshold": 0.0}])
def test_valid_arguments_host_only_need_a_device(api, cb_spec, kw):
    sc = api.Scene(16, 16, device=None).load(cb_spec)
    p = params(api, **kw)
    assert api.LIB.pt_render_adaptive_ex(sc._h, api._ptr(sc.camera), 4, C.byref(p)) == api.PT_ENODEVICE
    sc.close()


def test_work_item_check_belongs_to_the_megakernel_path(api):
    sc = api.Scene(64, 64, device=None)
    cam = api._ptr(sc.camera)
    p = params(api, min_spp=2, max_spp=1 << 26)
    assert api.LIB.pt_render_adaptive_ex(sc._h, cam, 4, C.byref(p)) == api.PT_EINVAL
    assert b"max_spp too large" in api.LIB.pt_last_error(sc._h)
    p.path = api.PT_ADAPT_PATH_NEE
    assert api.LIB.pt_render_adaptive_ex(sc._h, cam, 4, C.byref(p)) == api.PT_ENODEVICE
    sc.close()


# ---------------------------------------------------------------------------- the butterfly against a pairwise tree
def tree_sum(v):
    """A plain pairwise tree in float32 scalars: fold the upper half onto the lower half until one value is left."""
    v = [np.float32(x) for x in v]
    while len(v) > 1:
        half = len(v) // 2
        v = [np.float32(v[i] + v[i + half]) for i in range(half)]
    return v[0]


def test_butterfly_full_tile():
    rng = np.random.default_rng(11)
    lanes = (rng.random(64, dtype=np.float32) * np.float32(3.0)).astype(np.float32)
    s = AV.butterfly_sum(lanes)
    assert s.dtype == np.float32
    assert len(set(s.view(np.uint32).tolist())) == 1, "every lane must hold the same bits"
    assert s.view(np.uint32)[0] == np.float32(tree_sum(lanes)).view(np.uint32)
    assert abs(float(s[0]) - float(lanes.astype(np.float64).sum())) < 1e-4


def test_butterfly_ragged_tile():
    """A 4 x 6 frame is one tile with 4 columns x 6 rows inside: lanes (y&7)*8 + (x&7), 0 elsewhere; the divisor is 24."""
    W, H = 4, 6
    rng = np.random.default_rng(12)
    vals = rng.random(W * H, dtype=np.float32)
    lanes = AV.tile_lanes(vals, W, H)
    assert lanes.shape == (1, 64)
    want = np.zeros(64, np.float32)
    for y in range(H):
        for x in range(W):
            want[(y & 7) * 8 + (x & 7)] = vals[y * W + x]
    assert np.array_equal(lanes[0], want)
    s = AV.butterfly_sum(lanes)
    assert len(set(s.view(np.uint32).reshape(-1).tolist())) == 1
    assert s.view(np.uint32)[0, 0] == np.float32(tree_sum(want)).view(np.uint32)
    assert AV.pixels_inside(W, H).tolist() == [24]
    assert AV.pixels_inside(100, 70).reshape(9, 13)[-1, -1] == 4 * 6 and AV.pixels_inside(100, 70)[0] == 64


def test_tile_errors_formula():
    """One tile, hand-made moments: e = sqrt(mean v), v = max(m2 - mu^2, 0) / (b - 1), divided by (1 + mu)^4 when tonemapped."""
    c = np.zeros((64, 4), np.float32)
    c[:, :3] = 0.5                                           # mu = 0.5 (the weights sum to 1 up to rounding)
    c[:, 3] = 0.5
    mu = AV.luminance(c)
    v = np.maximum(AV.fmaf(-mu, mu, c[:, 3]), np.float32(0)) / np.float32(7)
    e = AV.tile_errors(c, 8, 8, 8, 0)
    assert e.shape == (1,) and abs(float(e[0]) - float(np.sqrt(v.astype(np.float64).mean()))) < 1e-6
    et = AV.tile_errors(c, 8, 8, 8, 1)
    assert abs(float(et[0]) - float(e[0]) / (1.5 * 1.5)) < 1e-6
    c[5, 3] = np.nan
    assert np.isposinf(AV.tile_errors(c, 8, 8, 8, 0)[0])
    c[:, 3] = 0.0                                            # m2 < mu^2 clamps to 0
    assert AV.tile_errors(c, 8, 8, 8, 0)[0] == 0


def test_replay_half_is_adaptive_refs():
    import adaptive_ref as R
    W = H = 16
    rn = np.arange(W * H, dtype=np.int32)
    snaps = {}
    for b in (1, 2, 4, 8):
        c = np.full((W * H, 4), 0.25, np.float32)
        if b >= 2:
            c[:8, 0] = 0.25 + 0.5 / b
        snaps[b] = (c, rn + b)
    a, r = AV.replay(snaps, W, H, 2, 8, 0.01, metric=AV.HALF), R.replay(snaps, W, H, 2, 8, 0.01)
    for k in ("spp", "err", "colors", "rnds", "pixel_spp"):
        assert np.array_equal(a[k], r[k])
    assert a["rounds"] == r["rounds"] and a["active_tiles"] == r["active_tiles"]


# ---------------------------------------------------------------------------- Scene.render_adaptive dispatch
class _Spy:
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        self.calls.append(name)
        return getattr(self._lib, name)


def test_python_entry_dispatch(api, cb_spec, monkeypatch):
    sc = api.Scene(16, 16, device=None).load(cb_spec)
    spy = _Spy(api.LIB)
    monkeypatch.setattr(api, "LIB", spy)
    with pytest.raises(api.PtError) as e:
        sc.render_adaptive(4, 16, 0.5)
    assert e.value.code == api.PT_ENODEVICE
    assert "pt_render_adaptive" in spy.calls and "pt_render_adaptive_ex" not in spy.calls
    for kw in ({"metric": "variance"}, {"path": "nee"}, {"strategy": "light"}, {"tonemapped": 0}, {"metric": api.PT_ADAPT_HALF}):
        spy.calls.clear()
        with pytest.raises(api.PtError) as e:
            sc.render_adaptive(4, 16, 0.5, **kw)
        assert e.value.code == api.PT_ENODEVICE
        assert "pt_render_adaptive_ex" in spy.calls and "pt_render_adaptive" not in spy.calls
    with pytest.raises(TypeError):
        sc.render_adaptive(4, 16, 0.5, metrics="variance")
    with pytest.raises(KeyError) as e:
        sc.render_adaptive(4, 16, 0.5, metric="halves")
    assert "half" in str(e.value) and "variance" in str(e.value)
    with pytest.raises(TypeError):
        sc.render_adaptive(4, 16, 0.5, tonemapped="1")
    monkeypatch.undo()
    sc.close()
