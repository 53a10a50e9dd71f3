"""-m "not gpu": temporal accumulation without a device -- the pinned defaults, the reprojection (pt_debug_reproject, the statement
k_temporal shares) against a float64 projection, and the argument checks that come before the device."""
import ctypes as C

import numpy as np
import pytest

import temporal_ref as T

W, H = 128, 96


def _cameras(api):
    """Cameras of pt_camera_init / pt_camera_move at several views, and a hand-made skewed one (axes not orthogonal, unequal lengths)."""
    out = [api.Camera(60.0, 0.0, 0.0, (0.0, 0.0, 0.0), W, H), api.Camera(75.0, -63.8, 15.6, (265.06, 162.31, 360.41), W, H)]
    shift = (0.0, 0.0, 0.0)
    for yaw, pitch, fwd, rgt, upw in ((3.0, -2.0, 40.0, -25.0, 10.0), (-10.0, 5.0, -60.0, 30.0, -15.0), (20.0, 12.0, 5.0, 80.0, 0.0)):
        shift = api.camera_move(shift, yaw, pitch, fwd, rgt, upw)
        out.append(api.Camera(55.0 + yaw, yaw, pitch, shift, W, H))
    sk = api.Camera(60.0, 8.0, -4.0, (20.0, -10.0, 30.0), W, H)
    sk["right"][0][:3] = sk["right"][0][:3] * 1.1 + sk["up"][0][:3] * 0.15
    sk["up"][0][:3] = sk["up"][0][:3] * 0.9 + np.array([3.0, 0.0, -2.0], np.float32)
    sk["lookat"][0][:3] = sk["lookat"][0][:3] + np.array([5.0, -4.0, 2.0], np.float32)
    out.append(sk)
    return out


def test_exports_name_the_new_entry_points(api):
    for name in ("pt_temporal_defaults", "pt_temporal_accumulate", "pt_read_temporal", "pt_device_temporal", "pt_denoise_temporal",
                 "pt_debug_reproject"):
        assert name in api.EXPORTS
        assert hasattr(api.LIB, name)


def test_defaults(api):
    d = api.temporal_defaults()
    assert d["max_history"] == 64
    assert d["normal_cos"] == np.float32(0.9) and d["depth_tolerance"] == np.float32(0.02)


def test_reproject_matches_float64(api):
    rng = np.random.default_rng(11)
    cams = _cameras(api)
    compared = 0
    for ci, cur in enumerate(cams):
        for pi, prev in enumerate(cams):
            xs, ys = rng.integers(0, W, 40), rng.integers(0, H, 40)
            depth = rng.uniform(300.0, 3000.0, 40).astype(np.float32)
            xp, yp, dist, a = T.reproject(cur, prev, xs, ys, depth)
            for t in range(40):
                if abs(a[t]) < 1e-3:
                    continue                                            # on prev's eye plane: the sign of a is rounding
                if a[t] < 0:
                    with pytest.raises(api.PtError) as e:
                        api.debug_reproject(cur, prev, int(xs[t]), int(ys[t]), float(depth[t]))
                    assert e.value.code == api.PT_EINVAL
                    continue
                got = api.debug_reproject(cur, prev, int(xs[t]), int(ys[t]), float(depth[t]))
                assert abs(got[2] - dist[t]) <= 1e-5 * dist[t]
                if not (-W <= xp[t] <= 2 * W and -H <= yp[t] <= 2 * H):
                    continue                                            # far outside the frame: no tap is read there
                assert abs(got[0] - xp[t]) <= 1e-4 and abs(got[1] - yp[t]) <= 1e-4, (ci, pi, t, got, xp[t], yp[t])
                compared += 1
    assert compared > 400


def test_pixel_centre_lands_on_itself(api):
    for cam in _cameras(api):
        for depth in (50.0, 317.0, 1000.0, 4096.5, 25000.0, 1e5):
            for x, y in ((0, 0), (W - 1, H - 1), (W // 2, H // 3), (17, 71), (W - 5, 2)):
                got = api.debug_reproject(cam, cam, x, y, depth)
                assert abs(got[0] - x) <= 2.0 ** -10 and abs(got[1] - y) <= 2.0 ** -10, (depth, x, y, got)
                assert abs(got[2] - depth) <= 1e-5 * depth


def test_point_behind_gives_einval(api):
    cam = api.Camera(60.0, 0.0, 0.0, (0.0, 0.0, 0.0), W, H)
    ahead = cam["lookat"][0][:3] - cam["eye"][0][:3]
    shift = tuple(float(v) for v in ahead / np.linalg.norm(ahead) * 2000.0)      # 2000 units forward: the old hits are behind it
    prev = api.Camera(60.0, 0.0, 0.0, shift, W, H)
    with pytest.raises(api.PtError) as e:
        api.debug_reproject(cam, prev, W // 2, H // 2, 1000.0)
    assert e.value.code == api.PT_EINVAL
    out = (C.c_float * 3)()
    assert api.LIB.pt_debug_reproject(api._ptr(cam), api._ptr(prev), W // 2, H // 2, C.c_float(1000.0), out) == api.PT_EINVAL
    assert api.LIB.pt_debug_reproject(api._ptr(cam), api._ptr(cam), W, 0, C.c_float(1000.0), out) == api.PT_EINVAL   # x outside
    assert api.LIB.pt_debug_reproject(None, api._ptr(cam), 0, 0, C.c_float(1000.0), out) == api.PT_EINVAL


@pytest.mark.parametrize("kw", [
    {"max_history": -1}, {"normal_cos": 1.5}, {"normal_cos": -1.01}, {"normal_cos": float("nan")},
    {"depth_tolerance": -1e-6}, {"depth_tolerance": float("nan")},
])
def test_bad_parameters(api, cb_spec, kw):
    sc = api.Scene(16, 12, device=None).load(cb_spec)
    p = api.TemporalParams(**dict(api.temporal_defaults(), **kw))
    assert api.LIB.pt_temporal_accumulate(sc._h, C.byref(p)) == api.PT_EINVAL
    assert b"pt_temporal_accumulate" in api.LIB.pt_last_error(sc._h)
    sc.close()


def test_host_only_and_tiled(api, cb_spec):
    sc = api.Scene(16, 12, device=None).load(cb_spec)
    assert api.LIB.pt_temporal_accumulate(sc._h, None) == api.PT_EINVAL
    for extreme in ({"max_history": 0, "normal_cos": -1.0, "depth_tolerance": 0.0}, {"normal_cos": 1.0, "depth_tolerance": float("inf")}, {}):
        p = api.TemporalParams(**dict(api.temporal_defaults(), **extreme))
        assert api.LIB.pt_temporal_accumulate(sc._h, C.byref(p)) == api.PT_ENODEVICE
    with pytest.raises(api.PtError) as e:
        sc.temporal_accumulate()
    assert e.value.code == api.PT_ENODEVICE
    for call in (sc.read_temporal, sc.denoise_temporal):
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_ENODEVICE
    assert sc.device_temporal() is None
    dp = api.DenoiseVarianceParams(**dict(api.denoise_variance_defaults(), iterations=0))
    assert api.LIB.pt_denoise_temporal(sc._h, C.byref(dp)) == api.PT_EINVAL
    tiled = api.Scene(16, 16, device=None, rank=0, world=2).load(cb_spec)
    p = api.TemporalParams(**api.temporal_defaults())
    assert api.LIB.pt_temporal_accumulate(tiled._h, C.byref(p)) == api.PT_EINVAL
    assert b"world" in api.LIB.pt_last_error(tiled._h)
    dp = api.DenoiseVarianceParams(**api.denoise_variance_defaults())
    assert api.LIB.pt_denoise_temporal(tiled._h, C.byref(dp)) == api.PT_EINVAL
    assert api.LIB.pt_temporal_accumulate(None, C.byref(p)) == api.PT_EINVAL
    sc.close()
    tiled.close()


def test_model_still_camera_is_one_long_frame(api):
    """The model's own sanity: four frames of k samples through a camera at rest add up like one frame of 4k."""
    w, h = 12, 9
    cam = api.Camera(60.0, 0.0, 0.0, (0.0, 0.0, 0.0), w, h)
    rng = np.random.default_rng(4)
    nd = np.zeros((w * h, 4), np.float32)
    nd[:, 2] = -1.0
    nd[:, 3] = rng.uniform(800, 1500, w * h)
    nd[::7, 3] = -1.0
    alb = np.zeros((w * h, 4), np.float32)
    frames = [rng.random((w * h, 4)).astype(np.float32) for _ in range(4)]
    hist = None
    for f in frames:
        hist, info = T.accumulate(hist, cam, f, 4, alb, nd, w, h, max_history=64)
    want = np.mean([f[:, :3].astype(np.float64) for f in frames], axis=0)
    hit = nd[:, 3] >= 0
    assert np.allclose(hist.c[hit], want[hit], rtol=1e-12) and np.all(hist.n[hit] == 16) and np.all(hist.n[~hit] == 4)
    assert np.all(info["margin"][hit] > 1e-4) and not info["no_tap"][hit].any()
