"""-m "not gpu": the firefly filter without a device -- the pinned defaults and struct layout, the argument checks that come before
the device, the float64 model (tests/despeckle_ref.py) against hand-worked cases, and the authored frames of test_gpu_despeckle.py:
none of their decisions may be within 1e-3 of the other outcome."""
import ctypes as C

import numpy as np
import pytest

import despeckle_ref as D

NEW = ("pt_despeckle_defaults", "pt_despeckle", "pt_read_despeckled", "pt_device_despeckled", "pt_denoise_despeckled", "pt_debug_despeckle")


def test_exports_name_the_new_entry_points(api):
    for name in NEW:
        assert name in api.EXPORTS
        assert hasattr(api.LIB, name)


def test_defaults_and_layout(api):
    assert C.sizeof(api.DespeckleParams) == 28
    assert [(n, C.sizeof(t)) for n, t in api.DespeckleParams._fields_] == [
        ("source", 4), ("radius", 4), ("rank", 4), ("threshold", 4), ("floor", 4), ("min_rel_sigma", 4), ("spread", 4)]
    # through the ABI: the library writes seven 4-byte words in that order and nothing past them
    raw = (C.c_uint32 * 9)(*([0xDEADBEEF] * 9))
    api.LIB.pt_despeckle_defaults(C.byref(raw))
    words = np.frombuffer(raw, dtype=np.uint32)
    assert words[7] == 0xDEADBEEF and words[8] == 0xDEADBEEF
    d = api.despeckle_defaults()
    assert list(words[:3].view(np.int32)) == [d["source"], d["radius"], d["rank"]]
    assert list(words[3:6].view(np.float32)) == [d["threshold"], d["floor"], d["min_rel_sigma"]]
    assert int(words[6]) == d["spread"]
    assert d["source"] == api.PT_DESPECKLE_FRAME == 0 and api.PT_DESPECKLE_TEMPORAL == 1
    assert 1 <= d["radius"] <= 3 and 1 <= d["rank"] <= 3 and d["threshold"] >= 1 and d["floor"] >= 0 and d["min_rel_sigma"] >= 0
    assert d["spread"] == 1
    assert {k: d[k] for k in D.DEFAULTS} == D.DEFAULTS
    api.LIB.pt_despeckle_defaults(None)


BAD = [{"radius": 0}, {"radius": 4}, {"rank": 0}, {"rank": 4}, {"threshold": 0.99}, {"threshold": float("nan")},
       {"floor": -1e-6}, {"floor": float("nan")}, {"min_rel_sigma": -0.1}, {"min_rel_sigma": float("nan")},
       {"spread": 2}, {"spread": -1}]


@pytest.mark.parametrize("kw", BAD + [{"source": 2}, {"source": -1}])
def test_bad_parameters(api, cb_spec, kw):
    sc = api.Scene(16, 12, device=None).load(cb_spec)
    p = api.DespeckleParams(**dict(api.despeckle_defaults(), **kw))
    assert api.LIB.pt_despeckle(sc._h, C.byref(p)) == api.PT_EINVAL
    assert b"pt_despeckle" in api.LIB.pt_last_error(sc._h)
    sc.close()


@pytest.mark.parametrize("kw", BAD)
def test_debug_bad_parameters(api, cb_spec, kw):
    sc = api.Scene(16, 12, device=None).load(cb_spec)
    with pytest.raises(api.PtError) as e:
        sc.debug_despeckle(np.ones((4, 4, 4), np.float32), **kw)
    assert e.value.code == api.PT_EINVAL
    sc.close()


def test_host_only_and_tiled(api, cb_spec):
    sc = api.Scene(16, 12, device=None).load(cb_spec)
    assert api.LIB.pt_despeckle(sc._h, None) == api.PT_EINVAL
    assert api.LIB.pt_despeckle(None, None) == api.PT_EINVAL
    # valid arguments reach the device check: the order is arguments, world, device, then the source's rule
    for ok in ({}, {"source": 1}, {"radius": 1, "rank": 3, "threshold": 1.0, "floor": 0.0, "min_rel_sigma": 0.0, "spread": 0},
               {"radius": 3, "rank": 1, "threshold": float("inf"), "floor": float("inf"), "min_rel_sigma": float("inf")}):
        p = api.DespeckleParams(**dict(api.despeckle_defaults(), **ok))
        assert api.LIB.pt_despeckle(sc._h, C.byref(p)) == api.PT_ENODEVICE, ok
    for call in (sc.despeckle, sc.read_despeckled, sc.denoise_despeckled, lambda: sc.despeckle(source="temporal")):
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_ENODEVICE
    assert sc.device_despeckled() is None
    dp = api.DenoiseVarianceParams(**dict(api.denoise_variance_defaults(), iterations=0))
    assert api.LIB.pt_denoise_despeckled(sc._h, C.byref(dp)) == api.PT_EINVAL
    assert api.LIB.pt_denoise_despeckled(sc._h, None) == api.PT_EINVAL
    # the debug entry: arguments (source ignored), the frame's size and pointers, then the device
    frame = np.ones((3, 5, 4), np.float32)
    with pytest.raises(api.PtError) as e:
        sc.debug_despeckle(frame, source=7)
    assert e.value.code == api.PT_ENODEVICE
    out, flags = np.empty_like(frame), np.empty((3, 5), np.int32)
    p = api.DespeckleParams(**api.despeckle_defaults())
    for w, h in ((0, 3), (5, 0), (4097, 1), (1, 4097)):
        assert api.LIB.pt_debug_despeckle(sc._h, api._ptr(frame), w, h, C.byref(p), api._ptr(out), api._ptr(flags)) == api.PT_EINVAL
    assert api.LIB.pt_debug_despeckle(sc._h, None, 5, 3, C.byref(p), api._ptr(out), api._ptr(flags)) == api.PT_EINVAL
    assert api.LIB.pt_debug_despeckle(sc._h, api._ptr(frame), 5, 3, None, api._ptr(out), api._ptr(flags)) == api.PT_EINVAL
    assert api.LIB.pt_debug_despeckle(sc._h, api._ptr(frame), 5, 3, C.byref(p), api._ptr(out), api._ptr(flags)) == api.PT_ENODEVICE
    with pytest.raises(TypeError):
        sc.despeckle(sigma=1.0)
    tiled = api.Scene(16, 16, device=None, rank=0, world=2).load(cb_spec)
    assert api.LIB.pt_despeckle(tiled._h, C.byref(p)) == api.PT_EINVAL
    assert b"world" in api.LIB.pt_last_error(tiled._h)
    dp = api.DenoiseVarianceParams(**api.denoise_variance_defaults())
    assert api.LIB.pt_denoise_despeckled(tiled._h, C.byref(dp)) == api.PT_EINVAL
    sc.close()
    tiled.close()


# ---------------------------------------------------------------------------------------------------------- the model
def test_model_hand_worked_centre():
    """5 x 5 of 1.0 with a centre of 100, radius 1, rank 1, threshold 4: the centre goes to 4, and 96 / 9 goes to each of the nine
    pixels of its window (the centre included)."""
    f = np.ones((5, 5, 4), np.float32)
    f[..., 3] = np.inf
    f[2, 2, :3] = 100.0
    r = D.despeckle(f, radius=1, rank=1, threshold=4.0, floor=0.0, min_rel_sigma=0.5, spread=1)
    want = np.ones((5, 5))
    want[1:4, 1:4] += 96.0 / 9.0
    want[2, 2] = 4.0 + 96.0 / 9.0
    for k in range(3):
        assert np.allclose(r["c"][..., k], want, rtol=1e-7, atol=0)     # (the float32 luminance weights do not sum to 1 exactly)
    assert r["flags"].sum() == 1 and r["flags"][2, 2] == 1
    assert np.all(np.isinf(r["v"]))
    off = D.despeckle(f, radius=1, rank=1, threshold=4.0, spread=0)
    assert np.allclose(off["c"][2, 2], 4.0, rtol=1e-7) and np.array_equal(np.delete(off["c"].reshape(25, 3), 12, 0), np.ones((24, 3)))
    # a finite variance of relative sigma 1 passes the gate and is scaled by s^2; the shares add their squared luminance
    f[..., 3] = 0.0
    f[2, 2, 3] = 100.0 ** 2
    r = D.despeckle(f, radius=1, rank=1, threshold=4.0, spread=1)
    s = 4.0 / 100.0
    assert np.isclose(r["v"][2, 2], 1e4 * s * s + (96.0 / 9.0) ** 2, rtol=1e-6) and np.isclose(r["v"][1, 1], (96.0 / 9.0) ** 2, rtol=1e-6)
    assert r["v"][0, 0] == 0.0
    # ... and a converged highlight (relative sigma 0.1) is refused
    f[2, 2, 3] = 10.0 ** 2
    r = D.despeckle(f, radius=1, rank=1, threshold=4.0, spread=1)
    assert r["flags"].sum() == 0 and np.array_equal(r["c"], f[..., :3].astype(np.float64))
    assert r["margin_gate"][2, 2] > 0.9 and r["margin_T"][2, 2] > 0.9


def test_model_constant_frame_is_untouched():
    for value in (0.0, 0.37, 5.0):
        f = np.full((7, 9, 4), value, np.float32)
        for spread in (0, 1):
            r = D.despeckle(f, radius=2, rank=2, threshold=4.0, spread=spread)
            assert not r["flags"].any()
            assert np.array_equal(r["c"], f[..., :3].astype(np.float64)) and np.array_equal(r["v"], f[..., 3].astype(np.float64))


def test_model_rank_and_window_rules():
    name = {n: (f, p) for n, f, p in D.authored()}
    f, p = name["24x20 pair and triple, rank 1 spread 0"]
    by_rank = {k: D.despeckle(f, **dict(p, rank=k))["flags"] for k in (1, 2, 3)}
    pair, triple, single = [(4, 4), (4, 5)], [(12, 10), (12, 11), (13, 10)], (17, 20)
    assert by_rank[1][single] == 1 and not any(by_rank[1][q] for q in pair + triple)          # rank 1 misses the pair
    assert all(by_rank[2][q] == 1 for q in pair) and not any(by_rank[2][q] for q in triple)   # rank 2 catches it
    assert all(by_rank[3][q] == 1 for q in pair + triple)
    f, p = name["1x1: K = 0"]
    assert D.despeckle(f, **p)["flags"][0, 0] == 0
    f, p = name["14x12 not live, radius 1 spread 1"]
    r = D.despeckle(f, **p)
    assert [r["flags"][q] for q in ((5, 6), (4, 5), (6, 4), (1, 13))] == [2, 2, 2, 2] and r["flags"][5, 5] == 1 and r["flags"][0, 13] == 1
    assert not np.isnan(r["c"][r["live"]]).any() and not np.isnan(r["v"][r["live"]]).any()
    # the corner firefly at (0, 13) has three in-frame neighbours, one of them not live: its share is e / 3
    share = r["c"][0, 12] - f[0, 12, :3]
    clipped = r["c"][0, 13] - share                                    # c' of the firefly: it received its own share
    assert np.allclose(share * 3.0, f[0, 13, :3] - clipped, rtol=1e-9) and np.all(share > 1.0)
    f, p = name["12x8 black, spread 1"]
    r = D.despeckle(f, **p)
    assert np.isfinite(r["c"]).all() and r["v"][5, 9] == np.inf and np.isfinite(np.delete(r["v"].reshape(-1), 5 * 12 + 9)).all()


def test_model_keeps_the_sum():
    checked = 0
    for name, f, p in D.authored():
        if not p["spread"] or not np.isfinite(f[..., :3]).all():
            continue
        r = D.despeckle(f, **p)
        before, after = f[..., :3].astype(np.float64).sum(axis=(0, 1)), r["c"].sum(axis=(0, 1))
        assert np.all(np.abs(after - before) <= 1e-12 * np.abs(before)), (name, before, after)
        checked += 1
    assert checked >= 15


def test_replay_with_the_models_flags_is_the_model():
    for name, f, p in D.authored():
        r = D.despeckle(f, **p)
        again = D.replay(f, r["flags"], **p)
        assert np.array_equal(again["c"], r["c"], equal_nan=True) and np.array_equal(again["v"], r["v"], equal_nan=True), name
        ratio, at = D.check_values(np.concatenate([r["c"], r["v"][..., None]], axis=-1).astype(np.float32), r)
        assert ratio <= 1.0, (name, ratio, at)          # rounding the model to float32 stays inside the GPU test's tolerance


def test_authored_inputs_have_clear_margins():
    cases = D.authored()
    names = [n for n, _, _ in cases]
    assert len(set(names)) == len(names) and D.LARGEST in names
    seen = {"flagged": 0, "gate_refused": 0, "not_live": 0, "inf_v": 0}
    for name, f, p in cases:
        r = D.despeckle(f, **p)
        assert r["margin"].min() >= 1e-3, (name, float(r["margin"].min()))
        seen["flagged"] += int((r["flags"] == 1).sum())
        seen["not_live"] += int((r["flags"] == 2).sum())
        seen["gate_refused"] += int((r["above"] & (r["flags"] == 0)).sum())
        seen["inf_v"] += int(((r["flags"] == 1) & np.isinf(f[..., 3])).sum())
    assert all(v > 0 for v in seen.values()), seen
    assert {p["radius"] for _, _, p in cases} == {1, 2, 3} and {p["rank"] for _, _, p in cases} == {1, 2, 3}
    assert {p["spread"] for _, _, p in cases} == {0, 1} and any(p["min_rel_sigma"] == 0.0 for _, _, p in cases)
    assert {f.shape[:2] for _, f, _ in cases} >= {(1, 1), (3, 2), (16, 16), (19, 17), (5, 33), (40, 48)}
