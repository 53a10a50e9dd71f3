"""-m "not gpu": adaptive frames (pt_render_adaptive) without a device -- the round boundaries, argument checking on a host-only
context, and the float32 noise estimate the GPU tests replay (tests/adaptive_ref.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import adaptive_ref as R


@pytest.mark.parametrize("lo,hi,want", [
    (2, 2, [1, 2]),
    (4, 64, [2, 4, 8, 16, 32, 64]),
    (16, 1024, [8, 16, 32, 64, 128, 256, 512, 1024]),
    (16, 1000, [8, 16, 32, 64, 128, 256, 512, 1000]),      # the last round is capped at max_spp
    (6, 100, [3, 6, 12, 24, 48, 96, 100]),
])
def test_rounds(api, lo, hi, want):
    assert api.adaptive_rounds(lo, hi) == want
    assert R.rounds(lo, hi) == want


def test_rounds_count_and_cap(api):
    n = C.c_int32()
    out = (C.c_int32 * 3)(-1, -1, -1)
    assert api.LIB.pt_adaptive_rounds(4, 64, C.cast(out, C.c_void_p), 2, C.byref(n)) == api.PT_OK
    assert n.value == 6 and list(out) == [2, 4, -1]
    assert api.LIB.pt_adaptive_rounds(4, 64, None, 0, C.byref(n)) == api.PT_OK and n.value == 6
    assert api.LIB.pt_adaptive_rounds(4, 64, None, 2, C.byref(n)) == api.PT_EINVAL
    assert api.LIB.pt_adaptive_rounds(4, 64, None, 0, None) == api.PT_EINVAL


@pytest.mark.parametrize("lo,hi", [(0, 4), (1, 4), (3, 8), (-2, 4), (8, 4), (2, 0)])
def test_rounds_bad_arguments(api, lo, hi):
    n = C.c_int32()
    assert api.LIB.pt_adaptive_rounds(lo, hi, None, 0, C.byref(n)) == api.PT_EINVAL
    with pytest.raises(api.PtError):
        api.adaptive_rounds(lo, hi)


@pytest.mark.parametrize("lo,hi,thr,it", [
    (0, 4, 0.1, 4), (1, 4, 0.1, 4), (5, 16, 0.1, 4), (8, 4, 0.1, 4), (-2, 4, 0.1, 4),
    (4, 16, -1.0, 4), (4, 16, float("nan"), 4), (4, 16, -float("inf"), 4), (4, 16, 0.1, -1),
])
def test_invalid_arguments_host_only(api, cb_spec, lo, hi, thr, it):
    sc = api.Scene(16, 16, device=None).load(cb_spec)
    rc = api.LIB.pt_render_adaptive(sc._h, api._ptr(sc.camera), it, lo, hi, thr)
    assert rc == api.PT_EINVAL
    assert b"pt_render_adaptive" in api.LIB.pt_last_error(sc._h)
    sc.close()


@pytest.mark.parametrize("thr", [0.0, 0.5, float("inf")])
def test_valid_arguments_host_only_need_a_device(api, cb_spec, thr):
    sc = api.Scene(16, 16, device=None).load(cb_spec)
    with pytest.raises(api.PtError) as e:
        sc.render_adaptive(4, 16, thr)
    assert e.value.code == api.PT_ENODEVICE
    for call in (sc.sample_counts, sc.tile_state):
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_ENODEVICE
    sc.close()


def test_estimate_zeros():
    z = np.zeros((5, 4), np.float32)
    e = R.pixel_estimate(z, z)
    assert e.dtype == np.float32 and np.all(e == 0)
    assert np.all(R.tile_errors(np.zeros((64, 4), np.float32), np.zeros((64, 4), np.float32), 8, 8) == 0)


def test_estimate_formula_in_float32():
    M = np.array([[0.5, 0.25, 0.125, 0.0]], np.float32)
    A = np.array([[0.25, 0.5, 0.0, 0.0]], np.float32)
    f = np.float32
    d = (abs(f(0.5) - f(0.25)) + abs(f(0.25) - f(0.5))) + abs(f(0.125) - f(0.0))
    s = (f(0.5) + f(0.25)) + f(0.125)
    want = f(d / (f(1e-4) + np.sqrt(s)))
    assert R.pixel_estimate(M, A)[0].view(np.uint32) == np.float32(want).view(np.uint32)
    assert abs(float(want) - 0.625 / (1e-4 + math.sqrt(0.875))) < 1e-6


def test_estimate_nan_and_negative_give_inf():
    M = np.zeros((64, 4), np.float32)
    A = np.zeros((64, 4), np.float32)
    M[10, 1] = np.nan
    assert np.isposinf(R.tile_errors(M, A, 8, 8)[0])
    M[10, 1] = 0.0
    M[3, 0] = -1.0                               # sqrt of a negative sum: NaN -> +inf
    assert np.isposinf(R.pixel_estimate(M, A)[3])
    M[3, 0] = np.inf
    assert np.isposinf(R.tile_errors(M, A, 8, 8)[0])


def test_ragged_frame_ignores_lanes_outside():
    W, H = 10, 9                                 # tiles 2 x 2; the right and bottom tiles are partial
    M = np.full((H * W, 4), 1.0, np.float32)
    A = np.full((H * W, 4), 1.0, np.float32)
    M[(8 * W) + 9, 0] = 2.0                      # pixel (9, 8): tile 3, the only pixel of it inside the frame
    e = R.tile_errors(M, A, W, H)
    assert e.shape == (4,)
    assert e[0] == 0 and e[1] == 0 and e[2] == 0 and e[3] > 0
    assert e[3] == R.pixel_estimate(M[(8 * W) + 9], A[(8 * W) + 9])


def test_replay_decisions():
    """Two boundaries worth of hand-made snapshots: a tile whose mean moved stays, the others retire."""
    W = H = 16
    n = W * H
    snaps = {}
    base = np.full((n, 4), 0.25, np.float32)
    rn = np.arange(n, dtype=np.int32)
    for b in (1, 2, 4, 8):
        c = base.copy()
        if b >= 2:
            c[:8, 0] = 0.25 + 0.5 / b           # row 0 of tile 0 keeps changing
        snaps[b] = (c, rn + b)
    out = R.replay(snaps, W, H, 2, 8, 0.01)
    assert out["rounds"] == [1, 2, 4, 8] and out["active_tiles"] == [4, 4, 1, 1]
    assert out["spp"].tolist() == [8, 2, 2, 2]
    assert np.isinf(out["err"][1]) == False and out["err"][1] == 0       # noqa: E712
    assert out["err"][0] > 0.01
    assert np.array_equal(out["rnds"][:8], rn[:8] + 8) and np.array_equal(out["rnds"][8:16], rn[8:16] + 2)


@pytest.mark.parametrize("W,H,hi,ok", [
    (64, 64, 1 << 26, False),       # longest round 2^25 samples x 64 tiles: past the 31-bit work-item counter
    (64, 64, 1 << 24, True),
    (1920, 1080, 1 << 18, False),   # 2^17 x 32,400 tiles
    (1920, 1080, 1 << 15, True),
])
def test_max_spp_fits_the_work_item_counter(api, W, H, hi, ok):
    """Checked before anything renders, on a host-only context too: a valid call then fails only for want of a device."""
    sc = api.Scene(W, H, device=None)
    rc = api.LIB.pt_render_adaptive(sc._h, api._ptr(sc.camera), 4, 2, hi, 0.5)
    if ok:
        assert rc == api.PT_ENODEVICE
    else:
        assert rc == api.PT_EINVAL and b"max_spp too large" in api.LIB.pt_last_error(sc._h)
    sc.close()
