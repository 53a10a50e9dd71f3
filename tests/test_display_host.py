"""-m "not gpu": the display stage without a device -- the pinned defaults and struct layout, every argument check in the pinned order
and before the device, the header's table, and the float64 model's own invariants (tests/display_ref.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import display_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pt_display_defaults", "pt_display", "pt_read_display", "pt_device_display", "pt_display_info", "pt_debug_display_histogram",
       "pt_display_reset", "pt_write_display_ppm", "pt_debug_display")
INF, NAN = float("inf"), float("nan")


def test_exports_name_the_new_entry_points(api):
    for name in NEW:
        assert name in api.EXPORTS
        assert hasattr(api.LIB, name)


def test_defaults_and_layout(api):
    assert C.sizeof(api.DisplayParams) == 60 and C.sizeof(api.DisplayInfo) == 24
    assert [n for n, _ in api.DisplayParams._fields_] == [
        "source", "metering", "ev", "key", "low_permille", "high_permille", "min_ev", "max_ev", "adapt", "bloom_levels", "bloom_threshold",
        "bloom_intensity", "curve", "white", "encoding"]
    raw = (C.c_uint32 * 17)(*([0xDEADBEEF] * 17))
    api.LIB.pt_display_defaults(C.byref(raw))
    words = np.frombuffer(raw, dtype=np.uint32)
    assert words[15] == 0xDEADBEEF and words[16] == 0xDEADBEEF and not (words[:15] == 0xDEADBEEF).any()
    d = api.display_defaults()
    assert d == D.DEFAULTS
    assert d == dict(source=api.PT_DISPLAY_FRAME, metering=api.PT_METER_AUTO, ev=0.0, key=np.float32(0.18), low_permille=100, high_permille=950,
                     min_ev=-16.0, max_ev=16.0, adapt=1.0, bloom_levels=4, bloom_threshold=1.0, bloom_intensity=0.0, curve=api.PT_CURVE_ACES,
                     white=INF, encoding=api.PT_ENCODE_SRGB)
    assert (api.PT_DISPLAY_FRAME, api.PT_DISPLAY_DENOISED, api.PT_DISPLAY_TEMPORAL, api.PT_DISPLAY_DESPECKLED) == (0, 1, 2, 3)
    assert (api.PT_METER_MANUAL, api.PT_METER_AUTO, api.PT_CURVE_LINEAR, api.PT_CURVE_REINHARD, api.PT_CURVE_ACES) == (0, 1, 0, 1, 2)
    assert (api.PT_ENCODE_SRGB, api.PT_ENCODE_LINEAR) == (0, 1)
    api.LIB.pt_display_defaults(None)


# every refusal in the pinned order: (what is wrong, a word of its message)
ORDER = [({"source": 4}, b"source"), ({"metering": 2}, b"metering"), ({"curve": 3}, b"curve"), ({"encoding": -1}, b"encoding"),
         ({"ev": NAN}, b"NaN"), ({"key": 0.0}, b"key"), ({"low_permille": 950, "high_permille": 950}, b"permille"),
         ({"min_ev": 1.0, "max_ev": 0.0}, b"min_ev"), ({"adapt": 0.0}, b"adapt"), ({"bloom_levels": 7}, b"bloom_levels"),
         ({"bloom_threshold": -1.0}, b"bloom_threshold"), ({"bloom_intensity": -0.5}, b"bloom_intensity"), ({"white": 0.0}, b"white")]
BAD = [kw for kw, _ in ORDER] + [{"source": -1}, {"metering": -1}, {"curve": -1}, {"encoding": 2}, {"key": NAN}, {"key": -1.0}, {"min_ev": NAN},
                                 {"max_ev": NAN}, {"adapt": NAN}, {"adapt": 1.5}, {"adapt": -0.1}, {"bloom_threshold": NAN}, {"bloom_intensity": NAN},
                                 {"white": NAN}, {"white": -2.0}, {"low_permille": -1}, {"high_permille": 1001}, {"low_permille": 960},
                                 {"bloom_levels": 0}]


@pytest.mark.parametrize("kw", BAD, ids=[repr(k) for k in BAD])
def test_bad_parameters(api, cb_spec, kw):
    sc = api.Scene(16, 12, device=None).load(cb_spec)
    p = api.DisplayParams(**dict(api.display_defaults(), **kw))
    assert api.LIB.pt_display(sc._h, C.byref(p)) == api.PT_EINVAL
    assert b"pt_display" in api.LIB.pt_last_error(sc._h)
    if "source" not in kw:
        with pytest.raises(api.PtError) as e:
            sc.debug_display(np.ones((4, 4, 4), np.float32), **kw)
        assert e.value.code == api.PT_EINVAL
    sc.close()


def test_refusals_come_in_the_pinned_order(api, cb_spec):
    tiled = api.Scene(16, 16, device=None, rank=0, world=2).load(cb_spec)
    for first in range(len(ORDER)):
        kw = {}
        for more, _ in reversed(ORDER[first:]):             # everything from `first` on is wrong at once
            kw.update(more)
        p = api.DisplayParams(**dict(api.display_defaults(), **kw))
        assert api.LIB.pt_display(tiled._h, C.byref(p)) == api.PT_EINVAL
        msg = api.LIB.pt_last_error(tiled._h)
        assert ORDER[first][1] in msg, (first, msg)
        for _, later in ORDER[first + 1:]:
            assert later not in msg, (first, msg)
    p = api.DisplayParams(**api.display_defaults())
    assert api.LIB.pt_display(tiled._h, C.byref(p)) == api.PT_EINVAL and b"world" in api.LIB.pt_last_error(tiled._h)     # world comes last
    assert api.LIB.pt_display(tiled._h, None) == api.PT_EINVAL and b"NULL" in api.LIB.pt_last_error(tiled._h)
    tiled.close()


def test_host_only(api, cb_spec, tmp_path):
    sc = api.Scene(16, 12, device=None).load(cb_spec)
    assert api.LIB.pt_display(sc._h, None) == api.PT_EINVAL
    assert api.LIB.pt_display(None, None) == api.PT_EINVAL
    # valid arguments reach the device check, which comes before the source's own rule
    for ok in ({}, {"source": 1}, {"source": 2}, {"source": 3}, {"metering": 0, "ev": -INF}, {"min_ev": -INF, "max_ev": INF, "white": 1e-3},
               {"low_permille": 0, "high_permille": 1000, "adapt": 1e-3, "bloom_levels": 6, "bloom_threshold": 0.0, "bloom_intensity": INF}):
        p = api.DisplayParams(**dict(api.display_defaults(), **ok))
        assert api.LIB.pt_display(sc._h, C.byref(p)) == api.PT_ENODEVICE, ok
    for call in (sc.display, sc.read_display, sc.display_info, sc.display_histogram, lambda: sc.write_display_ppm(str(tmp_path / "x.ppm")),
                 lambda: sc.display(source="despeckled", curve="reinhard", encoding="linear", metering="manual")):
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_ENODEVICE
    assert sc.device_display() is None
    sc.display_reset()
    assert api.LIB.pt_display_reset(None) == api.PT_EINVAL
    frame = np.ones((3, 5, 4), np.float32)
    with pytest.raises(api.PtError) as e:
        sc.debug_display(frame, source=7)                    # (source is ignored)
    assert e.value.code == api.PT_ENODEVICE
    p = api.DisplayParams(**api.display_defaults())
    args = lambda f, w, h, pp, prev=0.0: (sc._h, f, w, h, pp, prev, None, None, None, None)
    for w, h in ((0, 3), (5, 0), (4097, 1), (1, 4097)):
        assert api.LIB.pt_debug_display(*args(api._ptr(frame), w, h, C.byref(p))) == api.PT_EINVAL
    assert api.LIB.pt_debug_display(*args(None, 5, 3, C.byref(p))) == api.PT_EINVAL
    assert api.LIB.pt_debug_display(*args(api._ptr(frame), 5, 3, None)) == api.PT_EINVAL
    assert api.LIB.pt_debug_display(*args(api._ptr(frame), 5, 3, C.byref(p), NAN)) == api.PT_EINVAL
    assert api.LIB.pt_debug_display(*args(api._ptr(frame), 5, 3, C.byref(p))) == api.PT_ENODEVICE
    with pytest.raises(TypeError):
        sc.display(gamma=2.2)
    sc.close()


def test_header_table_is_log2_of_the_bin_centres():
    text = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    m = re.search(r"#define\s+PT_DISPLAY_LOG2_TABLE\s*\{([^}]*)\}", text)
    lits = [s.strip() for s in m.group(1).split(",")]
    assert len(lits) == 8 and all(s.endswith("f") for s in lits)
    got = np.array([np.float32(float(s[:-1])) for s in lits])
    want = np.float32(np.log2(1.0 + (np.arange(8) + 0.5) / 8.0))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(D.T.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------- the model's own invariants
def test_fma32_rounds_once():
    """the model's float32 fmaf against exact rational arithmetic"""
    from fractions import Fraction
    rng = np.random.RandomState(1)
    a = (rng.standard_normal(4000) * 2.0 ** rng.randint(-20, 20, 4000)).astype(np.float32)
    b = (rng.standard_normal(4000) * 2.0 ** rng.randint(-20, 20, 4000)).astype(np.float32)
    c = (-(a.astype(np.float64) * b) * (1 + rng.randint(-3, 4, 4000) * 2.0 ** -24)).astype(np.float32)      # heavy cancellation
    got = D.fma32(a, b, c)
    for i in range(0, 4000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        err = abs(Fraction(float(got[i])) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), i


def test_bit_indexed_bin_is_eight_bins_per_stop():
    """The bin from the bits is the stop, floor(log2 l), times eight plus the eighth of the mantissa, floor(8 (l / 2^stop - 1)): the edges
    inside a stop are linear in l (2^e (1 + j / 8), which T's centres log2(1 + (j + 0.5) / 8) go with), not logarithmic.  So it equals
    floor(8 log2 l) + 128 at stop granularity and at every power of two, and is at most one bin below it elsewhere (8 log2(1 + m) - 8 m
    lies in [0, 0.69)); `floor(8 log2 l) + 128` itself is not what the pinned bit rule computes."""
    rng = np.random.RandomState(2)
    l = np.concatenate([(2.0 ** rng.uniform(-16, 16, 20000)).astype(np.float32), np.float32(2.0) ** np.arange(-16, 16), D.lum32(D.ramp(64, 64)[..., :3]).ravel()])
    l = l[(l >= np.float32(2.0 ** -16)) & (l < np.float32(2.0 ** 16))]
    x = l.astype(np.float64)
    stop = np.floor(np.log2(x))
    m8 = 8.0 * (x / 2.0 ** stop - 1.0)                                       # exact: a power-of-two scaling and a difference of neighbours
    off_edge = np.abs(m8 - np.round(m8)) > 8.0 * 2.0 ** -22                  # farther than an ulp from an edge
    assert off_edge.mean() > 0.99
    b = D.bins_of(l)
    assert np.array_equal(b[off_edge], (8 * stop + np.floor(m8) + 128).astype(np.int64)[off_edge])
    assert np.array_equal(b >> 3, (stop + 16).astype(np.int64))
    logb = (np.floor(8.0 * np.log2(x)) + 128).astype(np.int64)
    assert np.all((logb - b >= 0) & (logb - b <= 1))
    assert np.array_equal(D.bins_of(np.float32(2.0) ** np.arange(-16, 16)), 8 * np.arange(32))
    assert D.bins_of(np.float32([2.0 ** 16, 1e30, 3e38])).tolist() == [255, 255, 255]
    assert D.bins_of(np.float32([np.nextafter(np.float32(2.0 ** 16), np.float32(0))])).tolist() == [255]
    # T: the centre of each eighth, as log2
    assert np.allclose(D.T, np.log2(1 + (np.arange(8) + 0.5) / 8), rtol=0, atol=2.0 ** -24)


def test_metering_by_hand():
    """four pixels, one per stop: 2^-2, 2^-1, 1, 2 -> bins 112, 120, 128, 136; permille 250 / 750 keeps the middle two"""
    f = np.zeros((1, 4, 4), np.float32)
    for i, v in enumerate((0.25, 0.5, 1.0, 2.0)):
        f[0, i, :3] = v / float(D.lum32(np.ones(3, np.float32)))            # luminance v up to rounding inside the bin
    r = D.meter(f, dict(D.DEFAULTS, low_permille=250, high_permille=750))
    assert np.flatnonzero(r["hist"]).tolist() == [112, 120, 128, 136] and r["K"] == 2 and r["n_dark"] == 0 and r["n_nonfinite"] == 0
    lam = lambda b: float(np.float32((b >> 3) - 16) + D.T[b & 7])
    assert r["M"] == pytest.approx((lam(120) + lam(128)) / 2, abs=1e-12)
    assert r["E"] == pytest.approx(float(np.float32(0.18)) * 2.0 ** -r["M"], rel=1e-12)
    r = D.meter(f, dict(D.DEFAULTS, low_permille=250, high_permille=750, min_ev=-1.0, max_ev=-1.0))
    assert r["E"] == 0.5
    r = D.meter(f, dict(D.DEFAULTS, adapt=0.25), prev_exposure=4.0)
    e1 = D.meter(f, D.DEFAULTS)["E"]
    assert r["E"] == pytest.approx(4.0 ** 0.75 * e1 ** 0.25, rel=1e-12)
    assert D.meter(f, dict(D.DEFAULTS, metering=D.MANUAL, ev=3.0), prev_exposure=4.0)["E"] == 8.0
    black = D.meter(np.zeros((2, 2, 4), np.float32), dict(D.DEFAULTS, ev=2.0))
    assert black["K"] == 0 and black["n_dark"] == 4 and black["E"] == 4.0


def test_reinhard_of_black_is_black():
    for white in (INF, 2.0):
        for enc in (D.SRGB, D.ENC_LINEAR):
            r = D.display(np.zeros((2, 3, 4), np.float32), curve=D.REINHARD, white=white, encoding=enc)
            assert np.array_equal(r["v"], np.zeros((2, 3, 3))) and not r["rgb8"].any()
    one = D.tone(np.full((1, 3), 3.0), dict(D.DEFAULTS, curve=D.REINHARD, white=INF, encoding=D.ENC_LINEAR))
    assert one == pytest.approx(3.0 / (1.0 + D.lum64(np.full((1, 3), 3.0))[0]))


@pytest.mark.parametrize("levels", [1, 2])
def test_bloom_closed_form_for_the_interior_impulse(levels):
    """every step's weights sum to 1 and the footprint stays off the border, so sum(out - h) = intensity sum(B)"""
    frame = dict(D.authored())[D.IMPULSE]
    r = D.display(frame, metering=D.MANUAL, ev=0.0, bloom_levels=levels, **D.BLOOM)
    assert not r["touches_border"]
    add = (r["out"] - r["h"]).sum(axis=(0, 1))
    want = D.BLOOM["bloom_intensity"] * r["B"].sum(axis=(0, 1))
    assert np.all(want > 0) and np.all(np.abs(add - want) <= 1e-12 * want)
    assert D.display(frame, metering=D.MANUAL, ev=0.0, bloom_levels=6, **D.BLOOM)["touches_border"]


def test_pyramid_weights_sum_to_one_and_clamp():
    ones = np.ones((9, 17, 3))
    assert np.allclose(D.down(ones), 1.0, rtol=0, atol=1e-15) and D.down(ones).shape == (5, 9, 3)
    assert np.allclose(D.up(D.down(ones), 17, 9), 1.0, rtol=0, atol=1e-15)
    assert D.level_sizes(64, 64, 6)[-1] == (1, 1) and D.level_sizes(17, 9, 6) == [(17, 9), (9, 5), (5, 3), (3, 2), (2, 1), (1, 1), (1, 1)]
    d = np.zeros((1, 4, 3))
    d[0, 0] = 8.0
    # x = 0 reads clamp(-1), 0, 1, 2 = two copies of the corner: (1 + 3) / 8; y the same four times: 1
    assert D.down(d)[0, 0, 0] == pytest.approx(8.0 * 0.5) and D.down(d)[0, 1, 0] == 0.0
    d[0, 0], d[0, 1] = 0.0, 8.0
    # source 1 is tap 2 of x = 0 (3 / 8) and tap 0 of x = 1 (1 / 8)
    assert D.down(d)[0, 0, 0] == pytest.approx(3.0) and D.down(d)[0, 1, 0] == pytest.approx(1.0)
    u = D.up(np.arange(3.0).reshape(1, 3, 1).repeat(3, axis=2), 6, 1)[0, :, 0]
    assert u.tolist() == [0.0, 0.25, 0.75, 1.25, 1.75, 2.0]


def test_bytes_of_the_authored_frames_are_decidable():
    """a condition on the inputs: per frame, over every configuration, at least 99 % of the model's bytes lie farther from k + 0.5 than
    255 x the float tolerance"""
    assert [f.shape[:2] for _, f in D.authored()].count((64, 64)) >= 2
    assert {f.shape[:2] for _, f in D.authored()} == {(1, 1), (2, 3), (9, 17), (31, 33), (64, 64)}
    for name, frame in D.authored():
        share = []
        for cname, p in D.configs():
            r = D.display(frame, **p)
            assert not np.isnan(r["v"]).any() and not np.isnan(r["tol"]).any(), (name, cname)
            assert np.all(r["v"] >= 0) and np.all(r["v"] <= 1)
            share.append(r["decidable"].mean())
        print("[display] %-36s decidable bytes: mean %.4f, worst configuration %.4f" % (name, np.mean(share), min(share)))
        assert np.mean(share) >= 0.99, name
