"""-m "not gpu": every entry point of the post-process chain on host-only contexts -- which check fails first, with which return code
and with exactly which pt_last_error text.  The functions do not agree on the order (pt_denoise asks for guides before it asks for a
device, pt_temporal_accumulate the other way round), and callers match on these texts: whichever check fails first must keep failing
first, with the same words.  Per entry point: one call per class of invalid parameter, a call with valid parameters, and a call on a
context of a two-rank frame (world = 2)."""
import ctypes as C

import numpy as np
import pytest

NAN, INF = float("nan"), float("inf")
NODEV = "context was created without a HIP device (host-only); no CPU render path exists"
NPIX_TEXT = "npix must equal the local pixel count"
W, H = 16, 12


def world_text(who):
    return who + ": contexts of one rank (world == 1) only"


def guides_text(who):
    return who + ": no guides (pt_render_aovs has not run since the scene was last uploaded)"


@pytest.fixture(scope="module")
def one(api, cb_spec):
    sc = api.Scene(W, H, device=None).load(cb_spec)
    yield sc
    sc.close()


@pytest.fixture(scope="module")
def tiled(api, cb_spec):
    sc = api.Scene(W, 16, device=None, rank=0, world=2).load(cb_spec)
    yield sc
    sc.close()


def refused(api, sc, rc, code, text):
    assert rc == code, (rc, api.LIB.pt_last_error(sc._h))
    assert api.LIB.pt_last_error(sc._h).decode() == text


def einval(api, sc, rc, text):
    refused(api, sc, rc, api.PT_EINVAL, text)


def nodevice(api, sc, rc):
    refused(api, sc, rc, api.PT_ENODEVICE, NODEV)


# ---------------------------------------------------------------------------------------------------------------- guide buffers
def test_render_aovs(api, one, tiled):
    f = api.LIB.pt_render_aovs
    cam = api._ptr(one.camera)
    assert f(None, cam, 1, 4) == api.PT_EINVAL
    for sub in (0, 9, -1):
        einval(api, one, f(one._h, cam, sub, 4), "pt_render_aovs: subpixels must be 1..8")
    for depth in (-1, 17):
        einval(api, one, f(one._h, cam, 1, depth), "pt_render_aovs: specular_depth must be 0..16")
    einval(api, one, f(one._h, cam, 0, 17), "pt_render_aovs: subpixels must be 1..8")            # subpixels first
    einval(api, one, f(one._h, None, 1, -1), "pt_render_aovs: specular_depth must be 0..16")       # the arguments before the camera
    for sub, depth in ((1, 0), (8, 16), (1, 4)):
        nodevice(api, one, f(one._h, cam, sub, depth))                                             # the device before the camera
    nodevice(api, one, f(one._h, None, 1, 4))
    nodevice(api, tiled, f(tiled._h, api._ptr(tiled.camera), 1, 4))                                # any number of ranks
    einval(api, tiled, f(tiled._h, api._ptr(tiled.camera), 9, 4), "pt_render_aovs: subpixels must be 1..8")


def test_render_aovs_ex(api, one, tiled):
    f = api.LIB.pt_render_aovs_ex
    cam = api._ptr(one.camera)
    P = lambda sub=1, depth=4, shading=api.PT_AOV_SHADED: C.byref(api.AovParams(sub, depth, shading))
    assert f(None, cam, P()) == api.PT_EINVAL
    einval(api, one, f(one._h, cam, None), "pt_render_aovs_ex: params is NULL")
    for shading in (api.PT_AOV_GEOMETRIC, api.PT_AOV_SHADED, 7):                                   # (its own prefix for either shading)
        for sub in (0, 9):
            einval(api, one, f(one._h, cam, P(sub, 4, shading)), "pt_render_aovs_ex: subpixels must be 1..8")
        for depth in (-1, 17):
            einval(api, one, f(one._h, cam, P(1, depth, shading)), "pt_render_aovs_ex: specular_depth must be 0..16")
    for shading in (-1, 2):
        einval(api, one, f(one._h, cam, P(1, 4, shading)), "pt_render_aovs_ex: shading must be PT_AOV_GEOMETRIC or PT_AOV_SHADED")
    einval(api, one, f(one._h, cam, P(0, 17, 2)), "pt_render_aovs_ex: subpixels must be 1..8")
    einval(api, one, f(one._h, cam, P(1, 17, 2)), "pt_render_aovs_ex: specular_depth must be 0..16")
    for shading in (api.PT_AOV_GEOMETRIC, api.PT_AOV_SHADED):
        for sub, depth in ((1, 0), (8, 16)):
            nodevice(api, one, f(one._h, cam, P(sub, depth, shading)))
        nodevice(api, one, f(one._h, None, P(1, 4, shading)))                                      # the device before the camera
        nodevice(api, tiled, f(tiled._h, api._ptr(tiled.camera), P(1, 4, shading)))
    einval(api, tiled, f(tiled._h, api._ptr(tiled.camera), P(1, 4, 2)), "pt_render_aovs_ex: shading must be PT_AOV_GEOMETRIC or PT_AOV_SHADED")


def test_read_aovs(api, one, tiled):
    f = api.LIB.pt_read_aovs
    buf = np.zeros((W * H, 4), np.float32)
    assert f(None, api._ptr(buf), api._ptr(buf), W * H) == api.PT_EINVAL
    nodevice(api, one, f(one._h, api._ptr(buf), api._ptr(buf), W * H))
    nodevice(api, one, f(one._h, api._ptr(buf), api._ptr(buf), 5))                                # the device before npix
    nodevice(api, one, f(one._h, None, None, W * H))
    nodevice(api, tiled, f(tiled._h, api._ptr(buf), api._ptr(buf), tiled.local_pixels))


# ---------------------------------------------------------------------------------------------------------------- a-trous filter
def test_denoise(api, one, tiled):
    f = api.LIB.pt_denoise
    P = lambda **kw: C.byref(api.DenoiseParams(**dict(api.denoise_defaults(), **kw)))
    assert f(None, P()) == api.PT_EINVAL
    einval(api, one, f(one._h, None), "pt_denoise: params is NULL")
    for it in (0, 11, -3):
        einval(api, one, f(one._h, P(iterations=it)), "pt_denoise: iterations must be 1..10")
    for kw in ({"sigma_color": -1.0}, {"sigma_normal": -0.5}, {"sigma_depth": -1e-3}, {"sigma_color": NAN}, {"sigma_normal": NAN}, {"sigma_depth": NAN}):
        einval(api, one, f(one._h, P(**kw)), "pt_denoise: sigmas must be >= 0 (and not NaN)")
    einval(api, one, f(one._h, P(iterations=0, sigma_color=NAN)), "pt_denoise: iterations must be 1..10")
    # valid parameters: the guides are asked for before the device
    for kw in ({}, {"iterations": 1}, {"iterations": 10, "sigma_color": INF, "sigma_normal": 0.0, "sigma_depth": INF, "demodulate": 0}):
        einval(api, one, f(one._h, P(**kw)), guides_text("pt_denoise"))
    # world = 2: after the parameters, before the guides
    einval(api, tiled, f(tiled._h, None), "pt_denoise: params is NULL")
    einval(api, tiled, f(tiled._h, P(iterations=0)), "pt_denoise: iterations must be 1..10")
    einval(api, tiled, f(tiled._h, P(sigma_depth=NAN)), "pt_denoise: sigmas must be >= 0 (and not NaN)")
    einval(api, tiled, f(tiled._h, P()), world_text("pt_denoise"))


# ---------------------------------------------------------------------------------------------------------------- variance
def test_read_variance(api, one, tiled):
    f = api.LIB.pt_read_variance
    buf = np.zeros(W * H, np.float32)
    assert f(None, api._ptr(buf), W * H) == api.PT_EINVAL
    nodevice(api, one, f(one._h, api._ptr(buf), W * H))
    nodevice(api, one, f(one._h, None, W * H))                                                     # the device before the arguments
    nodevice(api, one, f(one._h, api._ptr(buf), 5))
    nodevice(api, tiled, f(tiled._h, api._ptr(buf), tiled.local_pixels))


VARIANCE_BAD = [(None, "params is NULL"), ({"iterations": 0}, "iterations must be 1..10"), ({"iterations": 11}, "iterations must be 1..10"),
                ({"sigma_luminance": -1.0}, "sigmas must be >= 0 (and not NaN)"), ({"sigma_normal": -1.0}, "sigmas must be >= 0 (and not NaN)"),
                ({"sigma_depth": -1.0}, "sigmas must be >= 0 (and not NaN)"), ({"sigma_luminance": NAN}, "sigmas must be >= 0 (and not NaN)"),
                ({"sigma_normal": NAN}, "sigmas must be >= 0 (and not NaN)"), ({"sigma_depth": NAN}, "sigmas must be >= 0 (and not NaN)"),
                ({"iterations": 0, "sigma_depth": NAN}, "iterations must be 1..10")]
VARIANCE_OK = [{}, {"iterations": 1}, {"iterations": 10, "sigma_luminance": INF, "sigma_normal": 0.0, "sigma_depth": INF, "demodulate": 1}]


def variance_filter_entry(api, one, tiled, name, valid):
    """the three entry points of the variance-guided filter share the parameter checks and the place of the world check; `valid` is
    what valid parameters meet first on a host-only context"""
    f = getattr(api.LIB, name)
    P = lambda kw: None if kw is None else C.byref(api.DenoiseVarianceParams(**dict(api.denoise_variance_defaults(), **kw)))
    assert f(None, P({})) == api.PT_EINVAL
    for kw, why in VARIANCE_BAD:
        einval(api, one, f(one._h, P(kw)), name + ": " + why)
        einval(api, tiled, f(tiled._h, P(kw)), name + ": " + why)                                  # the parameters before the world
    for kw in VARIANCE_OK:
        valid(f(one._h, P(kw)))
        einval(api, tiled, f(tiled._h, P(kw)), world_text(name))                                   # the world before device and guides


def test_denoise_variance(api, one, tiled):
    variance_filter_entry(api, one, tiled, "pt_denoise_variance", lambda rc: einval(api, one, rc, guides_text("pt_denoise_variance")))


# ---------------------------------------------------------------------------------------------------------------- temporal
def test_temporal_accumulate(api, one, tiled):
    f = api.LIB.pt_temporal_accumulate
    P = lambda **kw: C.byref(api.TemporalParams(**dict(api.temporal_defaults(), **kw)))
    assert f(None, P()) == api.PT_EINVAL
    einval(api, one, f(one._h, None), "pt_temporal_accumulate: params is NULL")
    einval(api, one, f(one._h, P(max_history=-1)), "pt_temporal_accumulate: max_history must be >= 0")
    for v in (-1.5, 1.5, NAN):
        einval(api, one, f(one._h, P(normal_cos=v)), "pt_temporal_accumulate: normal_cos must be in [-1, 1]")
    for v in (-1e-3, NAN):
        einval(api, one, f(one._h, P(depth_tolerance=v)), "pt_temporal_accumulate: depth_tolerance must be >= 0 (and not NaN)")
    einval(api, one, f(one._h, P(max_history=-1, normal_cos=2.0, depth_tolerance=-1.0)), "pt_temporal_accumulate: max_history must be >= 0")
    einval(api, one, f(one._h, P(normal_cos=2.0, depth_tolerance=-1.0)), "pt_temporal_accumulate: normal_cos must be in [-1, 1]")
    # valid parameters: the device is asked for before the guides
    for kw in ({}, {"max_history": 0, "normal_cos": -1.0, "depth_tolerance": 0.0}, {"max_history": 2 ** 31 - 1, "normal_cos": 1.0, "depth_tolerance": INF}):
        nodevice(api, one, f(one._h, P(**kw)))
    einval(api, tiled, f(tiled._h, P(depth_tolerance=NAN)), "pt_temporal_accumulate: depth_tolerance must be >= 0 (and not NaN)")
    einval(api, tiled, f(tiled._h, P()), world_text("pt_temporal_accumulate"))


def test_denoise_temporal(api, one, tiled):
    variance_filter_entry(api, one, tiled, "pt_denoise_temporal", lambda rc: nodevice(api, one, rc))


# ---------------------------------------------------------------------------------------------------------------- firefly filter
DESPECKLE_BAD = [({"radius": 0}, "radius must be 1..3"), ({"radius": 4}, "radius must be 1..3"), ({"rank": 0}, "rank must be 1..3"),
                 ({"rank": 4}, "rank must be 1..3"), ({"threshold": 0.5}, "threshold must be >= 1 (and not NaN)"),
                 ({"threshold": NAN}, "threshold must be >= 1 (and not NaN)"), ({"floor": -1.0}, "floor must be >= 0 (and not NaN)"),
                 ({"floor": NAN}, "floor must be >= 0 (and not NaN)"), ({"min_rel_sigma": -1.0}, "min_rel_sigma must be >= 0 (and not NaN)"),
                 ({"min_rel_sigma": NAN}, "min_rel_sigma must be >= 0 (and not NaN)"), ({"spread": 2}, "spread must be 0 or 1"),
                 ({"spread": -1}, "spread must be 0 or 1")]
DESPECKLE_SOURCE_TEXT = "source must be PT_DESPECKLE_FRAME or PT_DESPECKLE_TEMPORAL"
# the order of the checks: everything from an entry on wrong at once names that entry
DESPECKLE_ORDER = [({"radius": 0}, "radius must be 1..3"), ({"rank": 0}, "rank must be 1..3"), ({"threshold": NAN}, "threshold must be >= 1 (and not NaN)"),
                   ({"floor": NAN}, "floor must be >= 0 (and not NaN)"), ({"min_rel_sigma": NAN}, "min_rel_sigma must be >= 0 (and not NaN)"),
                   ({"spread": 2}, "spread must be 0 or 1"), ({"source": 2}, DESPECKLE_SOURCE_TEXT)]
DESPECKLE_OK = [{}, {"source": 1}, {"radius": 1, "rank": 1, "threshold": 1.0, "floor": 0.0, "min_rel_sigma": 0.0, "spread": 0},
                {"radius": 3, "rank": 3, "threshold": INF, "floor": INF, "min_rel_sigma": INF, "spread": 1}]


def cumulative(order):
    for first in range(len(order)):
        kw = {}
        for more, _ in order[first:]:
            kw.update(more)
        yield kw, order[first][1]


def test_despeckle(api, one, tiled):
    f = api.LIB.pt_despeckle
    P = lambda kw: C.byref(api.DespeckleParams(**dict(api.despeckle_defaults(), **kw)))
    assert f(None, P({})) == api.PT_EINVAL
    einval(api, one, f(one._h, None), "pt_despeckle: params is NULL")
    for kw, why in DESPECKLE_BAD + [({"source": 2}, DESPECKLE_SOURCE_TEXT), ({"source": -1}, DESPECKLE_SOURCE_TEXT)] + list(cumulative(DESPECKLE_ORDER)):
        einval(api, one, f(one._h, P(kw)), "pt_despeckle: " + why)
        einval(api, tiled, f(tiled._h, P(kw)), "pt_despeckle: " + why)
    for kw in DESPECKLE_OK:
        nodevice(api, one, f(one._h, P(kw)))                                                       # the device before the source's own rule
        einval(api, tiled, f(tiled._h, P(kw)), world_text("pt_despeckle"))


def test_denoise_despeckled(api, one, tiled):
    variance_filter_entry(api, one, tiled, "pt_denoise_despeckled", lambda rc: nodevice(api, one, rc))


def test_debug_despeckle(api, one, tiled):
    f = api.LIB.pt_debug_despeckle
    P = lambda kw: C.byref(api.DespeckleParams(**dict(api.despeckle_defaults(), **kw)))
    frame, out, flags = np.ones((3, 5, 4), np.float32), np.zeros((3, 5, 4), np.float32), np.zeros((3, 5), np.int32)
    args = lambda sc, p, w=5, h=3, a=frame, b=out, c=flags: (sc._h, None if a is None else api._ptr(a), w, h, p, None if b is None else api._ptr(b),
                                                             None if c is None else api._ptr(c))
    assert f(None, api._ptr(frame), 5, 3, P({}), api._ptr(out), api._ptr(flags)) == api.PT_EINVAL
    einval(api, one, f(*args(one, None)), "pt_debug_despeckle: params is NULL")
    for kw, why in DESPECKLE_BAD + list(cumulative(DESPECKLE_ORDER[:-1])):
        einval(api, one, f(*args(one, P(kw))), "pt_debug_despeckle: " + why)
    for w, h in ((0, 3), (5, 0), (4097, 1), (1, 4097)):
        einval(api, one, f(*args(one, P({}), w, h)), "pt_debug_despeckle: w and h must be 1..4096")
    for hole in ({"a": None}, {"b": None}, {"c": None}):
        einval(api, one, f(*args(one, P({}), **hole)), "pt_debug_despeckle: NULL argument")
    einval(api, one, f(*args(one, P({"spread": 2}), 0, 3, None)), "pt_debug_despeckle: spread must be 0 or 1")       # parameters, size, pointers
    einval(api, one, f(*args(one, P({}), 0, 3, None)), "pt_debug_despeckle: w and h must be 1..4096")
    for kw in DESPECKLE_OK + [{"source": 2}, {"source": -7}]:                                      # (source is ignored)
        nodevice(api, one, f(*args(one, P(kw))))
        nodevice(api, tiled, f(*args(tiled, P(kw))))                                               # any number of ranks
    einval(api, tiled, f(*args(tiled, P({"rank": 0}))), "pt_debug_despeckle: rank must be 1..3")


# ---------------------------------------------------------------------------------------------------------------- display stage
DISPLAY_ORDER = [({"source": 4}, "source must be PT_DISPLAY_FRAME .. PT_DISPLAY_DESPECKLED"),
                 ({"metering": 2}, "metering must be PT_METER_MANUAL or PT_METER_AUTO"),
                 ({"curve": 3}, "curve must be PT_CURVE_LINEAR, PT_CURVE_REINHARD or PT_CURVE_ACES"),
                 ({"encoding": -1}, "encoding must be PT_ENCODE_SRGB or PT_ENCODE_LINEAR"),
                 ({"ev": NAN}, "a parameter is NaN"), ({"key": 0.0}, "key must be > 0"),
                 ({"low_permille": 950, "high_permille": 950}, "permille must be 0 <= low < high <= 1000"),
                 ({"min_ev": 1.0, "max_ev": 0.0}, "min_ev must be <= max_ev"), ({"adapt": 0.0}, "adapt must be in (0, 1]"),
                 ({"bloom_levels": 7}, "bloom_levels must be 1..6"), ({"bloom_threshold": -1.0}, "bloom_threshold must be >= 0"),
                 ({"bloom_intensity": -0.5}, "bloom_intensity must be >= 0"), ({"white": 0.0}, "white must be > 0")]
DISPLAY_BAD = DISPLAY_ORDER[1:] + [
    ({"metering": -1}, "metering must be PT_METER_MANUAL or PT_METER_AUTO"), ({"curve": -1}, "curve must be PT_CURVE_LINEAR, PT_CURVE_REINHARD or PT_CURVE_ACES"),
    ({"encoding": 2}, "encoding must be PT_ENCODE_SRGB or PT_ENCODE_LINEAR"), ({"key": NAN}, "a parameter is NaN"), ({"min_ev": NAN}, "a parameter is NaN"),
    ({"max_ev": NAN}, "a parameter is NaN"), ({"adapt": NAN}, "a parameter is NaN"), ({"bloom_threshold": NAN}, "a parameter is NaN"),
    ({"bloom_intensity": NAN}, "a parameter is NaN"), ({"white": NAN}, "a parameter is NaN"), ({"key": -1.0}, "key must be > 0"),
    ({"low_permille": -1}, "permille must be 0 <= low < high <= 1000"), ({"high_permille": 1001}, "permille must be 0 <= low < high <= 1000"),
    ({"low_permille": 960}, "permille must be 0 <= low < high <= 1000"), ({"adapt": 1.5}, "adapt must be in (0, 1]"), ({"adapt": -0.1}, "adapt must be in (0, 1]"),
    ({"bloom_levels": 0}, "bloom_levels must be 1..6"), ({"white": -2.0}, "white must be > 0")]
DISPLAY_OK = [{}, {"source": 1}, {"source": 2}, {"source": 3}, {"metering": 0, "ev": -INF}, {"min_ev": -INF, "max_ev": INF, "white": 1e-3},
              {"low_permille": 0, "high_permille": 1000, "adapt": 1e-3, "bloom_levels": 6, "bloom_threshold": 0.0, "bloom_intensity": INF},
              {"curve": 0, "encoding": 1, "bloom_levels": 1, "adapt": 1.0}]


def test_display(api, one, tiled):
    f = api.LIB.pt_display
    P = lambda kw: C.byref(api.DisplayParams(**dict(api.display_defaults(), **kw)))
    assert f(None, P({})) == api.PT_EINVAL
    einval(api, one, f(one._h, None), "pt_display: params is NULL")
    for kw, why in DISPLAY_BAD + [({"source": 4}, DISPLAY_ORDER[0][1]), ({"source": -1}, DISPLAY_ORDER[0][1])] + list(cumulative(DISPLAY_ORDER)):
        einval(api, one, f(one._h, P(kw)), "pt_display: " + why)
        einval(api, tiled, f(tiled._h, P(kw)), "pt_display: " + why)
    for kw in DISPLAY_OK:
        nodevice(api, one, f(one._h, P(kw)))                                                       # the device before the source's own rule
        einval(api, tiled, f(tiled._h, P(kw)), world_text("pt_display"))


def test_read_display_and_info(api, one, tiled):
    rgba, rgb8, info = np.zeros((W * H, 4), np.float32), np.zeros((H, W, 3), np.uint8), api.DisplayInfo()
    f = api.LIB.pt_read_display
    assert f(None, api._ptr(rgba), api._ptr(rgb8), W * H) == api.PT_EINVAL
    nodevice(api, one, f(one._h, api._ptr(rgba), api._ptr(rgb8), W * H))
    nodevice(api, one, f(one._h, api._ptr(rgba), api._ptr(rgb8), 5))                              # the device before npix
    nodevice(api, one, f(one._h, None, None, W * H))
    nodevice(api, tiled, f(tiled._h, api._ptr(rgba), api._ptr(rgb8), tiled.local_pixels))
    g = api.LIB.pt_display_info
    assert g(None, C.byref(info)) == api.PT_EINVAL
    nodevice(api, one, g(one._h, C.byref(info)))
    nodevice(api, one, g(one._h, None))                                                            # the device before the argument
    nodevice(api, tiled, g(tiled._h, C.byref(info)))


def test_display_reset(api, one, tiled):
    f = api.LIB.pt_display_reset
    assert f(None) == api.PT_EINVAL
    assert f(one._h) == api.PT_OK                                                                  # needs no device
    assert f(tiled._h) == api.PT_OK                                                                # and any number of ranks


def test_debug_display(api, one, tiled):
    f = api.LIB.pt_debug_display
    P = lambda kw: C.byref(api.DisplayParams(**dict(api.display_defaults(), **kw)))
    frame = np.ones((3, 5, 4), np.float32)
    args = lambda sc, p, w=5, h=3, a=frame, prev=0.0: (sc._h, None if a is None else api._ptr(a), w, h, p, prev, None, None, None, None)
    assert f(None, api._ptr(frame), 5, 3, P({}), 0.0, None, None, None, None) == api.PT_EINVAL
    einval(api, one, f(*args(one, None)), "pt_debug_display: params is NULL")
    for kw, why in DISPLAY_BAD + list(cumulative(DISPLAY_ORDER[1:])):
        einval(api, one, f(*args(one, P(kw))), "pt_debug_display: " + why)
    for w, h in ((0, 3), (5, 0), (4097, 1), (1, 4097)):
        einval(api, one, f(*args(one, P({}), w, h)), "pt_debug_display: w and h must be 1..4096")
    einval(api, one, f(*args(one, P({}), a=None)), "pt_debug_display: rgba_in is NULL or prev_exposure is NaN")
    einval(api, one, f(*args(one, P({}), prev=NAN)), "pt_debug_display: rgba_in is NULL or prev_exposure is NaN")
    einval(api, one, f(*args(one, P({"white": 0.0}), 0, 3, None)), "pt_debug_display: white must be > 0")             # parameters, size, pointers
    einval(api, one, f(*args(one, P({}), 0, 3, None)), "pt_debug_display: w and h must be 1..4096")
    for kw in DISPLAY_OK + [{"source": 7}, {"source": -1}]:                                        # (source is ignored)
        nodevice(api, one, f(*args(one, P(kw))))
        nodevice(api, tiled, f(*args(tiled, P(kw))))                                               # any number of ranks
    nodevice(api, one, f(*args(one, P({}), prev=2.5)))
    einval(api, tiled, f(*args(tiled, P({"key": 0.0}))), "pt_debug_display: key must be > 0")
