"""-m gpu: the display stage (Scene.display, pt_display; pinned in include/pt_api.h) against the float64 model tests/display_ref.py.

  * the kernels, through pt_debug_display, on the authored frames under manual and auto metering, three curves, two encodings, and no
    bloom / 1 / 2 / 6 levels: histogram and counts exact, E, the float result and the bytes within the model's derived bound;
  * pass-through, determinism, independence of the tiling, the bloom's closed form, adaptation;
  * the four sources on a rendered frame bit for bit against the debug entry, their refusals, what must stay untouched, the PPM, a
    bound framebuffer.

The bound's three library terms (exp2f, log2f, powf) are measured here against float64 with torch's device functions over the arguments
the stage can reach, never from pt_display's output; the model gets twice the measured values (profiles/display/README.md quotes them)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import display_ref as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = D.authored()
CONFIGS = D.configs()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ctx(api, cb_spec):
    sc = api.Scene(8, 8).load(cb_spec)
    yield sc
    sc.close()


_EPS_CHILD = r"""
import json
import numpy as np, torch
KNEE = %(knee)r
rng = np.random.RandomState(11)
n = 1 << 18
dev = lambda a: torch.from_numpy(a).cuda()
x = rng.uniform(-40.0, 40.0, n).astype(np.float32)
e_exp2 = np.abs(torch.exp2(dev(x)).cpu().numpy().astype(np.float64) / np.exp2(x.astype(np.float64)) - 1.0).max()
y = np.exp2(rng.uniform(-40.0, 40.0, n)).astype(np.float32)
want = np.log2(y.astype(np.float64))
e_log2 = (np.abs(torch.log2(dev(y)).cpu().numpy().astype(np.float64) - want) / np.maximum(np.abs(want), 1.0)).max()
v = np.concatenate([rng.uniform(KNEE, 1.0, n // 2), np.exp(rng.uniform(np.log(KNEE), 0.0, n // 2))]).astype(np.float32)
ex = float(np.float32(1.0 / 2.4))
e_pow = np.abs(torch.pow(dev(v), ex).cpu().numpy().astype(np.float64) / np.power(v.astype(np.float64), ex) - 1.0).max()
print("EPS " + json.dumps({"exp2": float(e_exp2), "log2": float(e_log2), "pow": float(e_pow)}))
"""


@pytest.fixture(scope="module")
def eps():
    """twice the measured error of the device's exp2f, log2f and powf(v, 1 / 2.4f) (display_ref's docstring names the three measures),
    taken with torch's device functions in a child process, as the other tests that put torch next to the library do"""
    out = subprocess.run([sys.executable, "-c", _EPS_CHILD % {"knee": D.KNEE}], capture_output=True, text=True, timeout=300)
    line = [l for l in out.stdout.splitlines() if l.startswith("EPS ")]
    assert line, out.stdout[-2000:] + out.stderr[-4000:]
    m = json.loads(line[0][4:])
    print("[display] measured library error: exp2f %.3g (relative), log2f %.3g (over max(|log2 x|, 1)), powf(v, 1/2.4) %.3g (relative); 2^-24 = %.3g"
          % (m["exp2"], m["log2"], m["pow"], D.U))
    return {k: 2.0 * v for k, v in m.items()}


def _check(name, frame, got, want):
    rgba, rgb8, hist, info = got
    h, w = frame.shape[:2]
    assert rgba.shape == (h, w, 4) and rgb8.shape == (h, w, 3) and hist.shape == (256,)
    assert np.array_equal(hist, want["hist"]), (name, np.flatnonzero(hist != want["hist"])[:8])
    assert (info["n_dark"], info["n_nonfinite"], info["n_metered"]) == (want["n_dark"], want["n_nonfinite"], want["K"]), name
    assert info["levels"] == want["levels"]
    assert abs(info["exposure"] - want["E"]) <= (want["E_rtol"] + D.U) * want["E"], (name, info["exposure"], want["E"], want["E_rtol"])
    if want["K"]:
        assert abs(info["mean_log2"] - want["M"]) <= want["M_atol"] + D.U * abs(want["M"]), name
    assert not np.isnan(rgba).any(), name
    assert np.all(rgba[..., 3] == 1.0)
    dead = ~want["live"]
    assert not rgba[dead][:, :3].any() and not rgb8[::-1][dead].any(), "%s: a pixel that is not live is not {0, 0, 0, 1}" % name
    err = np.abs(rgba[..., :3].astype(np.float64) - want["v"])
    ratio = err / np.maximum(want["tol"], 1e-300)
    worst = np.unravel_index(np.argmax(np.where(err > 0, ratio, 0.0)), err.shape)
    assert np.all(err <= want["tol"]), (name, worst, err[worst], want["tol"][worst], rgba[worst[:2]], want["v"][worst[:2]])
    d = rgb8.astype(np.int64) - want["rgb8"].astype(np.int64)
    assert not d[want["decidable"]].any(), (name, np.argwhere(want["decidable"] & (d != 0))[:8])
    assert np.abs(d).max() <= 1, name
    return float(np.where(err > 0, ratio, 0.0).max())


# ---------------------------------------------------------------------------------------------------------- 1. authored frames
@pytest.mark.parametrize("k", range(len(FRAMES)), ids=[n for n, _ in FRAMES])
def test_authored_frame(ctx, eps, k):
    name, frame = FRAMES[k]
    worst = 0.0
    for cname, p in CONFIGS:
        want = D.display(frame, eps=eps, **p)
        worst = max(worst, _check("%s / %s" % (name, cname), frame, ctx.debug_display(frame, **p), want))
    print("[display] %-36s %d configurations, worst error / bound %.3f" % (name, len(CONFIGS), worst))


# ---------------------------------------------------------------------------------------------------------- 2. pass-through, determinism
def test_pass_through_is_bit_exact(ctx):
    for name, frame in FRAMES:
        rgba, rgb8, _, info = ctx.debug_display(frame, metering="manual", ev=0.0, curve="linear", encoding="linear", bloom_intensity=0.0)
        assert info["exposure"] == 1.0 and info["levels"] == 0
        live, _ = D.live_of(frame)
        c = np.where(live[..., None], frame[..., :3], np.float32(0))
        want = np.where(c > 0, np.minimum(c, np.float32(1)), np.float32(0)).astype(np.float32)
        assert np.array_equal(_bits(rgba[..., :3]), _bits(want)), name


def test_two_runs_same_bits(ctx):
    frame = dict(FRAMES)["64x64 blobs with non-finite"]
    p = dict(D.BLOOM, bloom_levels=6)
    a, b = ctx.debug_display(frame, **p), ctx.debug_display(frame, **p)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


# ---------------------------------------------------------------------------------------------------------- 3. tiling
def test_result_does_not_depend_on_the_tiling(ctx, eps):
    """the 33 x 31 frame at two offsets (multiples of 2^levels) in a 64 x 64 zero frame: the same picture, shifted"""
    small = dict(FRAMES)["33x31 blobs"]
    p = dict(metering=D.MANUAL, ev=-6.0, curve=D.LINEAR, encoding=D.ENC_LINEAR, bloom_levels=2, bloom_threshold=0.05, bloom_intensity=0.5)
    res = []
    for ox, oy in ((12, 12), (16, 20)):
        big = np.zeros((64, 64, 4), np.float32)
        big[oy:oy + 31, ox:ox + 33] = small
        want = D.display(big, eps=eps, **p)
        assert not want["touches_border"] and want["v"].max() < 1.0 and want["bloom"].max() > 0.01
        got = ctx.debug_display(big, **p)
        _check("embedded at (%d, %d)" % (ox, oy), big, got, want)
        pad = 8                                                  # the picture with the bloom around it
        res.append((got[0][oy - pad:oy + 31 + pad, ox - pad:ox + 33 + pad, :3].astype(np.float64), want["tol"][oy - pad:oy + 31 + pad, ox - pad:ox + 33 + pad]))
    (a, ta), (b, tb) = res
    assert np.all(np.abs(a - b) <= ta + tb)


def test_corner_impulse_matches_the_clamped_edges(ctx, eps):
    frame = dict(FRAMES)["33x31 impulse in a corner"]
    p = dict(metering=D.MANUAL, ev=-8.0, curve=D.LINEAR, encoding=D.ENC_LINEAR, bloom_levels=3, bloom_threshold=0.01, bloom_intensity=1.0)
    want = D.display(frame, eps=eps, **p)
    assert want["touches_border"] and want["v"].max() < 1.0
    _check("corner impulse", frame, ctx.debug_display(frame, **p), want)


# ---------------------------------------------------------------------------------------------------------- 4. the bloom's closed form
@pytest.mark.parametrize("levels", [1, 2])
def test_bloom_closed_form(ctx, eps, levels):
    frame = dict(FRAMES)[D.IMPULSE]
    p = dict(metering=D.MANUAL, ev=-10.0, curve=D.LINEAR, encoding=D.ENC_LINEAR, bloom_levels=levels, bloom_threshold=2.0 ** -12, bloom_intensity=0.5)
    want = D.display(frame, eps=eps, **p)
    assert not want["touches_border"] and want["v"].max() < 1.0
    rgba = ctx.debug_display(frame, **p)[0]
    add = (rgba[..., :3].astype(np.float64) - want["h"]).sum(axis=(0, 1))
    closed = 0.5 * want["B"].sum(axis=(0, 1))
    assert np.all(closed > 0) and np.all(np.abs(add - closed) <= want["tol"].sum(axis=(0, 1))), (add, closed)


# ---------------------------------------------------------------------------------------------------------- 5. adaptation
def test_adaptation_from_a_given_exposure(ctx, eps):
    frame = dict(FRAMES)["33x31 blobs"]
    for prev in (4.0, 0.01):
        want = D.display(frame, prev_exposure=prev, eps=eps, adapt=0.25)
        target = D.display(frame, eps=eps)["E"]
        assert want["E"] == pytest.approx(float(np.float32(prev)) ** 0.75 * target ** 0.25, rel=1e-9) and abs(want["E"] / target - 1) > 0.1
        _check("adapt from %g" % prev, frame, ctx.debug_display(frame, prev_exposure=prev, adapt=0.25), want)
    # manual metering does not adapt; adapt = 1 ignores the remembered value
    assert ctx.debug_display(frame, prev_exposure=4.0, adapt=0.25, metering="manual", ev=1.0)[3]["exposure"] == 2.0
    assert ctx.debug_display(frame, prev_exposure=4.0)[3] == ctx.debug_display(frame)[3]


# ---------------------------------------------------------------------------------------------------------- 6. a rendered frame
W = H = 64


@pytest.fixture(scope="module")
def rendered(api, cb_spec):
    """The Cornell box, 64 x 64, 8 bounces, 16 spp, moments on; every source refuses before its producer, then the producers run."""
    sc = api.Scene(W, H).load(cb_spec)
    sc.set_option("moments", 1)
    sc.iterations = 8
    sc.render(16)
    refused = []
    for s in ("denoised", "temporal", "despeckled"):
        with pytest.raises(api.PtError) as e:
            sc.display(source=s)
        refused.append(e.value.code)
    with pytest.raises(api.PtError) as e:
        sc.read_display()
    refused.append(e.value.code)
    assert sc.device_display() is None
    sc.render_aovs()
    sc.temporal_accumulate()
    sc.despeckle()
    sc.denoise_variance()
    sc.refused = refused
    yield sc
    sc.close()


def test_sources_refuse_before_their_producers(api, rendered):
    assert rendered.refused == [api.PT_EINVAL] * 4


def test_adaptation_on_a_context(rendered, eps):
    sc = rendered
    sc.display_reset()
    sc.display(adapt=0.5)
    e1 = sc.display_info()["exposure"]
    sc.display(adapt=0.5, ev=2.0)                       # target 4 e1, half way in log2: 2 e1
    e2 = sc.display_info()["exposure"]
    tol = np.log(2.0) * (eps["log2"] * 8 + 8 * D.U * 16) + eps["exp2"] + 2 * eps["exp2"]
    assert abs(e2 / (2.0 * e1) - 1.0) <= tol, (e1, e2)
    sc.display(adapt=0.5, ev=2.0)                       # and half of the rest: 2^1.5 e1
    assert abs(sc.display_info()["exposure"] / (2.0 ** 1.5 * e1) - 1.0) <= 2 * tol
    sc.display_reset()
    sc.display(adapt=0.5)
    assert sc.display_info()["exposure"] == e1


@pytest.mark.parametrize("source", ["frame", "denoised", "temporal", "despeckled"])
def test_each_source_equals_the_debug_entry_on_its_read_out(api, rendered, source):
    sc = rendered
    keep = lambda: (sc.read_colors(), sc.read_rnds(), sc.read_denoised(), sc.read_despeckled()[0], sc.read_temporal()[0], sc.resolve_ldr(0))
    before = keep()
    read = {"frame": sc.read_colors, "denoised": sc.read_denoised, "temporal": lambda: sc.read_temporal()[0], "despeckled": lambda: sc.read_despeckled()[0]}[source]
    frame = read().reshape(H, W, 4)
    sc.display_reset()
    for p in (dict(), dict(D.BLOOM, bloom_levels=3, bloom_threshold=0.5, curve="reinhard", white=4.0)):
        sc.display(source=source, **p)
        rgba, rgb8 = sc.read_display()
        info, hist = sc.display_info(), sc.display_histogram()
        assert sc.device_display()
        d_rgba, d_rgb8, d_hist, d_info = sc.debug_display(frame, **p)
        assert np.array_equal(_bits(rgba.reshape(H, W, 4)), _bits(d_rgba)) and np.array_equal(rgb8, d_rgb8)
        assert np.array_equal(hist, d_hist) and info == d_info
        assert info["n_metered"] > 0 and 0 < rgb8.mean() < 255
    after = keep()
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_ppm_round_trip(api, rendered, tmp_path):
    sc = rendered
    sc.display(source="frame")
    rgb8 = sc.read_display()[1]
    path = str(tmp_path / "display.ppm")
    sc.write_display_ppm(path)
    back = api.read_ppm(path)
    assert back.shape == (H, W, 3) and np.array_equal(np.rint(back * 255.0).astype(np.uint8), rgb8)
    assert open(path, "rb").read(15).startswith(b"P6\n64 64\n255\n")


_BOUND_CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np, torch
from opencl_path_tracer_amd import api, scenes
torch.cuda.init()
W = H = 64
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
sc = api.Scene(W, H).load(scenes.cornell_box())
colors = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda:0")
rnds = torch.zeros((W * H,), dtype=torch.int32, device="cuda:0")
sc.bind_framebuffer(colors.data_ptr(), rnds.data_ptr())
sc.iterations = 4
sc.render(4)
sc.sync()
frame = colors.cpu().numpy().reshape(H, W, 4)
assert frame[..., :3].max() > 0
sc.display(source="frame")
rgba, rgb8 = sc.read_display()
d_rgba, d_rgb8, _, d_info = sc.debug_display(frame)
assert np.array_equal(bits(rgba.reshape(H, W, 4)), bits(d_rgba)) and np.array_equal(rgb8, d_rgb8) and sc.display_info() == d_info
assert 0 < rgb8.mean() < 255
colors.mul_(0.0)                 # the tensor itself is what is read: a changed tensor gives another picture
torch.cuda.synchronize()
sc.display(source="frame", metering="manual")
assert not sc.read_display()[1].any()
sc.close()
print("BOUND_OK")
"""


def test_bound_framebuffer_is_the_frame_source():
    """In a child process, as the other tests that put torch next to the library do."""
    out = subprocess.run([sys.executable, "-c", _BOUND_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=300)
    assert "BOUND_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
