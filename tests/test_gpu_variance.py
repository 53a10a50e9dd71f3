"""-m gpu: the second moment in colors[].w (option "moments") and the variance read-out (pt_read_variance).

  * .w is the pinned recurrence over the oracle's samples, bit for bit, in every render path: node modes, schedules, chained and
    tapered launches, LEAN and plain instances, the wavefront variant, pt_trace_rays, pt_render_nee (BSDF), adaptive frames, tiled ranks;
  * nothing else moves: .xyz, rnds and rays equal a moments-off run, and a moments-off run writes .w = 0;
  * pt_read_variance is the pinned formula over read_colors() and the sample counts; frame validity;
  * the reported variance agrees with the spread of independent runs."""

import numpy as np
import pytest

import variance_ref as V

pytestmark = pytest.mark.gpu

B = 8


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def replay_moments(oracle, osc, spec, W, H, bounces, spp):
    """m2 after 1..spp samples for every pixel of the frame: sample s is one oracle sample with first_sample = 0 rendered from the LCG
    state the frame has reached, so the oracle's colours are x_s exactly.  Returns [m2 after s + 1 samples for s in range(spp)]."""
    cam = oracle.make_camera(spec.fov, spec.yaw, spec.pitch, spec.shift, W, H)
    fr = oracle.OracleFrame(W, H)
    m2 = np.zeros(W * H, np.float32)
    out = []
    for s in range(spp):
        fr.render(osc, cam, bounces, 0, 1, nthreads=16)
        m2 = V.fold_moment(m2, fr.colors()[:, :3], s)
        out.append(m2.copy())
    return out


_REPLAY = {}


def cb_replay(oracle, osc, spec, W, H, spp):
    key = (W, H, spp)
    if key not in _REPLAY:
        _REPLAY[key] = replay_moments(oracle, osc, spec, W, H, B, spp)
    return _REPLAY[key]


def run(api, spec, W, H, steps, moments, pre=None, opts=None, how="render", **kw):
    sc = api.Scene(W, H, **kw)
    for k, v in (pre or {}).items():
        sc.set_option(k, v)
    sc.load(spec)
    for k, v in (opts or {}).items():
        sc.set_option(k, v)
    sc.set_option("moments", moments)
    sc.iterations = B
    for n in steps:
        if how == "render":
            sc.render(n)
        elif how == "trace":
            sc.render(n, fused=False)
        elif how == "nee":
            sc.render_nee(n, "bsdf")
    return sc


def check_path(api, oracle, cb_spec, cb_oracle_scene, W, H, steps, pre=None, opts=None, how="render", what=""):
    spp = sum(steps)
    m2 = cb_replay(oracle, cb_oracle_scene, cb_spec, W, H, spp)[spp - 1]
    on = run(api, cb_spec, W, H, steps, 1, pre, opts, how)
    off = run(api, cb_spec, W, H, steps, 0, pre, opts, how)
    c_on, c_off = on.read_colors(), off.read_colors()
    assert same_bits(c_on[:, 3], m2), what
    assert same_bits(c_on[:, :3], c_off[:, :3]), what
    assert np.array_equal(on.read_rnds(), off.read_rnds()), what
    r_on, r_off = on.read_rays(), off.read_rays()
    assert same_bits(r_on["P"][:, :3], r_off["P"][:, :3]) and same_bits(r_on["D"][:, :3], r_off["D"][:, :3]), what
    assert not np.any(c_off[:, 3].view(np.uint32)), what
    return on


# ---------------------------------------------------------------------------- 1 + 2: bit-exact second moment, nothing else moves
@pytest.mark.parametrize("lds,wide,mode", [(2, 1, 0), (0, 1, 1), (2, 2, 3)])
@pytest.mark.parametrize("schedule", [0, 1, 2])
def test_moment_node_modes_and_schedules(api, oracle, cb_spec, cb_oracle_scene, lds, wide, mode, schedule):
    sc = check_path(api, oracle, cb_spec, cb_oracle_scene, 48, 40, (2, 3), pre={"wide_nodes": wide},
                    opts={"lds_scene": lds, "schedule": schedule}, what="lds %d wide %d schedule %d" % (lds, wide, schedule))
    assert sc.stat("node_mode") == mode


@pytest.mark.parametrize("wps", [4, 7])
@pytest.mark.parametrize("schedule", [0, 1, 2])
def test_moment_plain_and_lean_instances(api, oracle, cb_spec, cb_oracle_scene, wps, schedule):
    """waves_per_simd 4 carries the moment in a register through the work item, 7 folds it into colors[] at every sample (LEAN)."""
    check_path(api, oracle, cb_spec, cb_oracle_scene, 48, 40, (2, 3), opts={"lds_scene": 0, "waves_per_simd": wps, "schedule": schedule},
               what="wps %d schedule %d" % (wps, schedule))


@pytest.mark.parametrize("schedule", [1, 2])
def test_moment_chained_and_tapered_launch(api, oracle, cb_spec, cb_oracle_scene, schedule):
    check_path(api, oracle, cb_spec, cb_oracle_scene, 48, 40, (7,), opts={"schedule": schedule, "chunk_spp": 4, "chunk_taper": 1},
               what="chained + tapered, schedule %d" % schedule)
    check_path(api, oracle, cb_spec, cb_oracle_scene, 48, 40, (7,), opts={"schedule": schedule, "chunk_spp": 2},
               what="chained, schedule %d" % schedule)


def test_moment_wavefront_variant(api, oracle, cb_spec, cb_oracle_scene):
    check_path(api, oracle, cb_spec, cb_oracle_scene, 48, 40, (2, 3), opts={"variant": 1}, what="wavefront")


def test_moment_trace_rays(api, oracle, cb_spec, cb_oracle_scene):
    check_path(api, oracle, cb_spec, cb_oracle_scene, 48, 40, (2, 3), how="trace", what="pt_trace_rays")


def test_moment_nee_bsdf_equals_render(api, oracle, cb_spec, cb_oracle_scene):
    nee = check_path(api, oracle, cb_spec, cb_oracle_scene, 48, 40, (2, 3), how="nee", what="pt_render_nee")
    ren = run(api, cb_spec, 48, 40, (2, 3), 1)
    assert same_bits(nee.read_colors(), ren.read_colors())


def test_moment_tiled_rank(api, oracle, cb_spec, cb_oracle_scene):
    W, H = 48, 40
    m2 = cb_replay(oracle, cb_oracle_scene, cb_spec, W, H, 5)[4]
    for r in range(2):
        sc = run(api, cb_spec, W, H, (2, 3), 1, rank=r, world=2, rows_per_block=8)
        ids = sc.local_pixel_ids()
        c = sc.read_colors()
        assert same_bits(c[:, 3], m2[ids])
        v = sc.read_variance().reshape(-1)
        assert same_bits(v, V.variance(c, 5))


def test_moment_adaptive_frame(api, oracle, cb_spec, cb_oracle_scene):
    """Retired tiles hold the moment at their own sample count; the read-out uses that count."""
    W, H = 48, 40
    reps = cb_replay(oracle, cb_oracle_scene, cb_spec, W, H, 16)
    sc = api.Scene(W, H).load(cb_spec)
    sc.set_option("moments", 1)
    sc.iterations = B
    for threshold in (0.5, 0.25, 1.0, 0.125, 2.0):          # the first that retires some tiles but not all
        sc.seed_default()
        sc.current_sample = 0
        sc.render_adaptive(4, 16, threshold)
        n = sc.sample_counts().reshape(-1)
        if len(set(n.tolist())) > 1:
            break
    assert len(set(n.tolist())) > 1, "no threshold retired some tiles but not all: the test needs both"
    c = sc.read_colors()
    want = np.empty(W * H, np.float32)
    for k in np.unique(n):
        want[n == k] = reps[k - 1][n == k]
    assert same_bits(c[:, 3], want)
    assert same_bits(sc.read_variance().reshape(-1), V.variance(c, n))


# ---------------------------------------------------------------------------- 3: the read-out and frame validity
def test_read_variance_formula_and_validity(api, cb_spec):
    W, H = 40, 24
    sc = run(api, cb_spec, W, H, (1,), 1)
    v = sc.read_variance().reshape(-1)
    assert np.all(np.isinf(v) & (v > 0))                              # n = 1
    sc.render(3)
    c = sc.read_colors()
    v = sc.read_variance().reshape(-1)
    assert same_bits(v, V.variance(c, 4))
    assert np.all(np.isfinite(v)) and np.all(v >= 0) and np.any(v > 0)
    assert sc.device_variance()                                      # the same buffer, left on the device
    # moments switched on mid-frame: the frame is invalid until the next one starts
    off = run(api, cb_spec, W, H, (2,), 0)
    for call in (lambda: off.read_variance(), lambda: off.device_variance()):
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_EINVAL
    off.set_option("moments", 1)
    off.render(2)
    with pytest.raises(api.PtError) as e:
        off.read_variance()
    assert e.value.code == api.PT_EINVAL
    off.current_sample = 0
    with pytest.raises(api.PtError) as e:                             # a frame with no samples
        off.read_variance()
    assert e.value.code == api.PT_EINVAL
    off.render(4)
    assert same_bits(off.read_variance().reshape(-1), V.variance(off.read_colors(), 4))


# ---------------------------------------------------------------------------- 4: the reported variance against independent runs
def test_variance_matches_spread_of_independent_runs(api, cb_spec):
    from opencl_path_tracer_amd import scenes
    spec = scenes.SceneSpec(materials=cb_spec.materials, objects=[scenes.cornell_walls()], name="walls")
    W = H = 32
    runs, means, reported = 64, [], []
    rng = np.random.default_rng(7)
    sc = api.Scene(W, H).load(spec)
    sc.set_option("moments", 1)
    sc.iterations = 4
    sc.render_aovs(1, 4)
    mat = sc.read_aovs()[0][:, 3].astype(np.int64).reshape(H, W)
    for _ in range(runs):
        sc.upload_seeds(rng.integers(1, 2**31 - 1, size=W * H, dtype=np.int64).astype(np.int32))
        sc.current_sample = 0
        sc.render(16)
        c = sc.read_colors()
        means.append(V.luminance(c).astype(np.float64))
        reported.append(sc.read_variance().reshape(-1).astype(np.float64))
    emit = np.isin(mat, [i for i, m in enumerate(spec.materials) if m[6] == 3])
    pad = np.pad(emit, 1)                           # the 3x3 neighbourhood inside the frame (no wrap-around)
    near = np.zeros_like(emit)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            near |= pad[dy:dy + H, dx:dx + W]
    keep = (~near).reshape(-1)
    keep &= (mat.reshape(-1) >= 0)
    emp = np.var(np.stack(means), axis=0, ddof=1)
    rep = np.mean(np.stack(reported), axis=0)
    ratio = emp[keep].sum() / rep[keep].sum()
    print("[variance] 32x32 walls, 16 spp, 64 runs: empirical / reported = %.4f over %d pixels" % (ratio, int(keep.sum())))
    assert 0.8 <= ratio <= 1.25, ratio
