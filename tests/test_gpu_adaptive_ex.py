"""-m gpu: pt_render_adaptive_ex -- the variance metric and the NEE path of adaptive frames -- against CPU replays, bit for bit.

Snapshots of a uniform render at every round boundary come from the oracle (megakernel path; the second moment is folded with
variance_ref.fold_moment over the oracle's single samples) or from a second Scene that renders pt_render_nee uniformly (NEE path: that
path is the parent's, and the existing tests hold it to the float64 models).  tests/adaptive_variance_ref.py replays the decisions; a
pixel that stopped after k samples must hold the snapshot at k in colours (all four lanes), rnds and (NEE) rays, and the tile counts,
tile errors (bits), rounds and active tile counts must be the replay's.

Every replay picks its threshold from the reference's own tile errors at the first decision; the counts must then take >= 3 distinct
values and the last round must render fewer tiles than the first, else the test fails (it would show nothing)."""
import numpy as np
import pytest

import adaptive_ref as R
import adaptive_variance_ref as AV
import variance_ref as V

pytestmark = pytest.mark.gpu

MIN_SPP, MAX_SPP, BOUNCES = 4, 64, 8
SIZES = [(100, 70), (96, 64)]
QUANTILES = (0.5, 0.6, 0.4, 0.75, 0.3, 0.25, 0.9, 0.1)
_CACHE = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def oracle_snapshots(oracle, osc, spec, W, H, lo, hi, key):
    """(colours with the replayed second moment in .w, rnds) of the oracle's uniform render at every boundary."""
    key = ("oracle",) + key
    if key in _CACHE:
        return _CACHE[key]
    cam = oracle.make_camera(spec.fov, spec.yaw, spec.pitch, spec.shift, W, H)
    fr, one = oracle.OracleFrame(W, H), oracle.OracleFrame(W, H)
    m2 = np.zeros(W * H, np.float32)
    snaps, prev = {}, 0
    for b in R.rounds(lo, hi):
        fr.render(osc, cam, BOUNCES, prev, b - prev, nthreads=16)
        for s in range(prev, b):             # sample s alone, from the LCG state the frame has reached: its colour is x_s
            one.render(osc, cam, BOUNCES, 0, 1, nthreads=16)
            m2 = V.fold_moment(m2, one.colors()[:, :3], s)
        assert np.array_equal(one.rnds(), fr.rnds())
        c = fr.colors().copy()
        c[:, 3] = m2
        snaps[b] = (c, fr.rnds().copy())
        prev = b
    _CACHE[key] = snaps
    return snaps


def nee_snapshots(api, spec, W, H, lo, hi, strategy, env, key):
    """(colours, rnds, ray origins, ray directions) of a uniform pt_render_nee frame (moments on) at every boundary."""
    key = ("nee", strategy, env is not None) + key
    if key in _CACHE:
        return _CACHE[key]
    un = api.Scene(W, H).load(spec)
    un.set_option("moments", 1)
    un.iterations = BOUNCES
    if env is not None:
        un.set_environment(env)
    snaps, prev = {}, 0
    for b in R.rounds(lo, hi):
        un.render_nee(b - prev, strategy)
        r = un.read_rays()
        snaps[b] = (un.read_colors().copy(), un.read_rnds().copy(), r["P"].copy(), r["D"].copy())
        prev = b
    un.close()
    _CACHE[key] = snaps
    return snaps


def pick(snaps, W, H, lo, hi, metric, tonemapped):
    """A threshold from the reference's own tile errors at the first decision that makes the replay worth running."""
    b = R.rounds(lo, hi)
    if metric == AV.HALF:
        e1 = R.tile_errors(snaps[b[1]][0], snaps[b[0]][0], W, H)
    else:
        e1 = AV.tile_errors(snaps[b[1]][0], b[1], W, H, tonemapped)
    tried = []
    for q in QUANTILES:
        thr = np.float32(np.quantile(e1[np.isfinite(e1)], q))
        ref = AV.replay(snaps, W, H, lo, hi, thr, metric=metric, tonemapped=tonemapped)
        tried.append((q, sorted(set(ref["spp"].tolist())), ref["active_tiles"]))
        if len(set(ref["spp"].tolist())) >= 3 and ref["active_tiles"][-1] < ref["active_tiles"][0]:
            return thr, ref
    raise AssertionError("no quantile gives >= 3 distinct tile counts and a shrinking last round: the replay would be vacuous %r" % (tried,))


def check(sc, res, ref, what, lanes=4, rays=False, stat=True):
    spp, err = sc.tile_state()
    print("[%s] rounds %s active %s" % (what, res["rounds"], res["active_tiles"]))
    assert np.array_equal(spp, ref["spp"]), "%s: tile counts differ" % what
    assert same_bits(err, ref["err"]), "%s: tile errors differ in bits" % what
    assert np.array_equal(sc.sample_counts().reshape(-1), ref["pixel_spp"]), what
    cols, rnds = sc.read_colors(), sc.read_rnds()
    assert int((rnds != ref["rnds"]).sum()) == 0, "%s: %d pixels consumed a different number of draws" % (what, int((rnds != ref["rnds"]).sum()))
    assert same_bits(cols[:, :lanes], ref["colors"][:, :lanes]), "%s: colours differ in bits" % what
    if rays:
        r = sc.read_rays()
        assert same_bits(r["P"], ref["extra"][0]) and same_bits(r["D"], ref["extra"][1]), "%s: rays differ in bits" % what
    total = int(ref["pixel_spp"].sum(dtype=np.int64))
    if stat:
        assert sc.stat("samples") == total, what
    assert sc.current_sample == int(ref["spp"].max())
    assert res["rounds"] == ref["rounds"] and res["active_tiles"] == ref["active_tiles"], (what, res, ref["rounds"], ref["active_tiles"])
    assert res["samples"] == total


def scene(api, spec, W, H, moments, opts=None, env=None):
    sc = api.Scene(W, H)
    for k, v in (opts or {}).items():
        sc.set_option(k, v)
    sc.load(spec)
    sc.set_option("moments", moments)
    sc.iterations = BOUNCES
    if env is not None:
        sc.set_environment(env)
    return sc


# ---------------------------------------------------------------------------- 1: {HALF, RENDER} is pt_render_adaptive
@pytest.mark.parametrize("W,H", SIZES)
def test_half_render_equals_old_entry_and_replay(api, oracle, cb_spec, cb_oracle_scene, W, H):
    snaps = oracle_snapshots(oracle, cb_oracle_scene, cb_spec, W, H, MIN_SPP, MAX_SPP, ("cb", W, H))
    thr, ref = pick(snaps, W, H, MIN_SPP, MAX_SPP, AV.HALF, 0)
    old_ref = R.replay(snaps, W, H, MIN_SPP, MAX_SPP, thr)
    assert np.array_equal(ref["spp"], old_ref["spp"]) and same_bits(ref["err"], old_ref["err"])
    new, old = scene(api, cb_spec, W, H, 0), scene(api, cb_spec, W, H, 0)
    res = new.render_adaptive(MIN_SPP, MAX_SPP, float(thr), metric="half", path="render")
    res_old = old.render_adaptive(MIN_SPP, MAX_SPP, float(thr))
    check(new, res, ref, "half/render %dx%d" % (W, H), lanes=3)
    assert res == res_old
    assert same_bits(new.read_colors(), old.read_colors()) and np.array_equal(new.read_rnds(), old.read_rnds())
    (s1, e1), (s2, e2) = new.tile_state(), old.tile_state()
    assert np.array_equal(s1, s2) and same_bits(e1, e2)
    assert np.array_equal(new.sample_counts(), old.sample_counts()) and new.stat("samples") == old.stat("samples")
    assert np.array_equal(new.debug_adaptive_list(), old.debug_adaptive_list())
    new.close()
    old.close()


# ---------------------------------------------------------------------------- 2: the variance metric on the megakernel
@pytest.mark.parametrize("tonemapped", [0, 1])
@pytest.mark.parametrize("W,H", SIZES)
def test_variance_render_against_oracle_replay(api, oracle, cb_spec, cb_oracle_scene, W, H, tonemapped):
    snaps = oracle_snapshots(oracle, cb_oracle_scene, cb_spec, W, H, MIN_SPP, MAX_SPP, ("cb", W, H))
    thr, ref = pick(snaps, W, H, MIN_SPP, MAX_SPP, AV.VARIANCE, tonemapped)
    sc = scene(api, cb_spec, W, H, 1)
    res = sc.render_adaptive(MIN_SPP, MAX_SPP, float(thr), metric="variance", path="render", tonemapped=tonemapped)
    check(sc, res, ref, "variance/render %dx%d tonemapped %d" % (W, H, tonemapped))
    assert same_bits(sc.read_variance().reshape(-1), V.variance(sc.read_colors(), ref["pixel_spp"]))
    final = np.nonzero(ref["spp"] == MAX_SPP)[0]
    assert np.array_equal(sc.debug_adaptive_list(), final.astype(np.int32))
    sc.close()


# ---------------------------------------------------------------------------- 3: the tiled NEE kernel, tied to the oracle through BSDF
@pytest.mark.parametrize("W,H", SIZES)
def test_nee_bsdf_equals_render_path(api, oracle, cb_spec, cb_oracle_scene, W, H):
    snaps = oracle_snapshots(oracle, cb_oracle_scene, cb_spec, W, H, MIN_SPP, MAX_SPP, ("cb", W, H))
    thr, ref = pick(snaps, W, H, MIN_SPP, MAX_SPP, AV.VARIANCE, 1)
    nee, ren = scene(api, cb_spec, W, H, 1), scene(api, cb_spec, W, H, 1)
    res = nee.render_adaptive(MIN_SPP, MAX_SPP, float(thr), metric="variance", path="nee", strategy="bsdf")
    res_r = ren.render_adaptive(MIN_SPP, MAX_SPP, float(thr), metric="variance", path="render")
    check(nee, res, ref, "variance/nee-bsdf %dx%d" % (W, H))
    assert res == res_r
    assert same_bits(nee.read_colors(), ren.read_colors()) and np.array_equal(nee.read_rnds(), ren.read_rnds())
    (s1, e1), (s2, e2) = nee.tile_state(), ren.tile_state()
    assert np.array_equal(s1, s2) and same_bits(e1, e2)
    nee.close()
    ren.close()


# ---------------------------------------------------------------------------- 4: the NEE path with MIS, without and with a map
def small_sky():
    from opencl_path_tracer_amd import scenes
    return scenes.sun_and_sky(width=16, height=8)


@pytest.mark.parametrize("with_env", [False, True])
@pytest.mark.parametrize("metric", ["variance", "half"])
@pytest.mark.parametrize("W,H", SIZES)
def test_nee_mis_against_uniform_nee_replay(api, cb_spec, W, H, metric, with_env):
    env = small_sky() if with_env else None
    snaps = nee_snapshots(api, cb_spec, W, H, MIN_SPP, MAX_SPP, "mis", env, ("cb", W, H))
    code = AV.VARIANCE if metric == "variance" else AV.HALF
    thr, ref = pick(snaps, W, H, MIN_SPP, MAX_SPP, code, 1)
    sc = scene(api, cb_spec, W, H, 1, env=env)
    res = sc.render_adaptive(MIN_SPP, MAX_SPP, float(thr), metric=metric, path="nee", strategy="mis")
    check(sc, res, ref, "%s/nee-mis %dx%d env %d" % (metric, W, H, with_env), rays=True)
    sc.close()


# ---------------------------------------------------------------------------- 5: every node mode's instance of the tiled kernel
@pytest.mark.parametrize("which,opts,mode", [
    ("mesh", {"lds_scene": 0, "wide_nodes": 2}, 3),                       # 4-wide nodes from global memory
    ("mesh", {"lds_scene": 2, "wide_nodes": 1, "treelet": -1}, 2),        # the BVH2 treelet
    ("cornell", {}, 0),                                                   # the whole tree in LDS (the default there)
    ("cornell", {"lds_scene": 0, "wide_nodes": 1}, 1),                    # BVH2 from global memory
])
def test_nee_mis_node_modes(api, cb_spec, which, opts, mode):
    from opencl_path_tracer_amd import scenes
    if which == "mesh":
        W, H, lo, hi = 64, 48, 4, 32
        spec = scenes.displaced_grid_mesh(20000)
    else:
        W, H, lo, hi = 96, 64, MIN_SPP, MAX_SPP
        spec = cb_spec
    snaps = nee_snapshots(api, spec, W, H, lo, hi, "mis", None, (which, W, H))
    thr, ref = pick(snaps, W, H, lo, hi, AV.VARIANCE, 1)
    pre = {k: v for k, v in opts.items() if k != "lds_scene" or which == "mesh"}
    sc = api.Scene(W, H)
    for k, v in pre.items():
        sc.set_option(k, v)
    sc.load(spec)
    if which != "mesh" and "lds_scene" in opts:
        sc.set_option("lds_scene", opts["lds_scene"])
    sc.set_option("moments", 1)
    sc.iterations = BOUNCES
    res = sc.render_adaptive(lo, hi, float(thr), metric="variance", path="nee", strategy="mis")
    assert sc.stat("node_mode") == mode
    check(sc, res, ref, "%s %s" % (which, opts), rays=True)
    sc.close()


# ---------------------------------------------------------------------------- 6: refusals and the held frame
def test_refusals_and_held_frame(api, cb_spec):
    W, H = 64, 40
    sc = scene(api, cb_spec, W, H, 0)
    sc.iterations = 4

    def refused(call):
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_EINVAL
        return str(e.value)

    for path in ("render", "nee"):                          # the variance metric needs option moments
        assert "moments" in refused(lambda: sc.render_adaptive(4, 16, 0.1, metric="variance", path=path))
    assert sc.current_sample == 0 and np.all(sc.sample_counts() == 0)
    sc.set_environment(small_sky())                         # the megakernel path does not draw a map
    for metric in ("half", "variance"):
        assert "pt_render_nee" in refused(lambda: sc.render_adaptive(4, 16, 0.1, metric=metric, path="render"))
    sc.clear_environment()
    sc.render_adaptive(4, 16, 0.1, metric="half", path="render")
    held = sc.read_colors().copy()
    for call in (lambda: sc.render(1), sc.trace_rays, lambda: sc.render_nee(1), lambda: sc.render_adaptive(4, 16, 0.1),
                 lambda: sc.render_adaptive(4, 16, 0.1, metric="half", path="nee")):
        refused(call)
    assert same_bits(sc.read_colors(), held)
    sc.current_sample = 0
    sc.set_option("moments", 1)
    sc.render_adaptive(4, 16, 0.05, metric="variance", path="nee", strategy="mis")
    assert np.all(sc.sample_counts() >= 4) and np.all(np.isfinite(sc.tile_state()[1]))
    assert sc.read_variance().shape == (H, W)
    for call in (lambda: sc.render(1), lambda: sc.render_nee(1), lambda: sc.render_adaptive(4, 16, 0.1, metric="variance")):
        refused(call)
    sc.current_sample = 0
    sc.render(2)
    assert sc.current_sample == 2 and np.all(sc.sample_counts() == 2)
    sc.current_sample = 0
    sc.render_nee(2)
    assert sc.current_sample == 2
    sc.current_sample = 0
    sc.render_adaptive(4, 16, 0.1)
    assert sc.current_sample in (4, 8, 16)
    sc.close()


def test_threshold_zero_and_inf_on_the_nee_path(api, cb_spec):
    """GPU against GPU: threshold 0 retires nothing (= render_nee(max)), +inf every tile at min_spp (= render_nee(min))."""
    W, H = 100, 70
    for thr, spp in ((0.0, 32), (float("inf"), 4)):
        ad, un = scene(api, cb_spec, W, H, 1), scene(api, cb_spec, W, H, 1)
        res = ad.render_adaptive(4, 32, thr, metric="variance", path="nee", strategy="mis")
        un.render_nee(spp, "mis")
        assert same_bits(ad.read_colors(), un.read_colors()) and np.array_equal(ad.read_rnds(), un.read_rnds()), thr
        ra, ru = ad.read_rays(), un.read_rays()
        assert same_bits(ra["P"], ru["P"]) and same_bits(ra["D"], ru["D"])
        assert ad.current_sample == spp and np.all(ad.sample_counts() == spp) and res["samples"] == W * H * spp
        assert res["rounds"] == ([2, 4, 8, 16, 32] if thr == 0.0 else [2, 4])
        ad.close()
        un.close()
