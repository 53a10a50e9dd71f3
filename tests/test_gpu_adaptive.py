"""-m gpu: adaptive frames (pt_render_adaptive) against a CPU replay of the oracle, bit for bit.

The oracle renders the frame uniformly to every round boundary; tests/adaptive_ref.py replays the tile decisions on those
snapshots in float32.  A pixel that stopped after k samples must then hold the oracle's colour and LCG state after k samples,
and the tile counts, the tile errors (bits) and the samples statistic must be the replay's."""
import numpy as np
import pytest

import adaptive_ref as R

pytestmark = pytest.mark.gpu

MIN_SPP, MAX_SPP, BOUNCES = 4, 64, 8
_SNAPS = {}


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def oracle_snapshots(oracle, osc, spec, W, H, bounces, min_spp, max_spp, key):
    """Colours and rnds of the oracle's uniform render at every boundary (copies: colors() / rnds() view live buffers)."""
    if key in _SNAPS:
        return _SNAPS[key]
    cam = oracle.make_camera(spec.fov, spec.yaw, spec.pitch, spec.shift, W, H)
    fr = oracle.OracleFrame(W, H)
    snaps, prev = {}, 0
    for b in R.rounds(min_spp, max_spp):
        fr.render(osc, cam, bounces, prev, b - prev, nthreads=16)
        snaps[b] = (fr.colors().copy(), fr.rnds().copy())
        prev = b
    _SNAPS[key] = snaps
    return snaps


def pick_replay(snaps, W, H, min_spp, max_spp):
    """A threshold taken from the oracle's own tile errors at the first decision, such that the counts take >= 3 values."""
    b = R.rounds(min_spp, max_spp)
    e1 = R.tile_errors(snaps[b[1]][0], snaps[b[0]][0], W, H)
    for q in (0.5, 0.6, 0.4, 0.75, 0.3):
        thr = np.float32(np.quantile(e1[np.isfinite(e1)], q))
        ref = R.replay(snaps, W, H, min_spp, max_spp, thr)
        if len(set(ref["spp"].tolist())) >= 3:
            return thr, ref
    raise AssertionError("no threshold gives >= 3 distinct tile counts: the replay would be vacuous")


def check_against_replay(sc, ref, thr, min_spp, max_spp, what):
    res = sc.render_adaptive(min_spp, max_spp, float(thr))
    spp, err = sc.tile_state()
    assert np.array_equal(spp, ref["spp"]), "%s: tile counts differ" % what
    assert same_bits(err, ref["err"]), "%s: tile errors differ in bits" % what
    assert np.array_equal(sc.sample_counts().reshape(-1), ref["pixel_spp"]), what
    cols, rnds = sc.read_colors(), sc.read_rnds()
    assert int((rnds != ref["rnds"]).sum()) == 0, "%s: %d pixels consumed a different number of draws" % (what, int((rnds != ref["rnds"]).sum()))
    assert same_bits(cols[:, :3], ref["colors"][:, :3]), "%s: colours differ in bits" % what
    assert sc.stat("samples") == int(ref["pixel_spp"].sum(dtype=np.int64)), what
    assert sc.current_sample == int(ref["spp"].max())
    assert res["rounds"] == ref["rounds"] and res["active_tiles"] == ref["active_tiles"], (what, res, ref["rounds"], ref["active_tiles"])
    assert res["samples"] == int(ref["pixel_spp"].sum(dtype=np.int64))
    return res


@pytest.mark.parametrize("W,H", [(96, 64), (100, 70)])
def test_oracle_replay(api, oracle, cb_spec, cb_oracle_scene, W, H):
    snaps = oracle_snapshots(oracle, cb_oracle_scene, cb_spec, W, H, BOUNCES, MIN_SPP, MAX_SPP, ("cb", W, H))
    thr, ref = pick_replay(snaps, W, H, MIN_SPP, MAX_SPP)
    sc = api.Scene(W, H).load(cb_spec)
    sc.iterations = BOUNCES
    res = check_against_replay(sc, ref, thr, MIN_SPP, MAX_SPP, "cornell %dx%d" % (W, H))
    assert res["active_tiles"][-1] < res["active_tiles"][0]
    sc.close()


@pytest.mark.parametrize("opts", [
    {"schedule": 0}, {"schedule": 1}, {"schedule": 2},
    {"schedule": 0, "chunk_spp": 8, "chunk_taper": 2}, {"schedule": 1, "chunk_spp": 8, "chunk_taper": 2},
    {"schedule": 2, "chunk_spp": 8, "chunk_taper": 2}, {"persistent": 0}, {"count_work": 1},
])
def test_oracle_replay_forced_launch_shapes(api, oracle, cb_spec, cb_oracle_scene, opts):
    """The tile indirection in every code path that reads it: each schedule, chained and tapered passes, one wave per tile."""
    W, H = 100, 70
    snaps = oracle_snapshots(oracle, cb_oracle_scene, cb_spec, W, H, BOUNCES, MIN_SPP, MAX_SPP, ("cb", W, H))
    thr, ref = pick_replay(snaps, W, H, MIN_SPP, MAX_SPP)
    sc = api.Scene(W, H).load(cb_spec)
    for k, v in opts.items():
        sc.set_option(k, v)
    sc.iterations = BOUNCES
    check_against_replay(sc, ref, thr, MIN_SPP, MAX_SPP, "options %s" % opts)
    sc.close()


@pytest.mark.parametrize("lds,wide", [(0, 2), (2, 1)])
def test_oracle_replay_mesh(api, oracle, lds, wide):
    """The displaced-grid mesh scene (the triangles its OBJ form holds) with 4-wide nodes from global memory or the BVH2 treelet."""
    from opencl_path_tracer_amd import scenes
    W, H, lo, hi = 64, 48, 4, 32
    spec = scenes.displaced_grid_mesh(20000)
    osc = oracle.load_scene(spec)
    snaps = oracle_snapshots(oracle, osc, spec, W, H, BOUNCES, lo, hi, ("mesh", W, H))
    thr, ref = pick_replay(snaps, W, H, lo, hi)
    sc = api.Scene(W, H)
    sc.set_option("lds_scene", lds)
    sc.set_option("wide_nodes", wide)
    if lds:
        sc.set_option("treelet", -1)
    sc.load(spec)
    sc.iterations = BOUNCES
    check_against_replay(sc, ref, thr, lo, hi, "mesh lds_scene %d wide_nodes %d" % (lds, wide))
    sc.close()


def test_full_size_threshold_zero_and_inf(api, cb_spec):
    """1080p, GPU against GPU: threshold 0 retires nothing (= render(256)); +inf retires every tile at min_spp (= render(16))."""
    W, H = 1920, 1080
    n_tiles = ((W + 7) // 8) * ((H + 7) // 8)
    for thr, spp in ((0.0, 256), (float("inf"), 16)):
        ad = api.Scene(W, H).load(cb_spec)
        ad.iterations = BOUNCES
        res = ad.render_adaptive(16, 256, thr)
        un = api.Scene(W, H).load(cb_spec)
        un.iterations = BOUNCES
        un.render(spp)
        assert np.array_equal(ad.read_rnds(), un.read_rnds()), "threshold %g" % thr
        assert same_bits(ad.read_colors()[:, :3], un.read_colors()[:, :3]), "threshold %g" % thr
        assert ad.current_sample == spp and np.all(ad.sample_counts() == spp)
        assert res["samples"] == W * H * spp and ad.stat("samples") == un.stat("samples")
        if thr == 0.0:
            assert res["active_tiles"] == [n_tiles] * 6 and res["rounds"] == [8, 16, 32, 64, 128, 256]
        else:
            assert res["rounds"] == [8, 16] and np.all(np.isfinite(ad.tile_state()[1]))
        ad.close()
        un.close()


def test_frame_state_rules(api, cb_spec):
    W, H = 64, 40
    sc = api.Scene(W, H).load(cb_spec)
    sc.iterations = 4
    assert np.all(sc.sample_counts() == 0)
    sc.render(2)
    assert np.all(sc.sample_counts() == 2) and np.all(sc.tile_state()[0] == 2) and np.all(np.isinf(sc.tile_state()[1]))
    with pytest.raises(api.PtError) as e:
        sc.render_adaptive(4, 16, 0.1)                   # starts a frame: current_sample must be 0
    assert e.value.code == api.PT_EINVAL
    sc.current_sample = 0
    sc.render_adaptive(4, 16, 0.1)
    for call in (lambda: sc.render(1), sc.trace_rays, lambda: sc.render_adaptive(4, 16, 0.1)):
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_EINVAL
    sc.current_sample = 0
    sc.render(2)
    assert sc.current_sample == 2 and np.all(sc.sample_counts() == 2)
    sc.close()


def test_scope(api, cb_spec):
    """The wavefront variant and tiled contexts of more than one rank refuse."""
    sc = api.Scene(64, 40).load(cb_spec)
    sc.set_option("variant", 1)
    with pytest.raises(api.PtError) as e:
        sc.render_adaptive(4, 16, 0.1)
    assert e.value.code == api.PT_EINVAL
    sc.close()
    rk = api.Scene(64, 40, rank=0, world=2).load(cb_spec)
    with pytest.raises(api.PtError) as e:
        rk.render_adaptive(4, 16, 0.1)
    assert e.value.code == api.PT_EINVAL
    rk.close()


def test_compaction_over_several_chunks(api, cb_spec):
    """640x480 = 4,800 tiles: k_compact_tiles walks two chunks of 4,096 flags with a sparse set, so the running base carried from
    chunk to chunk decides where the second chunk's tiles land.  The GPU's own uniform render to every boundary (bit-identical to the
    oracle: test_gpu_parity) is replayed; the counts, errors, colours and the list itself -- ascending -- must be the replay's."""
    W, H, lo, hi = 640, 480, 4, 16
    n_tiles = (W // 8) * (H // 8)
    un = api.Scene(W, H).load(cb_spec)
    un.iterations = 4
    snaps, prev = {}, 0
    for b in R.rounds(lo, hi):
        un.render(b - prev)
        snaps[b] = (un.read_colors().copy(), un.read_rnds().copy())
        prev = b
    un.close()
    thr, ref = pick_replay(snaps, W, H, lo, hi)
    sc = api.Scene(W, H).load(cb_spec)
    sc.iterations = 4
    assert len(sc.debug_adaptive_list()) == 0
    check_against_replay(sc, ref, thr, lo, hi, "640x480")
    final = np.nonzero(ref["spp"] == hi)[0]                 # active after the last decision, in ascending frame-tile order
    retired0 = np.nonzero(ref["spp"][:4096] < hi)[0]
    assert len(retired0) > 0 and np.any(final >= 4096), "the replay does not exercise the carry between chunks"
    lst = sc.debug_adaptive_list()
    assert lst.dtype == np.int32 and np.array_equal(lst, final.astype(np.int32))
    assert n_tiles > 4096
    sc.close()
