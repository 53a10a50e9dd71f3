"""-m gpu: the real shade_hit (pt_device.hpp) on authored items, in waves of authored composition, through pt_debug_shade
(Scene.debug_shade): all four plain instances -- SK on or off, REC on or off -- against the oracle's iteration body (orc_shade_step_n, the
function trace_ray_item calls) and against each other, at eight iterations and in preview mode (iterations == 1).

Every comparison is on bit patterns over every item: a NaN compares equal to any NaN and nothing else is relaxed.  The items come from
tests/shade_inputs.py, whose guards (asserted here from the oracle's results, and without a device in tests/test_shade_host.py) say that
each list reaches the branch it is meant to reach.  The oracle's triangle_intersect gives each item's t, as closest_hit would; the items
of the grazing list whose dot(D, N) is exactly 0 have no hit in the reference (it divides by the dot product), so for them the device
gets t = 100 and the four instances are compared with each other only.  Each test prints its counts and the wall time of both sides
(-s shows them; profiles/shade/README.md records a run)."""
import time

import numpy as np
import pytest

import shade_inputs as SI
import spec_inputs as S
from test_gpu_spec_math import assert_same_bits

pytestmark = pytest.mark.gpu
FLOAT_COLS = [c for c in range(23) if c not in (6, 7)]        # every output word but the LCG state and the inside flag
INSTANCES = ((0, "shade_hit<false, false>"), (1, "shade_hit<true, false>"), (2, "shade_hit<false, true>"), (3, "shade_hit<true, true>"))


@pytest.fixture(scope="module")
def ctx(api):
    sc, packed_of = SI.load_scene(api, 0)
    yield sc, packed_of
    sc.close()


@pytest.fixture(scope="module")
def lists(oracle):
    t0 = time.perf_counter()
    L, out, meta = SI.build_all()
    print("[shade] oracle: %d items, both passes, %.3f s" % (sum(v.shape[0] for v in L.values()), time.perf_counter() - t0))
    SI.check_guards(SI.guards())
    return L, out


@pytest.mark.timeout(60, method="thread")
def test_the_contexts_agree_on_the_scene(api, ctx):
    sc, packed_of = ctx
    assert sc.camera.tobytes() == SI.camera().tobytes()
    tris, mats, _ = sc.debug_scene()
    assert tris.tobytes() == SI.triangles().tobytes() and mats.tobytes() == SI.materials().tobytes()
    packets = sc.debug_bvh()[1]
    assert np.array_equal(S.bits(packets[packed_of, 9:12]), S.bits(SI.triangles()["N"][:, :3]))     # the packed normal is the record's
    assert sc.debug_launch_plan(1)["node_mode"] == 0                                                 # tree in LDS: shading records exist


@pytest.mark.timeout(60, method="thread")
@pytest.mark.parametrize("name", ["incidence", "grazing", "tir", "coin", "state", "lobe", "waves", "window"])
def test_all_four_instances_equal_the_oracle_and_each_other(api, ctx, lists, name):
    sc, packed_of = ctx
    L, out = lists
    it = L[name]
    for iterations, want in ((8, out[name][0]), (1, out[name][1])):
        hit = S.fl(want[:, 0]) > 0
        dev = SI.device_items(it, want, packed_of)
        dev[~hit, 6] = S.bits(np.float32(100.0))[0]
        assert (~hit).sum() == 0 or name == "grazing"
        got = {}
        t0 = time.perf_counter()
        for inst, label in INSTANCES:
            got[inst] = sc.debug_shade(inst, dev, iterations=iterations)
        dt = time.perf_counter() - t0
        print("[shade] %-10s iterations %d: %5d items (%d without a hit in the reference), four device instances %.4f s" % (name, iterations, it.shape[0],
                                                                                                                 int((~hit).sum()), dt))
        for inst, label in INSTANCES:
            assert_same_bits("%s, %s, iterations %d" % (label, name, iterations), dev[hit], got[inst][hit], want[hit, 1:], float_cols=FLOAT_COLS)
        for inst, label in INSTANCES[1:]:
            assert_same_bits("%s against %s, %s, iterations %d" % (label, INSTANCES[0][1], name, iterations), dev, got[inst], got[0], float_cols=FLOAT_COLS,
                             other=INSTANCES[0][1])


@pytest.mark.timeout(60, method="thread")
def test_a_last_wave_that_the_items_do_not_fill(api, ctx, lists):
    # 37 items of the mixed-window waves: the lanes past n leave before any vote, so the results are those of the full list's first items
    sc, packed_of = ctx
    L, out = lists
    it, want = L["window"][256:256 + 37], out["window"][0][256:256 + 37]
    dev = SI.device_items(it, want, packed_of)
    for inst, label in INSTANCES:
        assert_same_bits(label + ", 37 items", dev, sc.debug_shade(inst, dev, iterations=8), want[:, 1:], float_cols=FLOAT_COLS)


@pytest.mark.timeout(60, method="thread")
def test_rec_is_refused_without_shading_records(api, lists):
    # with the tree read from global memory no launch of the context carries shading records: REC is an error, the others still run
    sc, packed_of = SI.load_scene(api, 0)
    sc.set_option("lds_scene", 0)
    L, out = lists
    it, want = L["incidence"][:64], out["incidence"][0][:64]
    dev = SI.device_items(it, want, packed_of)
    for inst in (api.PT_SHADE_REC, api.PT_SHADE_REC | api.PT_SHADE_SK):
        with pytest.raises(api.PtError) as e:
            sc.debug_shade(inst, dev, iterations=8)
        assert e.value.code == api.PT_EINVAL
    assert_same_bits("shade_hit<false, false> without records", dev, sc.debug_shade(0, dev, iterations=8), want[:, 1:], float_cols=FLOAT_COLS)
    bad = dev.copy()
    bad[5, 7] = packed_of.size
    with pytest.raises(api.PtError) as e:                                                          # an index past the packed triangles: an error code
        sc.debug_shade(0, bad, iterations=8)
    assert e.value.code == api.PT_EINVAL
    sc.close()
