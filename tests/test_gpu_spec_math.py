"""-m gpu: the device's spec math and sampling primitives (pt_device.hpp: spec_sincos, spec_pow, spec_pow5, lcg_rand, diffuse_direction,
diffuse_direction_rec, fresnel) against their unit-level counterparts in the CPU oracle, through pt_debug_spec (Scene.debug_spec), and
the LCG's hand-reduced path against the 64-bit remainder on every non-negative seed (pt_debug_math, PT_MATH_LCG).

Every comparison is on bit patterns; a NaN compares equal to any NaN and nothing else is relaxed.  The inputs come from
tests/spec_inputs.py, whose guards (asserted here from the oracle's results, and without a device in tests/test_spec_host.py) say that
each list reaches the branches it is meant to reach.  Each test prints its input counts and the wall time of both sides (-s shows
them; profiles/spec/README.md records a run)."""
import time

import numpy as np
import pytest

import spec_inputs as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sc(api):
    return api.Scene(8, 8, device=0)


def timed(label, fn, *args):
    t0 = time.monotonic()
    r = fn(*args)
    print("[spec] %-34s %8.3f s" % (label, time.monotonic() - t0))
    return r


def hexrow(a):
    return " ".join("%08x" % int(v) for v in np.atleast_1d(a))


def assert_same_bits(what, inputs, got, want, float_cols=None, other="oracle"):
    """got and want as (n, k) 32-bit words; columns float_cols (default: all) hold floats, where NaN matches NaN"""
    n = len(inputs)
    inputs = np.ascontiguousarray(inputs).view(np.uint32).reshape(n, -1)
    got = np.ascontiguousarray(got).view(np.uint32).reshape(n, -1)
    want = np.ascontiguousarray(want).view(np.uint32).reshape(n, -1)
    assert got.shape == want.shape
    cols = list(range(got.shape[1])) if float_cols is None else list(float_cols)
    both_nan = np.zeros(got.shape, dtype=bool)
    both_nan[:, cols] = np.isnan(got[:, cols].view(np.float32)) & np.isnan(want[:, cols].view(np.float32))
    bad = ((got != want) & ~both_nan).any(axis=1)
    if bad.any():
        first = np.flatnonzero(bad)[:6]
        lines = ["item %d (lane %d of wave %d): in %s -> device %s, %s %s" % (i, i % 64, i // 64, hexrow(inputs[i]), hexrow(got[i]), other, hexrow(want[i]))
                 for i in first]
        raise AssertionError("%s: %d of %d items differ\n%s" % (what, int(bad.sum()), n, "\n".join(lines)))


# ------------------------------------------------------------------------------------------------ sine and cosine
@pytest.mark.timeout(60, method="thread")
def test_sincos_both_instances_equal_the_oracle(api, oracle, sc):
    th = S.sincos_inputs()
    assert th.min() >= 0.0 and th.max() <= 8.0                       # the oracle's domain
    q = S.sincos_quadrants(th)
    counts = [int((q == k).sum()) for k in range(4)]
    print("[spec] sincos inputs %d, q & 3 = 0..3: %s" % (th.size, counts))
    assert min(counts) >= 100000, counts
    s, c = timed("oracle sincos", oracle.spec_sincosf_n, th)
    want = np.stack([s, c], axis=1)
    plain = timed("device spec_sincos<false>", sc.debug_spec, api.PT_SPEC_SINCOS, th)
    pinned = timed("device spec_sincos<true>", sc.debug_spec, api.PT_SPEC_SINCOS_SK, th)
    assert_same_bits("spec_sincos<false>", th, plain, want)
    assert_same_bits("spec_sincos<true>", th, pinned, want)
    assert_same_bits("spec_sincos<true> against <false>", th, pinned, plain, other="spec_sincos<false>")


# ------------------------------------------------------------------------------------------------ pow
@pytest.mark.timeout(60, method="thread")
def test_pow_both_instances_equal_the_oracle(api, oracle, sc):
    x, y = S.pow_inputs()
    items = np.stack([x, y], axis=1)
    want = timed("oracle pow", oracle.spec_powf_n, x, y)
    guards = S.pow_guards(x, y, want)
    print("[spec] pow pairs %d (%d x values, %d y values, %d threshold pairs): %s" % (x.size, S.pow_x_list().size, len(S.POW_Y),
                                                                                   S.pow_threshold_pairs()[0].size, guards))
    for k, least in S.POW_GUARD_MIN.items():
        assert guards[k] >= least, (k, guards)
    plain = timed("device spec_pow<false>", sc.debug_spec, api.PT_SPEC_POW, items)
    pinned = timed("device spec_pow<true>", sc.debug_spec, api.PT_SPEC_POW_SK, items)
    assert_same_bits("spec_pow<false>", items, plain, want)
    assert_same_bits("spec_pow<true>", items, pinned, want)
    assert_same_bits("spec_pow<true> against <false>", items, pinned, plain, other="spec_pow<false>")


# ------------------------------------------------------------------------------------------------ pow5 and fresnel
@pytest.mark.timeout(60, method="thread")
def test_pow5_equals_the_oracle(api, oracle, sc):
    x = S.pow5_inputs()
    print("[spec] pow5 inputs %d" % x.size)
    want = timed("oracle pow5", oracle.spec_pow5_n, x)
    got = timed("device spec_pow5", sc.debug_spec, api.PT_SPEC_POW5, x)
    assert_same_bits("spec_pow5", x, got, want)


@pytest.mark.timeout(60, method="thread")
def test_fresnel_equals_the_oracle(api, oracle, sc):
    items, masks = S.fresnel_inputs()
    assert items.shape == (65536, 9)
    want = timed("oracle fresnel", oracle.fresnel_n, items)
    guards = S.fresnel_guards(items, masks, want)
    print("[spec] fresnel items %d: %s" % (items.shape[0], guards))
    for k, least in S.FRESNEL_GUARD_MIN.items():
        assert guards[k] >= least, (k, guards)
    got = timed("device fresnel", sc.debug_spec, api.PT_SPEC_FRESNEL, items)
    assert_same_bits("fresnel", items, got, want)


# ------------------------------------------------------------------------------------------------ LCG
@pytest.mark.timeout(60, method="thread")
def test_lcg_equals_the_oracle(api, oracle, sc):
    seeds = S.lcg_inputs()
    new, rnd = timed("oracle lcg", oracle.rand_n, seeds)
    print("[spec] lcg seeds %d, %d negative, %d with the float 1.0f, %d with the new seed 0" % (seeds.size, int((seeds < 0).sum()),
                                                                                            int((rnd == 1.0).sum()), int((new == 0).sum())))
    assert (seeds < 0).sum() >= 100000 and (seeds >= 0).sum() >= 100000
    assert (rnd == 1.0).any() and (new == 0).any() and (new[seeds == 0] == 0).all() and (new[seeds == S.LCG_M] == 0).all()
    want = np.stack([new.view(np.uint32), S.bits(rnd)], axis=1)
    got = timed("device lcg_rand", sc.debug_spec, api.PT_SPEC_LCG, seeds)
    assert_same_bits("lcg_rand", seeds, got, want, float_cols=[1])


@pytest.mark.timeout(120, method="thread")
def test_lcg_reduced_path_on_every_non_negative_seed(api, sc):
    # all 2^31 seeds >= 0: the Mersenne reduction against (uint64)seed * 48271 % 2147483647 written out in the kernel
    t0 = time.monotonic()
    miss, inside, bad = sc.debug_math(api.PT_MATH_LCG, 0, 1 << 31)
    dt = time.monotonic() - t0
    print("[spec] lcg enumeration of 2^31 seeds %.3f s" % dt)
    assert dt < 60.0, "enumeration took %.1f s, over its 60 s budget" % dt
    assert miss == 0, "%d mismatches, first (seed, new seed) bits: %s" % (miss, [tuple("%08x" % v for v in row) for row in bad])
    assert inside == 1 << 31


@pytest.mark.timeout(60, method="thread")
def test_lcg_enumeration_covers_negative_seeds_too(api, sc):
    # The first and the last 2^20 negative seeds: none of them counts as inside the reduced path's window.  For a negative seed the
    # kernel's reference is the same 64-bit multiply and remainder as lcg_rand's generic path, so miss == 0 says little here; what holds
    # the generic path to an independent statement is test_lcg_equals_the_oracle, half of whose seeds are negative.
    for first in (1 << 31, (1 << 32) - (1 << 20)):
        miss, inside, bad = sc.debug_math(api.PT_MATH_LCG, first, 1 << 20)
        assert miss == 0 and inside == 0, (first, miss, inside, bad)


# ------------------------------------------------------------------------------------------------ cosine-lobe direction
@pytest.mark.timeout(60, method="thread")
def test_diffuse_direction_in_every_kind_of_wave(api, oracle, sc):
    normals = S.cornell_normals()
    items = S.diffuse_inputs(normals)
    count, lane0, lane63 = S.diffuse_wave_kinds(items)
    kinds = {int(k): int((count == k).sum()) for k in np.unique(count)}
    print("[spec] diffuse items %d in %d waves (%d Cornell normals); waves by lanes with rnd1 == 1.0f: %s" % (items.shape[0], (items.shape[0] + 63) // 64,
                                                                                                       normals.shape[0], kinds))
    assert kinds.get(0, 0) >= 1 and kinds.get(64, 0) >= 1                              # all inside the window, all outside
    # rnd1 alone decides every lane's vote (no normal puts the frame's l2 outside rsqrt_window), so the waves without a lane at 1.0f
    # do take the cores, in the plain functions as in the _REC ones
    assert np.array_equal(S.diffuse_in_window(items), S.bits(items[:, 6]) != S.ONE)
    for k in S.DIFFUSE_MIXED:                                                         # mixed: at lane 0, at lane 63, at neither end
        mixed = count == k
        assert (mixed & lane0).any() and (mixed & lane63).any() and (mixed & ~lane0).any() and (mixed & ~lane63).any(), k
    assert items.shape[0] % 64 != 0 and items.shape[0] > 256                          # a last wave the items do not fill; many blocks
    rnd = S.bits(items[:, 6:8])
    assert (rnd == S.bits(S.lcg_float(1))[0]).any(axis=0).all() and (rnd == S.ONE).any(axis=0).all()      # 2^-31 and 1.0f, in both draws
    pmax = np.abs(items[:, :3]).max(axis=1)
    assert (pmax == 0).any() and ((pmax > 100.0) & (pmax <= 500.0)).any() and (pmax > 5000.0).any()      # the offset's fma at three magnitudes
    want = timed("oracle new_ray_diffuse", oracle.new_ray_diffuse_n, items)
    got = {}
    for name in ("DIFFUSE", "DIFFUSE_SK", "DIFFUSE_REC", "DIFFUSE_REC_SK"):
        got[name] = timed("device " + name.lower(), sc.debug_spec, getattr(api, "PT_SPEC_" + name), items)
        assert_same_bits(name.lower(), items, got[name], want)
    assert_same_bits("diffuse_direction_rec<false> against diffuse_direction<false>", items, got["DIFFUSE_REC"], got["DIFFUSE"], other="plain")
    assert_same_bits("diffuse_direction_rec<true> against diffuse_direction<true>", items, got["DIFFUSE_REC_SK"], got["DIFFUSE_SK"], other="plain")
