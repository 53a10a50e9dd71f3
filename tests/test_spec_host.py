"""-m "not gpu": pt_debug_spec's argument checks on a host-only context, its place in the ABI, and the input lists of
tests/test_gpu_spec_math.py (tests/spec_inputs.py) counted against the oracle alone: the guards that say each list reaches the branches
it is meant to reach hold before any device is asked."""
import ctypes as C

import numpy as np
import pytest

import spec_inputs as S


def test_abi_has_the_entry_point(api):
    assert "pt_debug_spec" in api.EXPORTS and hasattr(api.LIB, "pt_debug_spec")
    assert sorted(api.SPEC_WORDS) == list(range(11)) and api.PT_SPEC_FRESNEL == 10 and api.PT_MATH_LCG == 5


def test_arguments_are_checked_before_the_device(api):
    sc = api.Scene(8, 8, device=None)
    one = np.zeros(16, dtype=np.uint32)
    call = lambda fn, n, a, b: api.LIB.pt_debug_spec(sc._h, fn, n, a, b)
    p = one.ctypes.data_as(C.c_void_p)
    for fn in (-1, 11, 1 << 20):
        assert call(fn, 1, p, p) == api.PT_EINVAL and call(fn, 0, p, p) == api.PT_EINVAL
    for fn in api.SPEC_WORDS:
        assert call(fn, -1, p, p) == api.PT_EINVAL
        assert call(fn, 1, None, p) == api.PT_EINVAL and call(fn, 1, p, None) == api.PT_EINVAL
        assert call(fn, 0, None, None) == api.PT_OK and call(fn, 0, p, p) == api.PT_OK            # n = 0 does nothing
        assert call(fn, 1, p, p) == api.PT_ENODEVICE                                               # a host-only context has no device
    assert api.LIB.pt_debug_spec(None, api.PT_SPEC_POW5, 1, p, p) == api.PT_EINVAL
    with pytest.raises(api.PtError) as e:
        sc.debug_spec(api.PT_SPEC_LCG, np.zeros(3, dtype=np.int32))
    assert e.value.code == api.PT_ENODEVICE
    assert sc.debug_spec(api.PT_SPEC_FRESNEL, np.zeros((0, 9), dtype=np.float32)).shape == (0, 3)
    with pytest.raises(api.PtError) as e:                                                          # PT_MATH_LCG is a known enumeration
        sc.debug_math(api.PT_MATH_LCG, 0, 1)
    assert e.value.code == api.PT_ENODEVICE
    sc.close()


def test_sincos_list_reaches_every_quadrant():
    th = S.sincos_inputs()
    assert th.size > 5000000 and th.min() == 0.0 and th.max() == 8.0 and not np.isnan(th).any()
    q = S.sincos_quadrants(th)
    assert min(int((q == k).sum()) for k in range(4)) >= 100000
    # rnd == 1.0f gives the angle just past 2 pi, in quadrant 4
    t = S.theta_of(S.lcg_float(S.LCG_ONE))
    assert float(t) > 2 * np.pi and np.floor(float(t) * 0.63661977236758138 + 0.5) == 4 and (S.bits(th) == S.bits(t)[0]).any()


def test_pow_list_reaches_every_branch(oracle):
    x, y = S.pow_inputs()
    assert x.size == y.size == S.pow_x_list().size * len(S.POW_Y) + 2 * 9 * 4096
    guards = S.pow_guards(x, y, oracle.spec_powf_n(x, y))
    for k, least in S.POW_GUARD_MIN.items():
        assert guards[k] >= least, (k, guards)
    # the threshold pairs straddle both thresholds: around -126 some results are +0 and some are not, around 128 likewise with +inf
    tx, ty = S.pow_threshold_pairs()
    out = S.bits(oracle.spec_powf_n(tx, ty)).reshape(2, 9, 4096)
    assert (out[0] == 0).any(axis=0).all() and (out[0] != 0).any(axis=0).all()
    assert (out[1] == 0x7f800000).any(axis=0).all() and (out[1] != 0x7f800000).any(axis=0).all()


def test_fresnel_list_reaches_every_class(oracle):
    items, masks = S.fresnel_inputs()
    assert items.shape == (65536, 9) and items[:, :3].min() >= 0.0 and items[:, :3].max() <= 1.0
    guards = S.fresnel_guards(items, masks, oracle.fresnel_n(items))
    for k, least in S.FRESNEL_GUARD_MIN.items():
        assert guards[k] >= least, (k, guards)


def test_lcg_list_holds_the_edges(oracle):
    seeds = S.lcg_inputs()
    assert seeds.dtype == np.int32 and seeds.size == (1 << 20) + 10 + 64 * 4096
    for v in (0, 1, 2, S.LCG_ONE, S.LCG_M, -1, -2, -(1 << 31), -(1 << 31) + 1, S.LCG_TO_ONE):
        assert (seeds == v).any(), v
    new, rnd = oracle.rand_n(seeds)
    assert np.array_equal(new.astype(np.int64), S.lcg_step(seeds))                # numpy's statement of the same recurrence
    assert new[seeds == S.LCG_TO_ONE][0] == S.LCG_ONE and rnd[seeds == S.LCG_TO_ONE][0] == 1.0
    chain = seeds[-64 * 4096:].reshape(64, 4096)
    assert np.array_equal(chain[1:], new[-64 * 4096:].reshape(64, 4096)[:-1])     # each iterate is fed back


def test_diffuse_list_has_every_kind_of_wave(oracle):
    normals = S.cornell_normals()
    assert normals.shape[0] >= 64 and np.array_equal(normals[:normals.shape[0] // 2], -normals[normals.shape[0] // 2:])
    items = S.diffuse_inputs(normals)
    count, lane0, lane63 = S.diffuse_wave_kinds(items)
    assert (count == 0).sum() >= 100 and (count == 64).sum() >= 10
    for k in S.DIFFUSE_MIXED:
        mixed = count == k
        assert (mixed & lane0).any() and (mixed & lane63).any() and (mixed & ~lane0).any() and (mixed & ~lane63).any(), k
    assert items.shape[0] % 64 != 0
    assert np.array_equal(S.diffuse_in_window(items), S.bits(items[:, 6]) != S.ONE)      # rnd1 alone decides each lane's vote
    # both sides of the frame's y-axis decision, from the normals at the threshold
    N = items[:, 3:6]
    yaxis = (np.abs(N[:, 0]) <= np.float32(0.001)) & (np.abs(N[:, 2]) <= np.float32(0.001))
    e = int(S.bits(np.float32(0.001))[0])
    at = lambda col, d: S.bits(np.abs(N[:, col])) == e + d
    assert (yaxis & at(0, 0) & at(2, 0)).any() and (~yaxis & at(0, 1)).any() and (~yaxis & at(2, 1)).any() and (yaxis & at(0, -1)).any()
    out = oracle.new_ray_diffuse_n(items)
    assert not np.isnan(out).any() and np.abs(np.linalg.norm(out[:, 4:7].astype(np.float64), axis=1) - 1).max() < 1e-6
