"""-m "not gpu": pt_debug_shade's argument checks on a host-only context and its place in the ABI; the item lists of
tests/test_gpu_shade_vertex.py (tests/shade_inputs.py) counted against the oracle alone -- the guards that say each list reaches the
branch it is meant to reach hold before any device is asked; and the oracle's iteration body (orc_shade_step_n, the function
trace_ray_item calls) held to a second reading: a float64 numpy evaluation of the mirror / glass vertex."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import shade_inputs as SI
import spec_inputs as S


def test_abi_has_the_entry_point(api, oracle):
    assert "pt_debug_shade" in api.EXPORTS and hasattr(api.LIB, "pt_debug_shade")
    assert (api.SHADE_WORDS_IN, api.SHADE_WORDS_OUT) == (25, 23) and (api.PT_SHADE_SK, api.PT_SHADE_REC) == (1, 2)
    assert (oracle.SHADE_WORDS_IN, oracle.SHADE_WORDS_OUT) == (25, 24)
    hdr = open(os.path.join(os.path.dirname(api.__file__), "..", "include", "pt_api.h")).read()
    assert "#define PT_SHADE_WORDS_IN 25" in hdr and "#define PT_SHADE_WORDS_OUT 23" in hdr


def test_the_window_constant_is_the_kernels(api):
    src = open(os.path.join(os.path.dirname(api.__file__), "csrc", "pt_device.hpp")).read()
    m = re.search(r"kSqrtWindowLo = (0x1p-?\d+)f", src)
    assert m and float.fromhex(m.group(1)) == SI.SQRT_WINDOW_LO
    assert "PT_DEV bool rsqrt_window(float x) { return x >= kSqrtWindowLo && x < __builtin_inff(); }" in src


def test_arguments_are_checked_before_the_device(api):
    sc, packed_of = SI.load_scene(api, None)
    n_tris = packed_of.size
    assert n_tris == SI.triangles().shape[0] and sorted(packed_of) == list(range(n_tris))
    it = np.zeros((2, 25), dtype=np.uint32)
    out = np.zeros((2, 23), dtype=np.uint32)
    cam = sc.camera.ctypes.data_as(C.c_void_p)
    p, q = it.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    call = lambda inst, n, a, b, c=cam: api.LIB.pt_debug_shade(sc._h, c, 8, inst, n, a, b)
    for inst in (-1, 4, 1 << 20):
        assert call(inst, 2, p, q) == api.PT_EINVAL and call(inst, 0, p, q) == api.PT_EINVAL
    for inst in range(4):
        assert call(inst, -1, p, q) == api.PT_EINVAL
        assert call(inst, 2, None, q) == api.PT_EINVAL and call(inst, 2, p, None) == api.PT_EINVAL
        assert call(inst, 2, p, q, None) == api.PT_EINVAL                                          # no camera
        assert call(inst, 0, None, None) == api.PT_OK and call(inst, 0, p, q) == api.PT_OK          # n = 0 does nothing
        for bad in (n_tris, -1, 1 << 30, -(1 << 31)):                                              # an index outside the packed triangles
            it[1, 7] = np.int64(bad).astype(np.uint32)
            assert call(inst, 2, p, q) == api.PT_EINVAL, bad
            assert call(inst, 1, p, q) == api.PT_ENODEVICE                                         # (item 0 alone is fine)
        it[1, 7] = n_tris - 1
        assert call(inst, 2, p, q) == api.PT_ENODEVICE                                             # a host-only context has no device
    assert api.LIB.pt_debug_shade(None, cam, 8, 0, 2, p, q) == api.PT_EINVAL
    with pytest.raises(api.PtError) as e:
        sc.debug_shade(api.PT_SHADE_REC, it)
    assert e.value.code == api.PT_ENODEVICE
    assert sc.debug_shade(0, np.zeros((0, 25), dtype=np.uint32)).shape == (0, 23)
    sc.close()
    fresh = api.Scene(SI.W, SI.H, device=None)                                                     # nothing uploaded
    assert api.LIB.pt_debug_shade(fresh._h, cam, 8, 0, 0, None, None) == api.PT_EINVAL
    fresh.close()


def test_scene_holds_what_the_lists_need():
    mats, tris = SI.materials(), SI.triangles()
    assert mats.shape[0] == 14 and sorted(np.unique(mats["type"])) == [0, 1, 2, 3, 7]
    assert set(np.unique(tris["mati"])) == set(range(14))                                           # every material has a triangle
    assert sorted(mats["shininess"][[SI.M_SH0, SI.M_SH1, SI.M_SHF, SI.M_SH200]]) == [0.0, 1.0, 2.5, 200.0]
    assert mats["n"][SI.M_GLASS1] == 1.0 and mats["n"][SI.M_GLASSLT1] < 1.0 and (mats["F0"][SI.M_GLASSF0] == 0).all()
    assert (mats["F0"][SI.M_MIRROR0] == 0).all() and (mats["F0"][SI.M_MIRROR1, :3] == 1).all() and (mats["ks"][SI.M_PLAIN] == 0).all()
    N = tris["N"][:, :3]
    assert ((np.abs(N[:, 0]) <= 0.001) & (np.abs(N[:, 2]) <= 0.001) & (N[:, 0] != 0)).any()        # the tangent frame's y-axis branch
    assert np.abs(np.linalg.norm(N.astype(np.float64), axis=1) - 1).max() < 1e-6


def test_every_list_reaches_its_branch():
    L, out, meta = SI.build_all()
    g = SI.guards()
    print("[shade] items per list: %s, %d in all" % ({k: v.shape[0] for k, v in L.items()}, sum(v.shape[0] for v in L.values())))
    print("[shade] guards: %s" % g)
    SI.check_guards(g)
    assert 2000 <= sum(v.shape[0] for v in L.values()) <= 20000 and all(v.shape[0] % 64 == 0 for v in L.values())


def test_preview_pass_differs_only_in_the_colour():
    L, out, meta = SI.build_all()
    for k, v in L.items():
        full, prev = out[k]
        hit = S.fl(full[:, 0]) > 0
        same = (full[:, :21] == prev[:, :21]) | (np.isnan(S.fl(full[:, :21])) & np.isnan(S.fl(prev[:, :21])))
        same[:, 7:9] = full[:, 7:9] == prev[:, 7:9]
        assert same.all(), k
        m = SI.materials()[SI.triangles()["mati"][v[:, 7]]]
        base = (m["kd"] + m["emission"])[:, :3]                                                     # prog.cl:323-325, then an emitter adds to it
        plain = hit & (m["type"] != 3)
        assert np.array_equal(S.fl(prev[plain, 21:24]), base[plain]), k
        assert np.array_equal(prev[~hit, 21:24], v[~hit, 22:25]), k                                 # a miss leaves the colour alone


def test_oracle_step_against_a_float64_reading_of_the_specular_vertex():
    """prog.cl:326-328, 219-245, 341-357 for the mirror and glass items of the incidence and state lists, in float64.

    Clear margins.  A decision is compared where its float64 operand is further from its threshold than float32 rounding can move it:
    |dot(D, N)| > 1e-5 for the flip (three roundings of terms <= 1: < 2e-7), |disc| > 1e-4 (disc is 1 - s2 / n^2 with 1 / n^2 <= 2.25:
    four roundings of terms <= 2.25, < 6e-7, and near TIR the critical-angle items have their own list), |rnd - prob| > 1e-5 (prob is a
    dozen roundings of terms <= 1: < 1e-6; rnd is exact).
    Direction bound 2e-5 per component.  Every float32 operation carries a relative error of 2^-24 = 6e-8.  The reflected direction
    D - 2 (N.D) N: five operations on terms <= 2, < 1e-6.  The refracted one D / n + (cosa / n - sqrt(disc)) N: terms <= 1.5; the
    square root multiplies disc's absolute error (< 6e-7) by 1 / (2 sqrt(disc)) <= 50 at disc = 1e-4 -- 3e-5 -- so the bound is applied
    where disc > 1e-2 (factor 5: 3e-6) and the rest only have their decision compared; the normalisation adds four more roundings and
    divides by a length >= 2/3.  Together under 1e-5; 2e-5 leaves a factor two.
    The new origin is hp +- 0.001 N with hp a point with coordinates under 512 (ulp 6e-5, three roundings): the offset along N from
    the float64 hit point must be +-0.001 within 4e-4, which tells the sides apart."""
    L, out, meta = SI.build_all()
    it = np.concatenate([L["incidence"], L["state"]])
    o = np.concatenate([out["incidence"][0], out["state"][0]])
    mats = SI.materials()[SI.triangles()["mati"][it[:, 7]]]
    sel = ((mats["type"] == 1) | (mats["type"] == 2)) & np.isfinite(S.fl(it[:, 0:6])).all(axis=1)
    total = int(sel.sum())
    it, o, mats = it[sel], o[sel], mats[sel]
    glass = mats["type"] == 2
    P, D = S.fl(it[:, 0:3]).astype(np.float64), S.fl(it[:, 3:6]).astype(np.float64)
    N = SI.normals(it[:, 7]).astype(np.float64)
    t = np.einsum("ij,ij->i", SI.triangles()["r1"][it[:, 7], :3].astype(np.float64) - P, N) / np.einsum("ij,ij->i", D, N)
    hp = P + t[:, None] * D
    dn = np.einsum("ij,ij->i", D, N)
    Nf = np.where((dn > 0)[:, None], -N, N)
    cosa = -np.einsum("ij,ij->i", D, Nf)
    n = np.where(it[:, 9] != 0, 1.0 / np.where(glass, mats["n"], 1.0).astype(np.float64), np.where(glass, mats["n"], 1.0).astype(np.float64))
    disc = 1.0 - (1.0 - cosa * cosa) / n / n
    F = mats["F0"][:, :3].astype(np.float64)
    F = F + (1.0 - F) * ((1.0 - np.abs(dn)) ** 5)[:, None]
    prob = F.sum(axis=1) / 3.0
    rnd = SI.draws(it[:, 8]).astype(np.float64)
    refr = glass & (disc > 0) & (rnd > prob)
    with np.errstate(invalid="ignore"):
        d_refr = D / n[:, None] + (cosa / n - np.sqrt(np.maximum(disc, 0)))[:, None] * Nf
    d_new = np.where(refr[:, None], d_refr, D - 2.0 * np.einsum("ij,ij->i", D, Nf)[:, None] * Nf)
    d_new /= np.linalg.norm(d_new, axis=1)[:, None]
    clear = (np.abs(dn) > 1e-5) & (~glass | ((np.abs(disc) > 1e-4) & (np.abs(rnd - prob) > 1e-5)))
    assert clear.sum() >= total // 2 and total >= 500, (int(clear.sum()), total)
    print("[shade] float64 reading: %d mirror / glass items, %d with clear margins, %d of them refract" % (total, int(clear.sum()), int((clear & refr).sum())))
    got_refr = o[:, 8] != it[:, 9]
    assert np.array_equal(got_refr[clear], refr[clear])                                             # TIR and the coin
    side = np.einsum("ij,ij->i", S.fl(o[:, 1:4]).astype(np.float64) - hp, Nf)
    want_side = np.where(refr, -0.001, 0.001)
    assert np.abs(side - want_side)[clear].max() < 4e-4                                             # the flip and the side stepped off to
    tight = clear & (~refr | (disc > 1e-2))
    assert tight.sum() >= total // 2
    err = np.abs(S.fl(o[:, 4:7]).astype(np.float64) - d_new)[tight].max()
    print("[shade] float64 reading: largest direction difference %.3g over %d items" % (err, int(tight.sum())))
    assert err < 2e-5
    assert (clear & refr).sum() >= 100 and (clear & glass & ~refr).sum() >= 50 and (clear & ~glass).sum() >= 100
