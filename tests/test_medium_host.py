"""The homogeneous medium of Scene.set_medium on host-only contexts (the record, its checks, the refusals of the other render paths,
SceneSpec.medium; include/pt_api.h) and the pieces of tests/medium_ref.py against closed forms: no device needed."""

import ctypes as C
import os

import numpy as np
import pytest

import medium_ref as M

# (the library is imported inside the tests, through conftest's `api` fixture: see tests/test_lens_host.py)

NEW_SYMBOLS = ["pt_medium_defaults", "pt_set_medium", "pt_clear_medium", "pt_get_medium", "pt_debug_medium"]
INF = float("inf")


def test_abi_has_the_new_symbols_and_the_record(api):
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTS and hasattr(api.LIB, name)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pt_api.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header
    assert "typedef struct pt_medium {" in header and "0x5bd1e995" in header
    assert C.sizeof(api.Medium) == 44
    assert [n for n, _ in api.Medium._fields_] == ["sigma_t", "albedo", "g", "lo", "hi"]
    m = api.Medium(7.0, (C.c_float * 3)(0.5, 0.5, 0.5), 0.3, (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1))
    api.LIB.pt_medium_defaults(C.byref(m))
    want = {"sigma_t": 0.0, "albedo": (1.0, 1.0, 1.0), "g": 0.0, "lo": (-INF, -INF, -INF), "hi": (INF, INF, INF)}
    assert m.as_dict() == want and api.medium_defaults() == want
    api.LIB.pt_medium_defaults(None)


def host_scene(api, spec=None):
    from opencl_path_tracer_amd import scenes
    sc = api.Scene(16, 16, device=None)
    spec = spec or scenes.cornell_box(8, 4)
    for m in spec.materials:
        sc.add_Material(*m)
    for verts, mati in spec.objects:
        sc.add_Triangles(api.triangles_from_vertices(verts, mati))
        sc.end_Obj()
    sc.upload_Triangles()
    sc.upload_Materials()
    return sc


def test_set_medium_checks_its_arguments(api):
    sc = host_scene(api)
    assert sc.medium() is None
    good = dict(sigma_t=0.25, albedo=(0.9, 0.8, 0.7), g=0.6, bounds=((-1, -2, -3), (4, 5, 6)))
    sc.set_medium(**good)
    held = sc.medium()
    f32 = lambda v: tuple(float(np.float32(x)) for x in v)
    assert held == {"sigma_t": 0.25, "albedo": f32(good["albedo"]), "g": float(np.float32(0.6)), "lo": (-1.0, -2.0, -3.0), "hi": (4.0, 5.0, 6.0)}
    nan = float("nan")
    bad = [(dict(sigma_t=nan), "sigma_t"), (dict(sigma_t=-0.5), "sigma_t"), (dict(sigma_t=INF), "sigma_t"),
           (dict(albedo=(0.5, nan, 0.5)), "albedo"), (dict(albedo=(1.5, 0.5, 0.5)), "albedo"), (dict(albedo=(0.5, 0.5, -0.1)), "albedo"),
           (dict(g=nan), "g"), (dict(g=0.995), "g"), (dict(g=-1.0), "g"),
           (dict(bounds=((0, 0, 0), (1, 0, 1))), "lo"), (dict(bounds=((0, 0, 2), (1, 1, 1))), "lo"), (dict(bounds=((nan, 0, 0), (1, 1, 1))), "lo"),
           (dict(bounds=((0, 0, 0), (1, nan, 1))), "lo"), (dict(bounds=((INF, 0, 0), (INF, 1, 1))), "lo")]
    for change, field in bad:
        with pytest.raises(api.PtError) as e:
            sc.set_medium(**dict(good, **change))
        assert e.value.code == api.PT_EINVAL and "pt_set_medium" in str(e.value) and field in str(e.value), change
        assert sc.medium() == held, change                  # a refused call leaves the held medium as it was
    m = api.Medium()
    api.LIB.pt_medium_defaults(C.byref(m))
    assert api.LIB.pt_set_medium(None, C.byref(m)) == api.PT_EINVAL and api.LIB.pt_set_medium(sc._h, None) == api.PT_EINVAL
    assert api.LIB.pt_clear_medium(None) == api.PT_EINVAL and api.LIB.pt_debug_medium(None, None, 0, None) == api.PT_EINVAL
    assert api.LIB.pt_get_medium(None, C.byref(m)) == api.PT_EINVAL and api.LIB.pt_get_medium(sc._h, None) == api.PT_EINVAL
    assert sc.medium() == held
    # the edges of the ranges; half-open and open boxes; the defaults themselves
    sc.set_medium(0.0)
    assert sc.medium()["sigma_t"] == 0.0
    sc.set_medium(3.0, albedo=(0, 1, 0), g=-0.99, bounds=((-INF, 0, -INF), (INF, 2, INF)))
    assert sc.medium()["lo"] == (-INF, 0.0, -INF) and sc.medium()["g"] == float(np.float32(-0.99))
    sc.set_medium(3.0, albedo=0.5, g=0.99)
    assert sc.medium()["albedo"] == (0.5, 0.5, 0.5) and sc.medium()["hi"] == (INF, INF, INF)
    sc.upload_Triangles()                                    # uploads keep the medium: it is not part of the scene
    sc.upload_Materials()
    assert sc.medium()["sigma_t"] == 3.0
    with pytest.raises(api.PtError) as e:                   # the debug kernel needs a device (and a medium)
        sc.debug_medium(np.zeros((1, 12), dtype=np.float32))
    assert e.value.code == api.PT_ENODEVICE
    sc.clear_medium()
    assert sc.medium() is None
    with pytest.raises(api.PtError) as e:
        sc.debug_medium(np.zeros((1, 12), dtype=np.float32))
    assert e.value.code == api.PT_EINVAL and "pt_set_medium" in str(e.value)


def test_refusals_come_before_the_device_check(api):
    sc = host_scene(api)
    sc.iterations = 4
    calls = (lambda: sc.render(1), lambda: sc.trace_rays(), lambda: sc.generate_rays(), lambda: sc.render_adaptive(2, 4, 0.1),
             lambda: sc.render_adaptive(2, 4, 0.1, path="render"))
    nee_calls = (lambda: sc.render_nee(1, "mis"), lambda: sc.render_nee(1, "light"), lambda: sc.render_nee(1, "bsdf"),
                 lambda: sc.render_adaptive(2, 4, 0.1, path="nee", metric="half", strategy="mis"),
                 lambda: sc.render_adaptive(2, 4, 0.1, path="nee", metric="half", strategy="bsdf"))

    def codes(cs):
        out = []
        for call in cs:
            with pytest.raises(api.PtError) as e:
                call()
            out.append((e.value.code, str(e.value)))
        return out
    before = codes(calls)
    assert all(c == api.PT_ENODEVICE for c, _ in before)
    sc.set_medium(0.01, albedo=0.9, g=0.6)
    for (code, text), name in zip(codes(calls), ("pt_render", "pt_trace_rays", "pt_generate_rays", "pt_render_adaptive", "pt_render_adaptive")):
        assert code == api.PT_EINVAL and "pt_clear_medium" in text and name in text
    assert all(c == api.PT_ENODEVICE for c, _ in codes(nee_calls))       # every NEE strategy renders the fog; the guides keep the clear view
    assert all(c == api.PT_ENODEVICE for c, _ in codes((lambda: sc.render_aovs(1, 4),)))
    sc.set_medium(0.0, albedo=0.9, g=0.6)                                # sigma_t = 0 is no medium
    assert codes(calls) == before
    sc.set_medium(0.01)
    assert codes(calls)[0][0] == api.PT_EINVAL
    sc.clear_medium()
    assert codes(calls) == before


def test_scene_spec_medium_round_trips_through_load(api):
    from opencl_path_tracer_amd import scenes
    assert scenes.cornell_box(8, 4).medium == {}
    assert api.Scene(16, 16, device=None).load(scenes.cornell_box(8, 4)).medium() is None
    spec = scenes.cornell_box(8, 4, fog=1e-3)
    held = api.Scene(16, 16, device=None).load(spec).medium()
    assert held["sigma_t"] == float(np.float32(1e-3)) and held["lo"] == scenes.CORNELL_ROOM[0] and held["hi"] == scenes.CORNELL_ROOM[1]
    walls = spec.objects[0][0].reshape(-1, 3)[6:-6]                        # the room's walls and ceiling (not the lamp, not the wide floor)
    assert np.array_equal(walls.min(axis=0), [-100.0, 0.0, -1000.0]) and np.array_equal(walls.max(axis=0), [1100.0, 1000.0, 1000.0])
    shaft = scenes.light_shaft()
    sc = api.Scene(16, 16, device=None).load(shaft)
    assert sc.medium()["sigma_t"] > 0 and np.isfinite(sc.medium()["lo"]).all() and np.isfinite(sc.medium()["hi"]).all()
    d = sc.debug_lights()
    assert len(d["cdf"]) == 1 and d["P_ana"] == 1.0                      # no emitter: the spot is the only light
    spec = scenes.cornell_box(8, 4)
    spec.medium = dict(sigma_t=0.5, albedo=(0.1, 0.2, 0.3), g=-0.25)
    held = api.Scene(16, 16, device=None).load(spec).medium()
    assert held["albedo"] == tuple(float(np.float32(v)) for v in (0.1, 0.2, 0.3)) and held["g"] == -0.25 and held["hi"] == (INF, INF, INF)


# ---------------------------------------------------------------------------- tests/medium_ref.py against closed forms
@pytest.mark.parametrize("g", [0.0, 0.6, -0.6, 0.99])
def test_hg_integrates_to_one_and_its_inverse_cdf_reproduces_the_cosine(g):
    # Gauss-Legendre over the cosine (the density does not depend on the azimuth: 2 pi of it), in panels that follow the forward peak
    x, w = np.polynomial.legendre.leggauss(64)
    edges = np.concatenate([[-1.0], 1.0 - np.geomspace(2.0, 1e-9, 60)[1:], [1.0]])
    total = 0.0
    for lo, hi in zip(edges[:-1], edges[1:]):
        c = 0.5 * (hi - lo) * x + 0.5 * (hi + lo)
        total += float((2.0 * np.pi * M.hg(g, c) * w).sum()) * 0.5 * (hi - lo)
    assert abs(total - 1.0) < 1e-10
    # the inverse cdf against the closed-form cdf, and its mean cosine g
    for u in (0.0, 1e-6, 0.1, 0.5, 0.9, 1.0 - 2.0 ** -24):
        c = M.hg_cos(g, u)
        assert -1.0 - 1e-12 <= c <= 1.0 + 1e-12
        # (the pinned isotropic branch 1 - 2 u1 runs from +1 down, the general one from -1 up: both are inverse cdfs of the density)
        assert abs(M.hg_cdf(g, c) - (1.0 - u if g == 0.0 else u)) < 1e-9, (g, u)
    assert M.hg_cos(g, 0.0) == pytest.approx(1.0 if g == 0.0 else -1.0, abs=1e-12)
    us = (np.arange(200000) + 0.5) / 200000
    assert abs(np.mean([M.hg_cos(g, u) for u in us[::20]]) - g) < 1e-3
    # the sampled direction is unit, has that cosine to D, and its p_b is HG of it
    D = np.array([0.36, -0.48, 0.8])
    for u1, u2 in ((0.1, 0.2), (0.7, 0.9), (0.5, 0.0)):
        wdir, pb, c = M.direction(g, D, u1, u2)
        assert abs(np.linalg.norm(wdir) - 1.0) < 1e-12 and abs(float(wdir @ D) - c) < 1e-9 and pb == M.hg(g, c)


def test_slab_clip_on_hand_made_rays():
    lo, hi = np.array([0.0, 0.0, 0.0]), np.array([2.0, 4.0, 6.0])
    inside = M.clip(lo, hi, [1.0, 1.0, 1.0], [0.0, 0.0, 1.0], 100.0)                    # starts inside: leaves through z = 6
    assert inside[:2] == (0.0, 5.0)
    assert M.clip(lo, hi, [1.0, 1.0, 1.0], [0.0, 0.0, 1.0], 3.0)[:2] == (0.0, 3.0)    # ... unless the hit comes first
    outside = M.clip(lo, hi, [1.0, 1.0, -2.0], [0.0, 0.0, 1.0], np.inf)                # starts outside: enters at z = 0
    assert outside[:2] == (2.0, 8.0)
    d = np.array([1.0, 2.0, 2.0]) / 3.0
    a, b, _ = M.clip(lo, hi, [-1.0, -2.0, -2.0], d, np.inf)                            # oblique, through the corner (0, 0, 0)
    assert a == pytest.approx(3.0) and b == pytest.approx(9.0)                         # leaves through x = 2 and y = 4 at (2, 4, 4)
    parallel_in = M.clip(lo, hi, [-5.0, 1.0, 1.0], [1.0, 0.0, 0.0], np.inf)            # parallel to four faces, between them
    assert parallel_in[:2] == (5.0, 7.0)
    parallel_out = M.clip(lo, hi, [-5.0, 4.5, 1.0], [1.0, 0.0, 0.0], np.inf)           # parallel and outside the y slab
    assert max(parallel_out[1] - parallel_out[0], 0.0) == 0.0
    miss = M.clip(lo, hi, [-1.0, 10.0, 1.0], [1.0, 0.0, 0.0], np.inf)
    assert max(miss[1] - miss[0], 0.0) == 0.0
    away = M.clip(lo, hi, [1.0, 1.0, 7.0], [0.0, 0.0, 1.0], np.inf)                    # behind the ray
    assert max(away[1] - away[0], 0.0) == 0.0
    short = M.clip(lo, hi, [1.0, 1.0, -2.0], [0.0, 0.0, 1.0], 1.5)                     # the hit comes before the box
    assert max(short[1] - short[0], 0.0) == 0.0
    everywhere = M.clip(np.full(3, -np.inf), np.full(3, np.inf), [1.0, 2.0, 3.0], d, 12.0)
    assert everywhere[:2] == (0.0, 12.0)
    half = M.clip(np.array([-np.inf, 0.0, -np.inf]), np.array([np.inf, 2.0, np.inf]), [0.0, 5.0, 0.0], [0.0, -1.0, 0.0], np.inf)
    assert half[:2] == (3.0, 5.0)
    # the transmittance and the free flight of these
    med = dict(sigma_t=0.5, lo=lo, hi=hi)
    assert M.transmittance(med, [1.0, 1.0, -2.0], [0.0, 0.0, 1.0], np.inf)[0] == pytest.approx(np.exp(-3.0))
    assert M.transmittance(med, [-1.0, 10.0, 1.0], [1.0, 0.0, 0.0], np.inf)[0] == 1.0
    assert M.transmittance(dict(med, lo=np.full(3, -np.inf), hi=np.full(3, np.inf)), [0, 0, 0], [0, 1, 0], np.inf)[0] == 0.0
    assert M.flight(0.5, 0.0) == 0.0 and M.flight(0.5, 1.0 - np.exp(-1.0)) == pytest.approx(2.0)
