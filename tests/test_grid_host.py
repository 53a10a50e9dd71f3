"""The medium's density grid (Scene.set_medium_density; include/pt_api.h) on host-only contexts -- the checks of pt_set_medium_density,
the read-back, the refusal of an unbounded box at render time, SceneSpec.medium_density -- and tests/grid_ref.py against brute-force
integration and against tests/medium_ref.py: no device needed."""

import ctypes as C
import os

import numpy as np
import pytest

import grid_ref as GR
import medium_ref as M
import test_gpu_medium as TM

NEW_SYMBOLS = ["pt_set_medium_density", "pt_clear_medium_density", "pt_debug_medium_density", "pt_debug_grid"]
INF = float("inf")
BOX = ((-1.0, -2.0, -3.0), (4.0, 5.0, 6.0))


def host_scene(api):
    from opencl_path_tracer_amd import scenes
    return api.Scene(16, 16, device=None).load(scenes.cornell_box(8, 4))


def test_abi_has_the_new_symbols(api):
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pt_api.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name in api.EXPORTS and hasattr(api.LIB, name) and name + "(" in header
    assert "#define PT_GRID_MAX_DIM 256" in header and api.PT_GRID_MAX_DIM == 256
    assert C.sizeof(api.Medium) == 44                                # pt_medium is as it was


def test_set_medium_density_checks_its_arguments(api):
    sc = host_scene(api)
    assert sc.medium_density() is None
    rng = np.random.default_rng(1)
    good = rng.random((2, 3, 4)).astype(np.float32)                 # (nz, ny, nx): nx = 4, ny = 3, nz = 2
    good[1, 2, 3] = 0.0
    sc.set_medium_density(good)                                     # a grid may be set before its medium
    held = sc.medium_density()
    assert held.dtype == np.float32 and held.shape == (2, 3, 4) and np.array_equal(held, good)
    dims = (C.c_int32 * 3)()
    assert api.LIB.pt_debug_medium_density(sc._h, None, 0, dims) == 1 and list(dims) == [4, 3, 2]
    part = np.full(5, -1.0, dtype=np.float32)                       # cap below the size: the first cap values, i fastest
    assert api.LIB.pt_debug_medium_density(sc._h, part.ctypes.data_as(C.c_void_p), 5, dims) == 1
    assert np.array_equal(part, good.reshape(-1)[:5]) and part[4] == good[0, 1, 0]

    def refused(call, word):
        with pytest.raises(api.PtError) as e:
            call()
        assert e.value.code == api.PT_EINVAL and "pt_set_medium_density" in str(e.value) and word in str(e.value)
        assert np.array_equal(sc.medium_density(), good)            # a refused call leaves the held grid as it was

    for bad in (-0.5, float("nan"), INF, -INF):
        d = np.ones((2, 2, 2), dtype=np.float32)
        d[1, 0, 1] = bad
        refused(lambda: sc.set_medium_density(d), "density 5")
    one = np.ones(257, dtype=np.float32)
    ptr = one.ctypes.data_as(C.c_void_p)
    for nx, ny, nz in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (257, 1, 1), (1, 257, 1), (1, 1, 257)):
        refused(lambda: sc._ck(api.LIB.pt_set_medium_density(sc._h, ptr, nx, ny, nz)), "dimension")
    refused(lambda: sc._ck(api.LIB.pt_set_medium_density(sc._h, None, 1, 1, 1)), "NULL")
    assert api.LIB.pt_set_medium_density(None, ptr, 1, 1, 1) == api.PT_EINVAL and api.LIB.pt_clear_medium_density(None) == api.PT_EINVAL
    assert api.LIB.pt_debug_medium_density(None, None, 0, dims) == api.PT_EINVAL and api.LIB.pt_debug_medium_density(sc._h, None, 0, None) == api.PT_EINVAL
    assert api.LIB.pt_debug_medium_density(sc._h, None, -1, dims) == api.PT_EINVAL and api.LIB.pt_debug_grid(None, None, 0, None) == api.PT_EINVAL
    with pytest.raises(ValueError):
        sc.set_medium_density(np.ones((2, 2), dtype=np.float32))
    # the largest dimension, and the largest along each axis alone
    sc._ck(api.LIB.pt_set_medium_density(sc._h, ptr, 256, 1, 1))
    assert sc.medium_density().shape == (1, 1, 256)
    sc.set_medium_density(np.ones((256, 1, 1)))                     # float64 in: kept as float32
    assert sc.medium_density().shape == (256, 1, 1) and sc.medium_density().dtype == np.float32
    sc.set_medium_density(good)
    # uploads and the medium calls keep the grid; clearing the medium does not clear it; it is live only with sigma_t > 0
    sc.upload_Triangles()
    sc.upload_Materials()
    sc.set_medium(0.5, bounds=BOX)
    sc.clear_medium()
    assert np.array_equal(sc.medium_density(), good)
    for setup, word in ((lambda: None, "live"), (lambda: sc.set_medium(0.0, bounds=BOX), "live")):
        setup()
        with pytest.raises(api.PtError) as e:                       # no medium, or sigma_t = 0: nothing to walk
            sc.debug_grid(np.zeros((1, 12), dtype=np.float32))
        assert e.value.code == api.PT_EINVAL and word in str(e.value)
    sc.set_medium(0.5, bounds=BOX)
    with pytest.raises(api.PtError) as e:                           # live: the debug kernel needs a device
        sc.debug_grid(np.zeros((1, 12), dtype=np.float32))
    assert e.value.code == api.PT_ENODEVICE
    sc.clear_medium_density()
    assert sc.medium_density() is None and sc.medium()["sigma_t"] == 0.5
    assert api.LIB.pt_debug_medium_density(sc._h, None, 0, dims) == 0 and list(dims) == [0, 0, 0]
    sc.clear_medium_density()                                       # clearing nothing is fine


def test_an_unbounded_box_is_refused_at_render_time_before_the_device(api):
    sc = host_scene(api)
    sc.iterations = 4
    nee_calls = (lambda: sc.render_nee(1, "mis"), lambda: sc.render_nee(1, "bsdf"),
                 lambda: sc.render_adaptive(2, 4, 0.1, path="nee", metric="half", strategy="mis"))

    def codes():
        out = []
        for call in nee_calls:
            with pytest.raises(api.PtError) as e:
                call()
            out.append((e.value.code, str(e.value)))
        return out
    sc.set_medium_density(np.ones((2, 2, 2), dtype=np.float32))
    assert all(c == api.PT_ENODEVICE for c, _ in codes())           # a grid without a medium is not live
    sc.set_medium(0.01)                                             # the defaults: unbounded everywhere; lo.x is the first bound met
    for (code, text), name in zip(codes(), ("pt_render_nee", "pt_render_nee", "pt_render_adaptive")):
        assert code == api.PT_EINVAL and name in text and "lo.x" in text and "infinite" in text
    for k, (axis, side) in enumerate([(a, s) for a in "xyz" for s in ("lo", "hi")]):
        lo, hi = [-1.0, -2.0, -3.0], [4.0, 5.0, 6.0]
        (lo if side == "lo" else hi)["xyz".index(axis)] = -INF if side == "lo" else INF
        sc.set_medium(0.01, bounds=(lo, hi))
        for code, text in codes():
            assert code == api.PT_EINVAL and side + "." + axis in text, (side, axis, text)
        with pytest.raises(api.PtError) as e:
            sc.debug_grid(np.zeros((1, 12), dtype=np.float32))
        assert e.value.code == api.PT_EINVAL and side + "." + axis in str(e.value)
    sc.set_medium(0.01, bounds=BOX)                                 # a finite box: only the device is missing
    assert all(c == api.PT_ENODEVICE for c, _ in codes())
    sc.set_medium(0.0)                                              # sigma_t = 0: no medium, so no live grid, whatever the box
    assert all(c == api.PT_ENODEVICE for c, _ in codes())
    sc.set_medium(0.01)
    sc.clear_medium_density()                                       # the homogeneous medium may be unbounded
    assert all(c == api.PT_ENODEVICE for c, _ in codes())
    with pytest.raises(api.PtError) as e:                           # and the other paths refuse as for any medium
        sc.render(1)
    assert e.value.code == api.PT_EINVAL and "pt_clear_medium" in str(e.value)


def test_scene_spec_density_round_trips_through_load_and_the_plume_is_a_plume(api):
    from opencl_path_tracer_amd import scenes
    assert scenes.cornell_box(8, 4).medium_density is None and scenes.cornell_box(8, 4, fog=1e-3).medium_density is None
    assert api.Scene(16, 16, device=None).load(scenes.cornell_box(8, 4, fog=1e-3)).medium_density() is None
    plume = scenes.smoke_plume(8)
    assert plume.shape == (8, 8, 8) and plume.dtype == np.float32 and np.isfinite(plume).all()
    assert plume.min() == 0.0 and 1.0 < plume.max() <= 4.0 and 0.2 < (plume == 0.0).mean() < 0.9
    assert scenes.smoke_plume().shape == (32, 32, 32) and np.array_equal(scenes.smoke_plume(8), plume)
    big = scenes.smoke_plume(32)
    peak, filled = big.max(axis=(0, 2)), (big > 0.0).sum(axis=(0, 2))       # per height (axis 1 is y), above the ground mist:
    assert peak[4] > peak[16] > peak[30] > 0.0 and filled[4] < filled[16] < filled[30]      # it thins and widens upwards
    column = big[:, :, 12:20][12:20].sum()                          # the middle of the box holds most of it above the mist
    assert column > 0.5 * big[:, 4:, :].sum()
    spec = scenes.cornell_box(8, 4, fog=1e-3, density=plume)
    sc = api.Scene(16, 16, device=None).load(spec)
    assert np.array_equal(sc.medium_density(), plume) and sc.medium()["lo"] == scenes.CORNELL_ROOM[0]
    with pytest.raises(ValueError):
        scenes.cornell_box(8, 4, density=plume)
    spec = scenes.cornell_box(8, 4)
    spec.medium = dict(sigma_t=0.5, bounds=BOX)
    spec.medium_density = [[[1.0, 2.0]], [[3.0, 4.0]]]              # anything array-like of three dimensions
    assert np.array_equal(api.Scene(16, 16, device=None).load(spec).medium_density(), np.asarray(spec.medium_density, dtype=np.float32))


# ---------------------------------------------------------------------------- tests/grid_ref.py
def random_ray(rng, lo, hi):
    """from around the box towards a point of it (three in four), or anywhere"""
    P = rng.uniform(lo - 2.0, hi + 2.0)
    d = rng.uniform(lo, hi) - P if rng.random() < 0.75 else rng.normal(size=3)
    return P, d / np.linalg.norm(d)


def test_the_float64_walk_integrates_the_density():
    """walk() with tau = +inf against the midpoint rule on 200,000 points per ray, each looking its voxel up by its own position: the rule's
    error is one sample's worth per density jump, (length / 200,000) x the jump x at most nx + ny + nz jumps -- below 1e-3 here."""
    rng = np.random.default_rng(11)
    lo, hi = np.array([0.0, -1.0, 2.0]), np.array([4.0, 2.0, 4.0])
    rho = rng.random((2, 3, 4)) * 3.0
    rho[0, 1, 2] = 0.0
    rho[1, 2, 0] = 8.0
    sigma = 0.7
    crossing = 0
    for _ in range(60):
        P, D = random_ray(rng, lo, hi)
        t = np.inf if rng.random() < 0.5 else rng.uniform(1.0, 8.0)
        w = GR.walk(sigma, rho, lo, hi, P, D, t, np.inf)
        assert not w["scatter"] and w["visited"] <= 4 + 3 + 2 + 3
        if not max(w["b"] - w["a"], 0.0) > 0.0:
            assert w["acc"] == 0.0 and w["visited"] == 0
            continue
        crossing += 1
        want = GR.brute_depth(sigma, rho, lo, hi, P, D, w["a"], w["b"])
        assert abs(w["acc"] - want) < 1e-3, (P, D, t, w["acc"], want)
        assert abs(sum(t1 - t0 for _, t0, t1 in w["voxels"]) - (w["b"] - w["a"])) < 1e-12           # the voxels tile [a, b]
        # the free flight inverts the depth: the walk that stops at half of it has accumulated exactly that much
        if w["acc"] > 0.0:
            half = GR.walk(sigma, rho, lo, hi, P, D, t, 0.5 * w["acc"])
            assert half["scatter"] and w["a"] <= half["s"] <= w["b"]
            assert abs(GR.brute_depth(sigma, rho, lo, hi, P, D, w["a"], half["s"]) - 0.5 * w["acc"]) < 1e-3
            assert rho.reshape(-1)[half["voxel"]] > 0.0
            assert not GR.walk(sigma, rho, lo, hi, P, D, t, w["acc"] * (1.0 + 1e-9))["scatter"]
    assert crossing > 20


def test_the_walk_on_hand_made_rays():
    lo, hi = np.array([0.0, 0.0, 0.0]), np.array([4.0, 3.0, 2.0])
    rho = np.arange(24, dtype=np.float64).reshape(2, 3, 4)          # voxel (i, j, k) holds (k 3 + j) 4 + i
    along_x = GR.walk(1.0, rho, lo, hi, [-1.0, 1.5, 0.5], [1.0, 0.0, 0.0], np.inf, np.inf)
    assert [v for v, _, _ in along_x["voxels"]] == [4, 5, 6, 7] and along_x["acc"] == 4 + 5 + 6 + 7 and (along_x["a"], along_x["b"]) == (1.0, 5.0)
    back_z = GR.walk(1.0, rho, lo, hi, [3.5, 2.5, 5.0], [0.0, 0.0, -1.0], np.inf, np.inf)
    assert [v for v, _, _ in back_z["voxels"]] == [23, 11] and back_z["acc"] == 34.0
    cut = GR.walk(1.0, rho, lo, hi, [-1.0, 1.5, 0.5], [1.0, 0.0, 0.0], 2.5, np.inf)                 # t ends inside voxel 5
    assert [v for v, _, _ in cut["voxels"]] == [4, 5] and cut["acc"] == 4 + 0.5 * 5
    hit = GR.walk(1.0, rho, lo, hi, [-1.0, 1.5, 0.5], [1.0, 0.0, 0.0], np.inf, 4.0 + 2.5)           # half way through voxel 5
    assert hit["scatter"] and hit["voxel"] == 5 and hit["s"] == 2.5 and hit["visited"] == 2
    first = GR.walk(1.0, rho, lo, hi, [0.5, 0.5, 0.5], [1.0, 0.0, 0.0], np.inf, 0.5)                # voxel 0 is empty: never scatters there
    assert first["voxel"] == 1 and first["s"] == 0.5 + 0.5        # (voxel 1 starts at parameter 0.5)
    edge = GR.walk(1.0, rho, lo, hi, [0.5, 0.5, 0.5], [1.0, 0.0, 0.0], np.inf, 1.0)                 # d = seg exactly is no scatter (d < seg):
    assert edge["voxel"] == 2 and edge["s"] == 1.5                                                  # the next voxel takes it at its start
    diagonal = GR.walk(1.0, np.ones((2, 2, 2)), [0, 0, 0], [2, 2, 2], [-1, -1, -1], np.ones(3) / np.sqrt(3.0), np.inf, np.inf)
    assert diagonal["near"]                                         # through the centre: three planes at once
    assert abs(diagonal["acc"] - 2.0 * np.sqrt(3.0)) < 1e-12 and diagonal["visited"] <= 2 + 2 + 2 + 3
    assert GR.walk(1.0, rho, lo, hi, [5.0, 1.0, 1.0], [1.0, 0.0, 0.0], np.inf, 1.0)["visited"] == 0   # the box is behind the ray


def test_a_unit_grid_is_the_medium_model_exactly(api):
    """GridModel with a 1 x 1 x 1 grid of 1 against MediumModel on test_gpu_medium.py's replay scene in its fog (host-only context): the
    same colours, states and ties to the last bit, for pixels spread over the frame, in both strategies"""
    import test_gpu_lights as TL
    sc, spec, rgb = TM.fog_replay_scene(api, True, device=None)
    plain = TM.fog_replay_model(api, sc, spec, rgb, True)
    sc.set_medium_density(np.ones((1, 1, 1), dtype=np.float32))
    verts, mo = spec.objects[0]
    env = dict(rgb=rgb, tables=sc.debug_environment(), scale=TL.REPLAY["scale"], yaw_degrees=TL.REPLAY["yaw_degrees"])
    grid = GR.GridModel(verts, api.triangles_from_vertices(verts, mo)["N"], np.concatenate([api.Material(*m) for m in spec.materials]), mo, sc.camera[0],
                        sc.debug_lights(), sc.medium(), env=env, table=sc.debug_light_table(), density=sc.medium_density())
    seeds = TL.replay_seeds()
    scattered = 0
    module = M.clip, M.flight, M.transmittance
    for gid in range(5, TL.REPLAY["W"] * TL.REPLAY["H"], 37):
        for strategy in (1, 2):
            a = plain.sample(gid, int(seeds[gid]), 4, strategy)
            events = dict(plain.last)
            b = grid.sample(gid, int(seeds[gid]), 4, strategy)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1] and (a[2] or not b[2]), gid      # (the walk may add a tie, never lose one)
            assert all(grid.last[k] == v for k, v in events.items())
            scattered += events["scatter"]
    assert scattered > 20 and (M.clip, M.flight, M.transmittance) == module          # the module is as it was after the calls
    none = GR.GridModel(verts, api.triangles_from_vertices(verts, mo)["N"], np.concatenate([api.Material(*m) for m in spec.materials]), mo, sc.camera[0],
                        sc.debug_lights(), sc.medium(), env=env, table=sc.debug_light_table(), density=None)
    assert np.array_equal(none.sample(5, int(seeds[5]), 4, 2)[0], plain.sample(5, int(seeds[5]), 4, 2)[0])
