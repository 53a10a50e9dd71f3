"""No GPU: the host side of environment lighting (pt_set_environment and friends, include/pt_api.h).

  * PFM files: what write_pfm writes read_pfm reads, float for float; damaged files give PT_EIO;
  * env_lookup against the numpy statement of the mapping (tests/env_ref.py);
  * the sampling tables of a host-only context against a double-precision numpy build, the forced values of P_env;
  * every argument pt_set_environment must refuse."""

import numpy as np
import pytest

import env_ref as E


def host_scene(api, lights=False):
    sc = api.Scene(16, 16, device=None)
    from opencl_path_tracer_amd import scenes
    mats = [scenes.BUILTIN_MATERIALS[scenes.WHITE_DIFFUSE], scenes.BUILTIN_MATERIALS[scenes.LAMP]]
    spec = scenes.SceneSpec(materials=mats, name="host")
    tris = [((0, 0, 0), (1, 0, 0), (0, 0, 1))] + ([((0, 5, 0), (1, 5, 0), (0, 5, 1))] if lights else [])
    spec.objects.append((np.asarray(tris, dtype=np.float32), np.arange(len(tris), dtype=np.uint16)))
    return sc.load(spec)


# ---------------------------------------------------------------------------- PFM
def test_pfm_round_trip(api, tmp_path):
    rng = np.random.default_rng(3)
    w, h = 13, 7
    img = np.zeros((h, w, 4), dtype=np.float32)
    img[..., :3] = rng.standard_normal((h, w, 3)).astype(np.float32) * np.float32(1e3)
    img[0, 0, :3] = (0.0, np.float32(1e-38), np.float32(3e38))
    path = str(tmp_path / "a.pfm")
    api.write_pfm(path, img, w, h)
    back = api.read_pfm(path)
    assert back.shape == (h, w, 4)
    assert np.array_equal(back[..., :3].view(np.uint32), img[..., :3].view(np.uint32))
    assert not back[..., 3].any()


def test_pfm_big_endian_and_grey(api, tmp_path):
    w, h = 3, 2
    vals = np.arange(w * h, dtype=np.float32) + 0.5
    path = str(tmp_path / "g.pfm")
    with open(path, "wb") as f:
        f.write(b"Pf\n%d %d\n1.0\n" % (w, h))
        f.write(vals.astype(">f4").tobytes())
    back = api.read_pfm(path)
    assert np.array_equal(back[..., 0].reshape(-1), vals) and np.array_equal(back[..., 2].reshape(-1), vals)


def test_pfm_crlf_header(api, tmp_path):
    w, h = 3, 2
    vals = (np.arange(w * h * 3, dtype=np.float32) + 0.25).reshape(h, w, 3)
    path = str(tmp_path / "c.pfm")
    with open(path, "wb") as f:
        f.write(b"PF\r\n%d %d\r\n-1.0\r\n" % (w, h))
        f.write(vals.astype("<f4").tobytes())
    assert np.array_equal(api.read_pfm(path)[..., :3], vals)


@pytest.mark.parametrize("damage", ["truncated", "magic", "size", "scale", "empty", "missing"])
def test_pfm_damaged_files_give_eio(api, tmp_path, damage):
    w, h = 5, 4
    img = np.ones((h, w, 4), dtype=np.float32)
    path = str(tmp_path / "d.pfm")
    api.write_pfm(path, img, w, h)
    data = open(path, "rb").read()
    if damage == "truncated":
        data = data[:-5]
    elif damage == "magic":
        data = b"P6" + data[2:]
    elif damage == "size":
        data = data.replace(b"5 4", b"5 -4", 1)
    elif damage == "scale":
        data = data.replace(b"-1.0", b"zero", 1)
    elif damage == "empty":
        data = b""
    if damage == "missing":
        path = str(tmp_path / "nothing.pfm")
    else:
        open(path, "wb").write(data)
    with pytest.raises(api.PtError) as e:
        api.read_pfm(path)
    assert e.value.code == api.PT_EIO


# ---------------------------------------------------------------------------- the mapping
def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v)).astype(np.float32)


@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (64, 32)])
@pytest.mark.parametrize("yaw", [0.0, 37.5, -200.0])
def test_env_lookup_matches_numpy(api, w, h, yaw):
    rng = np.random.default_rng(w * 100 + h)
    dirs = [unit(v) for v in rng.standard_normal((3000, 3))]
    dirs += [unit(v) for v in ((0, 1, 0), (0, -1, 0), (1e-4, 1, 0), (0, -1, 1e-4))]                     # the poles
    yr = E.yaw_radians(yaw)
    for eps in (1e-3, -1e-3, 1e-4, -1e-4):                                                              # the phi seam, both sides
        for th in (0.3, 1.5, 2.9):
            dirs.append(unit((np.sin(th) * np.cos(yr + eps), np.cos(th), np.sin(th) * np.sin(yr + eps))))
    checked = 0
    for d in dirs:
        row, col, dist = E.lookup(w, h, yaw, d)
        if dist <= 1e-5:
            continue
        assert api.env_lookup(w, h, yaw, d) == (row, col), (d, dist)
        checked += 1
    assert checked > 0.99 * len(dirs)
    if (w, h) == (64, 32) and yaw == 0.0:
        assert api.env_lookup(w, h, 0.0, (0, 1, 0))[0] == 0 and api.env_lookup(w, h, 0.0, (0, -1, 0))[0] == h - 1
        assert api.env_lookup(w, h, 0.0, unit((1, 0, 1e-3))) == (16, 0) and api.env_lookup(w, h, 0.0, unit((1, 0, -1e-3))) == (16, 63)
        assert api.env_lookup(w, h, 0.0, (0, 0, 1)) == (16, 16) and api.env_lookup(w, h, 0.0, unit((-1, 0, 1e-3)))[1] == 31


# ---------------------------------------------------------------------------- the distribution
def test_tables_match_double_precision_build(api):
    from opencl_path_tracer_amd import scenes
    rng = np.random.default_rng(9)
    maps = [scenes.sun_and_sky(), rng.random((8, 16, 3)).astype(np.float32), np.full((1, 1, 3), 2.0, np.float32),
            rng.random((1, 2, 3)).astype(np.float32)]
    sparse = np.zeros((32, 64, 3), dtype=np.float32)          # rows of weight 0, one hot texel, a dim band
    sparse[5, 40] = (900.0, 800.0, 700.0)
    sparse[20:24] = 0.01
    maps.append(sparse)
    sc = host_scene(api)
    for rgb in maps:
        sc.set_environment(rgb)
        t = sc.debug_environment()
        row, col, has = E.tables(rgb)
        assert has
        h, w = rgb.shape[:2]
        assert np.array_equal(t["row_cdf"], row.astype(np.float32)) or np.abs(t["row_cdf"] - row).max() <= 2.0 ** -24
        assert np.abs(t["col_cdf"] - col).max() <= 2.0 ** -24
        assert t["row_cdf"][-1] == 1.0 and (t["col_cdf"][:, -1] == 1.0).all()
        assert (np.diff(t["row_cdf"]) >= 0).all() and (np.diff(t["col_cdf"], axis=1) >= 0).all()
        # p_env is P(texel) / Omega(row) with P from the stored cdfs' own steps, and the probabilities sum to 1
        want = E.texel_pdf(t["row_cdf"], t["col_cdf"])
        assert np.allclose(t["pdf"], want, rtol=2e-7, atol=0)
        total = float((t["pdf"].astype(np.float64) * E.solid_angles(w, h)[:, None]).sum())
        assert abs(total - 1.0) < 1e-6, total
        # proportional to luminance x solid angle wherever the share is large enough to survive the float cdf
        share = E.luminance(rgb) * E.solid_angles(w, h)[:, None]
        share /= share.sum()
        big = share > 1e-4
        assert np.allclose((t["pdf"] * E.solid_angles(w, h)[:, None])[big], share[big], rtol=2e-3)


def test_forced_and_effective_select(api):
    from opencl_path_tracer_amd import scenes
    rgb = scenes.sun_and_sky(16, 8)
    for lights in (False, True):
        sc = host_scene(api, lights)
        assert len(sc.debug_light_table()[0]) == (1 if lights else 0)
        for select in (0.0, 0.3, 0.5, 1.0 / 3.0, 1.0):
            sc.set_environment(rgb, select=select)
            want = float(np.ceil(float(np.float32(select)) * 2.0 ** 24) / 2.0 ** 24) if lights else 1.0
            assert sc.debug_environment()["P_env"] == want
        sc.set_environment(np.zeros((4, 8, 3), dtype=np.float32))            # all zero: no distribution
        t = sc.debug_environment()
        assert t["P_env"] == 0.0 and not t["pdf"].any()
    # the uploads keep the map; only the forced value follows the light table
    sc = host_scene(api, lights=True)
    sc.set_environment(rgb, select=0.25)
    assert sc.debug_environment()["P_env"] == 0.25
    sc.upload_Triangles()
    sc.upload_Materials()
    t = sc.debug_environment()
    assert t["P_env"] == 0.25 and t["pdf"].shape == (8, 16)
    sc.clear_environment()
    with pytest.raises(api.PtError) as e:
        sc.debug_environment()
    assert e.value.code == api.PT_EINVAL


def test_defaults(api):
    assert api.environment_defaults() == {"scale": 1.0, "yaw_degrees": 0.0, "select": 0.5}


# ---------------------------------------------------------------------------- validation
def test_set_environment_refuses_bad_arguments(api):
    sc = host_scene(api)
    good = np.ones((4, 8, 3), dtype=np.float32)

    def refused(rgb, **kw):
        with pytest.raises(api.PtError) as e:
            sc.set_environment(rgb, **kw)
        assert e.value.code == api.PT_EINVAL

    for bad in (np.nan, np.inf, -np.inf, -1e-3):
        m = good.copy()
        m[2, 5, 1] = bad
        refused(m)
    refused(np.ones((0, 8, 3), dtype=np.float32))
    refused(np.ones((4, 0, 3), dtype=np.float32))
    refused(np.ones((1, 4097, 3), dtype=np.float32))
    refused(np.ones((2049, 1, 3), dtype=np.float32))
    for s in (-0.01, 1.01, np.nan):
        refused(good, select=s)
    for s in (-1.0, np.inf, np.nan):
        refused(good, scale=s)
    refused(good, yaw_degrees=np.inf)
    with pytest.raises(api.PtError):
        sc.debug_environment()                    # nothing was set by the refused calls
    sc.set_environment(np.ones((4, 4096, 3), dtype=np.float32))      # the cap itself is allowed
    sc.set_environment(good, scale=0.0, select=1.0, yaw_degrees=720.0)
    with pytest.raises(TypeError):
        sc.set_environment(good, gamma=2.2)
