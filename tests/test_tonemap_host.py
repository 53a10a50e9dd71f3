"""-m "not gpu": the authored frames of tests/test_gpu_tonemap.py (tests/tonemap_inputs.py) hold what they are built for, counted against
the oracle alone; the numpy restatements used there (the median's selection order, the 8-bit quantiser) agree with the oracle and with
pt_image_write_ppm."""
import numpy as np

import spec_inputs as S
import tonemap_inputs as T


def oracle_filt(oracle, frame, w, h):
    f = oracle.OracleFrame(w, h, seed_default=False)
    f.colors()[:] = frame
    f.filt_im()
    out = f.tex().copy()
    f.close()
    return out


def test_reinhard_pool_holds_every_category(oracle):
    pool, cat = T.reinhard_pool()
    out = oracle.reinhard_n(pool)
    count = {k: int((cat == k).sum()) for k in np.unique(cat)}
    print("[tonemap] Reinhard pool: %d pixels, %s" % (pool.shape[0], count))
    for k in ("zero", "denormal", "negative", "knee", "huge", "nan", "zero_luminance", "ordinary"):
        assert count.get(k, 0) >= 3, k
    pb = S.bits(pool)
    assert (pb == 0).any() and (pb == 0x80000000).any()                                              # zeros of both signs
    assert (((pb & 0x7f800000) == 0) & ((pb & 0x7fffff) != 0)).any()                                 # denormals
    assert (pool == np.inf).any() and (pool == np.float32(1e30)).any() and np.isnan(pool).any() and (pool < 0).any()
    # the knee: the value handed to the sRGB curve within 8 ulps of 0.00304 on either side of it, and exactly on it or next to it
    a, _ = T.reinhard_scale(pool[cat == "knee"])
    d = S.bits(a).astype(np.int64) - int(S.bits(T.KNEE)[0])
    assert ((d <= 0) & (d >= -8)).sum() >= 8 and ((d > 0) & (d <= 8)).sum() >= 8, np.sort(d.reshape(-1))
    # zero luminance with non-zero channels: L is exactly 0, positive and negative channels cancel, and the map gives NaN (0 / 0)
    z = pool[cat == "zero_luminance"]
    _, L = T.reinhard_scale(z)
    assert (L == 0).all() and ((z > 0).any(axis=1) & (z < 0).any(axis=1)).all() and np.isnan(out[cat == "zero_luminance", :3]).all()
    assert np.isnan(out[cat == "zero", :3]).all() and (out[:, 3] == 1.0).all()
    # every size from 3 x 3 up shows all categories but possibly a few; the largest holds the whole pool
    assert T.SIZES[-1][0] * T.SIZES[-1][1] >= pool.shape[0]
    for w, h in T.SIZES:
        fr = T.reinhard_frame(w, h)
        assert fr.shape == (w * h, 4) and np.array_equal(S.bits(fr[:, :3]), S.bits(pool[(np.arange(w * h) + 7 * w + h) % pool.shape[0]]))


def test_median_frames_hold_ties_that_show_the_selection_order(oracle):
    total = {"two": 0, "three": 0, "nine": 0, "nan_grey": 0, "order_matters": 0, "at_004": 0}
    for w, h in T.SIZES:
        fr = T.median_frame(w, h)
        want = oracle_filt(oracle, fr, w, h).reshape(h, w, 4)
        border = np.ones((h, w), dtype=bool)
        border[1:h - 1, 1:w - 1] = False
        assert (want[border] == 0).all()                                                            # border pixels read 0
        if w < 3 or h < 3:
            continue
        nb = T.neighbourhoods(fr, w, h)
        mine = T.median_by_selection(nb)
        film = np.zeros((mine.shape[0], 4), dtype=np.float32)
        for i in range(mine.shape[0]):
            oracle.lib().orc_filmic_tone_map(film[i].ctypes.data_as(oracle.C.POINTER(oracle.C.c_float)), mine[i].ctypes.data_as(oracle.C.POINTER(oracle.C.c_float)))
        got, ref = S.bits(film), S.bits(want[1:h - 1, 1:w - 1].reshape(-1, 4))
        assert ((got == ref) | (np.isnan(film) & np.isnan(S.fl(ref)))).all(), (w, h)                # the restated selection is the oracle's
        other = T.median_by_stable_sort(nb)
        g = T.grey(nb)
        gm = T.grey(mine)
        ties = (g == gm[:, None]).sum(axis=1)
        total["two"] += int((ties == 2).sum())
        total["three"] += int((ties == 3).sum())
        total["nine"] += int((ties == 9).sum())
        total["nan_grey"] += int(np.isnan(g).any(axis=1).sum())
        total["order_matters"] += int((S.bits(mine) != S.bits(other)).any(axis=1).sum())
        total["at_004"] += int((np.abs(S.bits(mine).astype(np.int64) - T.E004) <= 3).any(axis=1).sum())
    print("[tonemap] median neighbourhoods: %s" % total)
    assert total["two"] >= 50 and total["three"] >= 50 and total["nine"] >= 5 and total["nan_grey"] >= 100, total
    assert total["order_matters"] >= 100 and total["at_004"] >= 20, total


def test_quantiser_restates_the_writer(api, tmp_path):
    w, h = 33, 9
    fr = T.reinhard_frame(w, h)                                                                     # infinities, negatives, NaN and all
    fr[:12, 0] = np.array([0.5 / 255, 1.5 / 255, 2.5 / 255, 254.5 / 255, 1.0, 1.0000001, 0.999999, -0.0, 0.0019607844, 0.0019607842, 1e-9, 0.49803922],
                          dtype=np.float32)                                                         # ties to even, and the clamp's edges
    path = str(tmp_path / "q.ppm")
    assert api.LIB.pt_image_write_ppm(path.encode(), fr.ctypes.data_as(api.C.c_void_p), w, h) == api.PT_OK
    raw = open(path, "rb").read()
    head = b"P6\n%d %d\n255\n" % (w, h)
    assert raw[:len(head)] == head and raw[len(head):] == T.quantise(fr, w, h)
