"""Adaptive frames (pt_render_adaptive / pt_render_adaptive_ex) against uniform ones: samples spent, wall time, rounds and error against a
high-spp frame.

usage: python tools/adaptive_sweep.py scene=cornell|mesh100k [W=1920 H=1080] [min=16] [max=1024] [ref=4096] [bounces=8]
                                      [thr=2,1.5,1,0.7,0.5,0.3,0.2,0.1,0] [uniform_steps=4]
                                      [metric=half|variance] [path=render|nee] [strategy=mis] [tonemapped=0|1] [env=0|1]
                                      [tiled_ab=0|1]

metric / path / strategy / tonemapped go to Scene.render_adaptive (none given: the old entry); the variance metric switches option
"moments" on.  With path=nee the uniform frames and the reference are render_nee at the same strategy; env=1 sets scenes.sun_and_sky()
(only the NEE path draws it).  tiled_ab=1 also times, by HIP events (option "timing"), two launches of 32 samples over the whole frame:
uniform render_nee (k_nee) against the rounds of an adaptive frame with min = max = 64 (its TILED instances).

The reference is a uniform render of `ref` samples on its own context.  For every threshold: samples spent, wall time of the
call (host clock around render_adaptive + sync, which includes the per-round synchronisation), the rounds with their active
tiles, and RMSE / rel-L2 of the colours against the reference (and the RMSE after Reinhard's c / (1 + c): "RMSE tm"); the same for uniform renders of max, max/2, max/4 and max/8 samples."""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from opencl_path_tracer_amd import api, scenes  # noqa: E402


def scene_spec(name):
    if name == "cornell":
        return scenes.cornell_box()
    if name == "mesh100k":
        return scenes.displaced_grid_mesh(100000)
    raise SystemExit("scene must be cornell or mesh100k")


def errors(cols, ref):
    """RMSE and rel-L2 of the colours, and the RMSE after Reinhard's c / (1 + c) per channel (display-referred)."""
    c, r = cols[:, :3].astype(np.float64), ref[:, :3].astype(np.float64)
    d = c - r
    t = c / (1.0 + c) - r / (1.0 + r)
    return float(np.sqrt(np.mean(d * d))), float(np.linalg.norm(d) / np.linalg.norm(r)), float(np.sqrt(np.mean(t * t)))


def main():
    a = dict(kv.split("=", 1) for kv in sys.argv[1:])
    name = a.get("scene", "cornell")
    W, H = int(a.get("W", 1920)), int(a.get("H", 1080))
    lo, hi, ref_spp, bounces = int(a.get("min", 16)), int(a.get("max", 1024)), int(a.get("ref", 4096)), int(a.get("bounces", 8))
    thrs = [float(t) for t in a.get("thr", "2,1.5,1,0.7,0.5,0.3,0.2,0.1,0").split(",")]
    spec = scene_spec(name)
    ex = {k: a[k] for k in ("metric", "path", "strategy") if k in a}
    if "tonemapped" in a:
        ex["tonemapped"] = int(a["tonemapped"])
    nee = ex.get("path") == "nee"
    strategy = ex.get("strategy", "mis")
    env = scenes.sun_and_sky() if int(a.get("env", 0)) else None
    if env is not None and not nee:
        raise SystemExit("env=1 needs path=nee")

    def ctx():
        sc = api.Scene(W, H).load(spec)
        sc.iterations = bounces
        if ex.get("metric") == "variance":
            sc.set_option("moments", 1)
        if env is not None:
            sc.set_environment(env)
        return sc

    def uniform(sc, n):
        if nee:
            sc.render_nee(n, strategy)
        else:
            sc.render(n)

    sc = ctx()
    uniform(sc, 2)                                   # warm-up: code objects, LDS attributes
    sc.sync()
    sc.close()
    if ex:
        sc = ctx()
        sc.render_adaptive(2, 4, 0.0, **ex)          # the tiled instances and the decision kernels too
        sc.sync()
        sc.close()
    sc = ctx()
    t0 = time.perf_counter()
    uniform(sc, ref_spp)
    sc.sync()
    ref = sc.read_colors()
    print("%s %dx%d, %d bounces; reference: uniform %s %d spp (%.2f s)" % (name + (" + sun_and_sky" if env is not None else ""), W, H, bounces,
                                                                        "render_nee(%s)" % strategy if nee else "render", ref_spp, time.perf_counter() - t0))
    print("adaptive entry: %s" % (" ".join("%s=%s" % kv for kv in sorted(ex.items())) if ex else "pt_render_adaptive (half, render)"))
    sc.close()
    rows = []
    for spp in [hi >> k for k in range(int(a.get("uniform_steps", 4))) if (hi >> k) >= lo]:     # the uniform curve, for equal-RMSE reads
        sc = ctx()
        t0 = time.perf_counter()
        uniform(sc, spp)
        sc.sync()
        dt = time.perf_counter() - t0
        rmse, rel, tm = errors(sc.read_colors(), ref)
        rows.append(("uniform %d" % spp, W * H * spp, dt, rmse, rel, tm, ""))
        sc.close()
    for thr in thrs:
        sc = ctx()
        t0 = time.perf_counter()
        res = sc.render_adaptive(lo, hi, thr, **ex)
        sc.sync()
        dt = time.perf_counter() - t0
        rmse, rel, tm = errors(sc.read_colors(), ref)
        rounds = " ".join("%d:%d" % (b, n) for b, n in zip(res["rounds"], res["active_tiles"]))
        rows.append(("adaptive %d-%d thr %g" % (lo, hi, thr), res["samples"], dt, rmse, rel, tm, rounds))
        sc.close()
    print("%-28s %14s %9s %9s %10s %10s %10s  %s" % ("run", "samples", "x uniform", "wall ms", "RMSE", "rel-L2", "RMSE tm", "rounds (boundary:active tiles)"))
    for r in rows:
        print("%-28s %14d %9.3f %9.1f %10.5f %10.5f %10.5f  %s" % (r[0], r[1], r[1] / float(rows[0][1]), 1e3 * r[2], r[3], r[4], r[5], r[6]))
    if int(a.get("tiled_ab", 0)) and nee:
        for rep in range(2):
            un = ctx()
            un.set_option("timing", 1)
            un.render_nee(32, strategy)
            un.render_nee(32, strategy)
            un.sync()
            ti = ctx()
            ti.set_option("timing", 1)
            ti.render_adaptive(64, 64, 0.0, **ex)
            ti.sync()
            same = np.array_equal(un.read_colors().view(np.uint32), ti.read_colors().view(np.uint32))
            print("tiled_ab %d: 2 x 32 samples, whole frame: k_nee %.2f ms, k_nee TILED %.2f ms (HIP events), same bits: %s"
                  % (rep, un.stat("kernel_ms"), ti.stat("kernel_ms"), same))
            un.close()
            ti.close()


if __name__ == "__main__":
    main()
