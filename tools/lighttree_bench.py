"""The light hierarchy (option light_tree): launch time and variance of render_nee on scenes.many_lights, the table against the tree, and the
host build time of the tree.

usage: python tools/lighttree_bench.py [W=1920 H=1080] [bounces=4] [spp=16] [reps=7] [lamps=256] [build=1]

render_nee(spp, "mis") with option moments: wall clock around one launch and a sync, after one warm-up launch per context; `reps` launches
each, the two contexts alternating -- off: many_lights(lamps) with the table's cdf (the family the scene took before: k_nee); on: the same
with option light_tree (k_nee<kNeeLightTree>).  variance: the mean over the pixels of Scene.read_variance() after the last launch (the variance
of the pixel's mean luminance at `spp` samples).  build=1: the wall clock of the first Scene.debug_light_tree() on host-only contexts
holding 2, 512 and 100,000 emitting triangles (the light table and the tree; the scene's own upload is not in it).  One JSON line on
stdout."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from opencl_path_tracer_amd import api, scenes  # noqa: E402


def build_ms(n):
    rng = np.random.default_rng(n)
    c = rng.uniform(-100.0, 100.0, size=(n, 1, 3))
    v = (c + rng.uniform(-0.5, 0.5, size=(n, 3, 3))).astype(np.float32)
    sc = api.Scene(16, 16, device=None)
    sc.add_Material((0, 0, 0), (0, 0, 0), (6.0, 5.0, 4.0), (0, 0, 0), (0, 0, 0), 0.0, 3)
    sc.add_Triangles(api.triangles_from_vertices(v, np.zeros(n, dtype=np.uint16)))
    sc.end_Obj()
    sc.upload_Triangles()
    sc.upload_Materials()
    sc.debug_light_table()
    t0 = time.perf_counter()
    nodes, _ = sc.debug_light_tree()
    ms = (time.perf_counter() - t0) * 1e3
    return dict(lights=n, nodes=len(nodes), depth=int(sc.stat("light_tree_depth")), ms=round(ms, 3))


def main():
    kw = dict(W=1920, H=1080, bounces=4, spp=16, reps=7, lamps=256, build=1)
    for a in sys.argv[1:]:
        k, v = a.split("=")
        kw[k] = type(kw[k])(v)
    ctx = {}
    for name in ("off", "on"):
        sc = api.Scene(kw["W"], kw["H"]).load(scenes.many_lights(kw["lamps"]))
        sc.iterations = kw["bounces"]
        sc.set_option("moments", 1)
        sc.set_option("light_tree", 1 if name == "on" else 0)
        sc.render_nee(kw["spp"], "mis")
        sc.sync()
        ctx[name] = sc
    ms = {name: [] for name in ctx}
    for _ in range(kw["reps"]):
        for name, sc in ctx.items():
            sc.current_sample = 0
            sc.seed_default()
            sc.sync()
            t0 = time.perf_counter()
            sc.render_nee(kw["spp"], "mis")
            sc.sync()
            ms[name].append(round((time.perf_counter() - t0) * 1e3, 2))
    out = dict(kw)
    for name, sc in ctx.items():
        out[name + "_ms"] = ms[name]
        out[name + "_median_ms"] = sorted(ms[name])[len(ms[name]) // 2]
        out[name + "_family"] = int(sc.stat("nee_family"))
        out[name + "_variance"] = float(np.asarray(sc.read_variance(), dtype=np.float64).mean())
    out["variance_ratio"] = out["off_variance"] / out["on_variance"]
    out["tree_nodes"], out["tree_depth"] = int(ctx["on"].stat("light_tree_nodes")), int(ctx["on"].stat("light_tree_depth"))
    if kw["build"]:
        out["build"] = [build_ms(n) for n in (2, 512, 100000)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
