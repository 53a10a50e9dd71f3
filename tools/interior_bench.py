"""Interiors of dielectrics (Scene.set_material_interior): launch time of render_nee on the Cornell box, clear glass against a null binding,
a tinted sphere and a waxy sphere.

usage: python tools/interior_bench.py [W=1920 H=1080] [bounces=8] [spp=16] [reps=7] [wax=4.0]

render_nee(spp, "mis"): wall clock around one launch and a sync, after one warm-up launch per context; `reps` launches each, the
contexts alternating -- clear: cornell_box() (the family the scene took before: k_nee); null: the same with an all-zero interior on
GLASS (k_nee<kNeeInterior> computing the same frame: what the family's run-time fields cost); tint: cornell_box(tint=(0.9, 0.5, 0.2))
(absorption only: the same paths); wax: cornell_box(tint=..., wax=wax) (paths scatter inside the sphere: the frame and its path lengths
differ).  One JSON line on stdout."""
import json
import sys
import time

sys.path.insert(0, ".")
from opencl_path_tracer_amd import api, scenes  # noqa: E402

TINT = (0.9, 0.5, 0.2)


def main():
    kw = dict(W=1920, H=1080, bounces=8, spp=16, reps=7, wax=4.0)
    for a in sys.argv[1:]:
        k, v = a.split("=")
        kw[k] = type(kw[k])(v)
    specs = {"clear": scenes.cornell_box(), "null": scenes.cornell_box(), "tint": scenes.cornell_box(tint=TINT),
             "wax": scenes.cornell_box(tint=TINT, wax=kw["wax"])}
    ctx = {}
    for name, spec in specs.items():
        sc = api.Scene(kw["W"], kw["H"]).load(spec)
        sc.iterations = kw["bounces"]
        if name == "null":
            sc.set_material_interior(scenes.GLASS)
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
    print(json.dumps(out))


if __name__ == "__main__":
    main()
