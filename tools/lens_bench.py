"""Thin lens (Scene.set_lens): launch time of render_nee with the lens on and off.

usage: python tools/lens_bench.py [W=1920 H=1080] [bounces=8] [spp=16] [reps=5] [aperture=25] [focus=1600]

The Cornell box, render_nee(spp, "mis"): wall clock around one launch and a sync, after one warm-up launch per context; `reps` launches
each, the two contexts alternating (lens on: k_nee<kNeeLens>; lens off: the parent's k_nee, the parent's bits).  One JSON line on stdout."""
import json
import sys
import time

sys.path.insert(0, ".")
from opencl_path_tracer_amd import api, scenes  # noqa: E402


def main():
    kw = dict(W=1920, H=1080, bounces=8, spp=16, reps=5, aperture=25.0, focus=1600.0)
    for a in sys.argv[1:]:
        k, v = a.split("=")
        kw[k] = type(kw[k])(v)
    spec = scenes.cornell_box()
    ctx = {}
    for name in ("lens", "pinhole"):
        sc = api.Scene(kw["W"], kw["H"]).load(spec)
        sc.iterations = kw["bounces"]
        if name == "lens":
            sc.set_lens(kw["aperture"], kw["focus"])
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
    for name in ctx:
        out[name + "_ms"] = ms[name]
        out[name + "_median_ms"] = sorted(ms[name])[len(ms[name]) // 2]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
