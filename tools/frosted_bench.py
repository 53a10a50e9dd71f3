"""Rough dielectric (option frosted): launch time of render_nee on the Cornell box with the frosted sphere against the glass sphere.

usage: python tools/frosted_bench.py [W=1920 H=1080] [bounces=8] [spp=16] [reps=5] [aperture=25] [focus=1600]

The Cornell box, render_nee(spp, "mis") through a lens (so that both frames run the same launch shape): wall clock around one launch and
a sync, after one warm-up launch per context; `reps` launches each, the two contexts alternating (frosted: cornell_box(frosted=True) with
the option on, k_nee<kNeeFrosted>; glass: cornell_box() on the lens-family kernels, k_nee<kNeeLens>).  One JSON line on stdout."""
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
    ctx = {}
    for name in ("frosted", "glass"):
        sc = api.Scene(kw["W"], kw["H"]).load(scenes.cornell_box(frosted=name == "frosted"))
        sc.iterations = kw["bounces"]
        sc.set_lens(kw["aperture"], kw["focus"])
        if name == "frosted":
            sc.set_option("frosted", 1)
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
