"""Next-event estimation (render_nee): rate, kernel time per path segment, and what each strategy buys in RMSE.

usage: python tools/nee_bench.py [--smooth] [--textured | --textures-on] [scene=cornell|walls|mesh100k|all] [W=1920 H=1080] [bounces=8] [ref=4096] [spp=64] [quality=1] [out=DIR]

--smooth: the Cornell box carries its spheres' analytic vertex normals and render_nee runs with option smooth_normals = 1 (render(),
which refuses under the option, runs with it off); quality=0 skips the reference frame and the RMSE curve (rates only).
--textured: the Cornell box carries its checker floor (scenes.cornell_box(textured=True)) and render_nee runs with option textures = 1;
--textures-on: option textures = 1 on the untextured scene (what the textured kernel instances cost by themselves); rates only make sense
with quality=0 here (the reference frame of the quality part is render()'s, which has no textures).

One JSON line per scene on stdout; with out=DIR also DIR/<scene>_<W>x<H>.json.

Per scene, at W x H and `bounces` bounces:
  * Msamples/s of render(spp) and of render_nee(spp) in each strategy (HIP events around the call alone, re-seeding done and
    synchronised before the first event; median of 3 after a warm-up; the library's own launch events, stat kernel_ms, alongside),
    and the kernel time per path segment: the segments are those of render(spp) from the same seeds (stat "segments"), which
    every strategy traces (the light samples never touch the LCG, so the BSDF paths are the same); LIGHT and MIS add one shadow
    ray at every lobe vertex that is not on the last segment;
  * RMSE at 4 / 16 / 64 spp against a `ref`-spp render() frame (other seeds), the efficiency 1 / (MSE x kernel time) at each, and
    the RMSE at equal time: RMSE(16 spp) x sqrt(t_strategy / t_render) (MSE falls as 1 / spp, so a strategy that costs k times
    the time per sample reaches that RMSE in render()'s time)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from opencl_path_tracer_amd import api, scenes  # noqa: E402

STRATEGIES = ("bsdf", "light", "mis")


def scene_spec(name, smooth=False, textured=False):
    if name == "cornell":
        return scenes.cornell_box(smooth=smooth, textured=textured)
    if name == "walls":
        spec = scenes.SceneSpec(materials=list(scenes.BUILTIN_MATERIALS), name="cornell_walls")
        spec.objects.append(scenes.cornell_walls())
        return spec
    if name == "mesh100k":
        return scenes.displaced_grid_mesh(100000)
    raise SystemExit("scene must be cornell, walls, mesh100k or all")


def rmse(a, b):
    d = a[:, :3].astype(np.float64) - b[:, :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def timed(sc, fn, setup, reps=3):
    """Median over `reps` calls of fn(), after a warm-up, of (ms between two HIP events on the null stream -- the library's
    default -- around fn() alone, ms of the library's own launch events: stat kernel_ms with option timing = 1).  setup()
    (re-seeding: host work and a synchronising copy) runs and is synchronised BEFORE the first event."""
    setup()
    fn()
    torch.cuda.synchronize()
    ev, kern = [], []
    for _ in range(reps):
        setup()
        torch.cuda.synchronize()
        k0 = sc.stat("kernel_ms")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
        kern.append(sc.stat("kernel_ms") - k0)
    return float(np.median(ev)), float(np.median(kern))


def run_scene(name, W, H, bounces, ref_spp, spp, smooth=False, quality=True, textures=0):
    spec = scene_spec(name, smooth, textures == 2)
    npix = W * H
    res = {"scene": name, "W": W, "H": H, "bounces": bounces, "ref_spp": ref_spp, "rate_spp": spp, "smooth": bool(smooth), "textures": ("off", "on", "on, textured scene")[textures]}

    def nee(sc, n, s):
        sc.set_option("smooth_normals", 1 if smooth else 0)
        sc.set_option("textures", 1 if textures else 0)
        sc.render_nee(n, s)
        sc.set_option("smooth_normals", 0)
        sc.set_option("textures", 0)

    def ctx(seed=None):
        sc = api.Scene(W, H, device=0).load(spec)
        sc.iterations = bounces
        if seed is not None:
            sc.upload_seeds(np.random.default_rng(seed).integers(1, 2 ** 31 - 2, npix).astype(np.int32))
        return sc

    gt = None
    if quality:
        sc = ctx(seed=12345)
        if smooth:
            nee(sc, ref_spp, "mis")            # the reference of a smooth frame is a smooth frame
        else:
            sc.render(ref_spp)
        gt = sc.read_colors()
        sc.close()
    sc = ctx()
    res["lights"] = int(len(sc.debug_light_table()[0]))

    # ---- rates and time per segment (every call starts from the default seeds: the same paths)
    sc.set_option("reset_stats", 1)
    sc.render(spp)
    segs = float(sc.stat("segments"))
    res["segments_per_sample"] = segs / (npix * spp)

    def reseed():
        sc.seed_default()
        sc.current_sample = 0
    sc.set_option("timing", 1)
    rates = {}

    def rate(key, fn):
        ms, kms = timed(sc, fn, reseed)
        rates[key] = {"ms": ms, "kernel_ms": kms, "msamples_s": npix * spp / (ms * 1e-3) / 1e6, "ns_per_segment": ms * 1e6 / segs}
    rate("render", lambda: sc.render(spp))
    for s in STRATEGIES:
        rate("nee_" + s, lambda s=s: nee(sc, spp, s))
    res["rates"] = rates
    sc.close()
    if not quality:
        return res

    # ---- quality
    curve = {}
    for n in (4, 16, 64):
        row = {}
        for s in ("render",) + STRATEGIES:
            sc = ctx()
            if s == "render":
                sc.render(n)
            else:
                nee(sc, n, s)
            e = rmse(sc.read_colors(), gt)
            t = rates["render" if s == "render" else "nee_" + s]["ms"] * n / spp
            row[s] = {"rmse": e, "ms": t, "efficiency": 1.0 / (e * e * t * 1e-3)}
            sc.close()
        curve[n] = row
    res["curve"] = curve
    t0 = rates["render"]["ms"]
    res["rmse16_equal_time"] = {s: curve[16][s]["rmse"] * float(np.sqrt((rates["nee_" + s]["ms"] if s != "render" else t0) / t0))
                                for s in ("render",) + STRATEGIES}
    res["mis_over_bsdf_rmse16"] = curve[16]["mis"]["rmse"] / curve[16]["bsdf"]["rmse"]
    return res


def main():
    smooth = "--smooth" in sys.argv[1:]
    textures = 2 if "--textured" in sys.argv[1:] else 1 if "--textures-on" in sys.argv[1:] else 0
    a = dict(kv.split("=", 1) for kv in sys.argv[1:] if not kv.startswith("--"))
    names = ["cornell", "walls", "mesh100k"] if a.get("scene", "all") == "all" else [a["scene"]]
    W, H, B = int(a.get("W", 1920)), int(a.get("H", 1080)), int(a.get("bounces", 8))
    ref, spp = int(a.get("ref", 4096)), int(a.get("spp", 64))
    out_dir = a.get("out")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    for name in names:
        r = run_scene(name, W, H, B, ref, spp, smooth, int(a.get("quality", 1)) != 0, textures)
        print(json.dumps(r), flush=True)
        if out_dir:
            with open(os.path.join(out_dir, "%s%s%s_%dx%d.json" % (name, "_smooth" if smooth else "", ("", "_texopt", "_textured")[textures], W, H)), "w") as f:
                json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
