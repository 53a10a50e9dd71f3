"""Environment lighting (Scene.set_environment + render_nee): what it costs when no sky is set, and a sky-lit frame.

usage: python tools/env_bench.py mode=nosky|sky [W=1920 H=1080] [bounces=8] [spp=64] [reps=7] [ref=4096] [out=FILE]

One JSON line on stdout (and into out=FILE).
  mode=nosky  render_nee(spp, "mis") on the Cornell box with no environment: `reps` timings (HIP events around the call alone,
              re-seeding synchronised before the first event, after a warm-up), their median and spread.  For an A/B against
              another commit run it once per tree and alternate: PTAMD_TREE=<root of the other checkout, built> selects the
              package the script imports (the default is this tree); the symbols differ between commits, so PTAMD_LIB alone is
              not enough.
  mode=sky    MESH-100k without its lamp under scenes.sun_and_sky(): the time of render_nee(spp) in each strategy, and the RMSE of
              16-spp BSDF and MIS frames against a `ref`-spp BSDF frame from other seeds."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.environ.get("PTAMD_TREE", "."))
from opencl_path_tracer_amd import api, scenes  # noqa: E402


def timed(sc, fn, reps):
    def reseed():
        sc.seed_default()
        sc.current_sample = 0
    reseed()
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        reseed()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def summary(ms):
    return {"ms": ms, "median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}


def rmse(a, b):
    d = a[:, :3].astype(np.float64) - b[:, :3].astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def main():
    a = dict(kv.split("=", 1) for kv in sys.argv[1:])
    mode = a.get("mode", "nosky")
    W, H, B = int(a.get("W", 1920)), int(a.get("H", 1080)), int(a.get("bounces", 8))
    spp, reps, ref_spp = int(a.get("spp", 64)), int(a.get("reps", 7)), int(a.get("ref", 4096))
    res = {"mode": mode, "W": W, "H": H, "bounces": B, "spp": spp, "library": api._LIB_PATH}
    if mode == "nosky":
        sc = api.Scene(W, H, device=0).load(scenes.cornell_box())
        sc.iterations = B
        res.update(summary(timed(sc, lambda: sc.render_nee(spp, "mis"), reps)))
    elif mode == "sky":
        spec = scenes.displaced_grid_mesh(100000)
        verts, mati = spec.objects[0]
        spec.objects[0] = (verts[2:], mati[2:])                      # the lamp's two triangles
        sky = scenes.sun_and_sky()

        def ctx(seed=None):
            sc = api.Scene(W, H, device=0).load(spec)
            sc.set_environment(sky)
            sc.iterations = B
            if seed is not None:
                sc.upload_seeds(np.random.default_rng(seed).integers(1, 2 ** 31 - 2, W * H).astype(np.int32))
            return sc
        sc = ctx()
        res["P_env"] = sc.debug_environment()["P_env"]
        res["rates"] = {s: summary(timed(sc, lambda s=s: sc.render_nee(spp, s), 3)) for s in ("bsdf", "light", "mis")}
        sc.close()
        sc = ctx(seed=12345)
        sc.render_nee(ref_spp, "bsdf")
        gt = sc.read_colors()
        sc.close()
        res["rmse16"] = {}
        for s in ("bsdf", "light", "mis"):
            sc = ctx()
            sc.render_nee(16, s)
            res["rmse16"][s] = rmse(sc.read_colors(), gt)
            sc.close()
        res["mis_over_bsdf_rmse16"] = res["rmse16"]["mis"] / res["rmse16"]["bsdf"]
    else:
        raise SystemExit("mode must be nosky or sky")
    print(json.dumps(res), flush=True)
    if a.get("out"):
        with open(a["out"], "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
