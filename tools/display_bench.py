"""The display stage (Scene.display, pt_display): its cost next to the byte model and next to pt_resolve_ldr, and the two pictures.

usage: python tools/display_bench.py [mode=time|loop|images] [W=1920 H=1080] [bounces=8] [spp=4] [reps=20] [levels=4] [outdir=DIR]

mode=time    the Cornell box at W x H: pt_display with the defaults (no bloom) and with bloom at `levels`: device time (HIP events around
             the call on the context's stream) and host time of the call itself (it only enqueues: no synchronise), each the median of
             `reps` after three warm-up calls, with minimum and maximum; pt_resolve_ldr(0) on the same frame (its read-back included, and
             its kernel alone by events); the byte model: every buffer read and written once per level.
mode=loop    `reps` calls of each of the two, nothing else: the program to put behind `rocprofv3 --kernel-trace --stats --` for the time
             of each kernel.
mode=images  64 x 64 scenes.sun_and_sky_light() over the Cornell box and scenes.light_shaft(), 64 spp of render_nee, each through despeckle ->
             denoise_despeckled -> display(source="denoised") with the defaults -> write_display_ppm into `outdir`; prints the metered numbers.
One JSON line on stdout."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from opencl_path_tracer_amd import api, scenes  # noqa: E402


def timed(sc, call, reps):
    """(device ms, host ms of the call) per repetition of call() after three warm-up calls"""
    dev, host = [], []
    for i in range(reps + 3):
        sc.sync()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        rc = call()
        t1 = time.perf_counter()
        e1.record()
        e1.synchronize()
        if rc != api.PT_OK:
            raise SystemExit("call failed: %d %s" % (rc, api.LIB.pt_last_error(sc._h)))
        if i >= 3:
            dev.append(e0.elapsed_time(e1))
            host.append((t1 - t0) * 1e3)
    return dev, host


def stats(ts):
    return {"median": float(np.median(ts)), "min": float(np.min(ts)), "max": float(np.max(ts))}


def byte_model(W, H, levels):
    """MB: the histogram reads the frame; the final kernel reads it, writes 16 + 3 B; with bloom the first level down reads the frame and
    every level is written once and read once by the next level down and once by the level up (which also rewrites the level it adds to)"""
    px = W * H
    no_bloom = px * (16 + 16 + 19)
    lv, w, h = [], W, H
    for _ in range(levels):
        w, h = (w + 1) // 2, (h + 1) // 2
        lv.append(w * h * 16)
    bloom = px * 16 + sum(lv) + sum(lv[:-1]) + sum(lv[1:]) + 2 * sum(lv[:-1]) + lv[0]
    return {"no_bloom_mb": no_bloom / 1e6, "bloom_mb": (no_bloom + bloom) / 1e6}


def cornell(W, H, bounces, spp):
    sc = api.Scene(W, H).load(scenes.cornell_box())
    sc.iterations = bounces
    sc.render(spp)
    sc.sync()
    return sc


def mode_time(kv):
    W, H, reps, levels = int(kv.get("W", 1920)), int(kv.get("H", 1080)), int(kv.get("reps", 20)), int(kv.get("levels", 4))
    sc = cornell(W, H, int(kv.get("bounces", 8)), int(kv.get("spp", 4)))
    res = {"W": W, "H": H, "levels": levels, "reps": reps, "model": byte_model(W, H, levels), "device_ms": {}, "host_call_ms": {}}
    plain = api.DisplayParams(**api.display_defaults())
    bloom = api.DisplayParams(**dict(api.display_defaults(), bloom_intensity=0.5, bloom_levels=levels))
    for name, p in (("display", plain), ("display_bloom", bloom)):
        dev, host = timed(sc, lambda: api.LIB.pt_display(sc._h, C.byref(p)), reps)
        res["device_ms"][name], res["host_call_ms"][name] = stats(dev), stats(host)
        res[name + "_info"] = sc.display_info()
    out = np.empty((sc.local_pixels, 4), dtype=np.float32)
    dev, host = timed(sc, lambda: api.LIB.pt_resolve_ldr(sc._h, 0, api._ptr(out), out.shape[0]), reps)
    res["device_ms"]["resolve_ldr_with_read_back"], res["host_call_ms"]["resolve_ldr_with_read_back"] = stats(dev), stats(host)
    sc.close()
    return res


def mode_loop(kv):
    sc = cornell(int(kv.get("W", 1920)), int(kv.get("H", 1080)), int(kv.get("bounces", 8)), int(kv.get("spp", 4)))
    for p in (dict(), dict(bloom_intensity=0.5, bloom_levels=int(kv.get("levels", 4)))):
        for _ in range(int(kv.get("reps", 20)) + 3):
            sc.display(**p)
        sc.sync()
    sc.resolve_ldr(0)
    sc.close()
    return {"mode": "loop"}


def mode_images(kv):
    outdir = kv.get("outdir", ".")
    os.makedirs(outdir, exist_ok=True)
    res = {}
    img, sun = scenes.sun_and_sky_light()

    def sunlit(sc):
        sc.set_environment(img)
        sc.set_area_lights([api.area_light_from(sun)])
    for name, spec, prepare in (("sun_and_sky_light", scenes.cornell_box(), sunlit), ("light_shaft", scenes.light_shaft(), None)):
        sc = api.Scene(64, 64).load(spec)
        if prepare:
            prepare(sc)
        sc.set_option("moments", 1)
        sc.iterations = 8
        sc.render_nee(64, "mis")
        sc.render_aovs()
        sc.despeckle()
        sc.denoise_despeckled()
        sc.display(source="denoised")
        info = sc.display_info()
        rgb8 = sc.read_display()[1]
        sc.write_display_ppm(os.path.join(outdir, "display_%s.ppm" % name))
        ldr = sc.resolve_ldr(0)[:, :3]
        res[name] = dict(info, mean_byte=float(rgb8.mean()), share_0=float((rgb8 == 0).mean()), share_255=float((rgb8 == 255).mean()),
                         resolve_ldr_share_nan=float(np.isnan(ldr).mean()), resolve_ldr_share_above_0_99=float((np.nan_to_num(ldr) > 0.99).mean()),
                         resolve_ldr_mean=float(np.nan_to_num(ldr).clip(0, 1).mean()))
        sc.close()
    return res


def main():
    kv = dict(a.split("=", 1) for a in sys.argv[1:])
    mode = kv.get("mode", "time")
    if mode not in ("time", "loop", "images"):
        raise SystemExit("mode must be time, loop or images")
    print(json.dumps({"time": mode_time, "loop": mode_loop, "images": mode_images}[mode](kv)), flush=True)


if __name__ == "__main__":
    main()
