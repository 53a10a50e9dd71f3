"""Rate of the megakernel in launch shapes other than the headline's, one k_render instance each, for A/B runs of two builds.

usage (from the root of the tree whose library is measured): python <path>/launch_shape_ab.py [reps=3] [spp=64] [only=name,...]

Per shape: the instance the launch policy picked (threads per workgroup, waves per SIMD, schedule, samples per item), Msamples/s from
HIP-event kernel time over `reps` launches of `spp` samples after one warm-up launch, and a checksum of colours + LCG states, so that
two builds can be compared for speed and for results.  A rank of a tiled context (world > 1) renders its own rows on this one GPU: the
launch shape a rank of an N-GPU job gets."""
import hashlib
import sys
import time

sys.path.insert(0, ".")
from opencl_path_tracer_amd import api, scenes  # noqa: E402

PRE = ("treelet", "lds_scene", "wide_nodes", "wide_lds_entries")         # options the upload depends on
SHAPES = [
    # name, scene, world, options
    ("cb_sched0", "cornell", 1, {"schedule": 0}),
    ("cb_sched1", "cornell", 1, {"schedule": 1}),
    ("cb_rank_of_2", "cornell", 2, {}),
    ("cb_rank_of_4", "cornell", 4, {}),
    ("cb_rank_of_8", "cornell", 8, {}),
    ("cb_block512_sched1", "cornell", 1, {"lds_block": 512, "schedule": 1}),
    ("cb_block512_sched2", "cornell", 1, {"lds_block": 512, "schedule": 2}),
    ("mesh_default", "mesh100k", 1, {}),
    ("mesh_sched1", "mesh100k", 1, {"schedule": 1}),
    ("mesh_sched1_wps6", "mesh100k", 1, {"schedule": 1, "waves_per_simd": 6}),
    ("mesh_sched1_wps5", "mesh100k", 1, {"schedule": 1, "waves_per_simd": 5}),
    ("mesh_bvh2_sched1", "mesh100k", 1, {"wide_nodes": 0, "schedule": 1}),
    ("mesh_bvh2_sched1_wps6", "mesh100k", 1, {"wide_nodes": 0, "schedule": 1, "waves_per_simd": 6}),
    ("mesh_bvh2_sched1_wps4", "mesh100k", 1, {"wide_nodes": 0, "schedule": 1, "waves_per_simd": 4}),
    ("mesh_bvh2_sched2_wps5", "mesh100k", 1, {"wide_nodes": 0, "schedule": 2, "waves_per_simd": 5}),
]


def main():
    a = dict(kv.split("=", 1) for kv in sys.argv[1:])
    reps, spp = int(a.get("reps", 3)), int(a.get("spp", 64))
    only = set(a["only"].split(",")) if "only" in a else None
    specs = {}
    W, H = 1920, 1080
    for name, scene, world, opts in SHAPES:
        if only and name not in only:
            continue
        if scene not in specs:
            specs[scene] = scenes.cornell_box() if scene == "cornell" else scenes.displaced_grid_mesh(100000)
        sc = api.Scene(W, H, rank=0, world=world)
        for k in PRE:
            if k in opts:
                sc.set_option(k, opts[k])
        sc.load(specs[scene])
        for k, v in opts.items():
            if k not in PRE:
                sc.set_option(k, v)
        sc.iterations = 8
        plan = sc.debug_launch_plan(spp)
        sc.set_option("timing", 1)
        sc.render(spp)
        sc.sync()
        sc.set_option("reset_stats", 1)
        t0 = time.perf_counter()
        for _ in range(reps):
            sc.render(spp)
        sc.sync()
        wall = time.perf_counter() - t0
        samples, kms = sc.stat("samples"), sc.stat("kernel_ms")
        digest = hashlib.sha1(sc.read_colors().tobytes() + sc.read_rnds().tobytes()).hexdigest()[:12]
        print("%-24s block %4d wps %d sched %d chunk %2d tiles %6d | %8.1f Msamples/s (kernel) %8.1f (wall) | %s" % (
            name, plan["block"], plan["waves_per_simd"], plan["schedule"], plan["chunk_spp"], plan["tiles"],
            samples / kms / 1e3, samples / wall / 1e6, digest), flush=True)
        sc.close()


if __name__ == "__main__":
    main()
