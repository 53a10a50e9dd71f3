"""Test helper: the scenes of test_wallpair_host.py / test_gpu_wallpair.py and the frozen packed lists of
tests/golden/wallpair_lists.npz.  Scene data only.

Run as a script to rewrite the golden file from the library in the tree (packets, ranks and meta of the big-triangle
list do not depend on pairing, so any build gives the same file; it was first written by the build before pairing)."""
import copy
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "wallpair_lists.npz")


def _with_walls(cb_spec, walls):
    spec = copy.copy(cb_spec)
    spec.objects = [(np.ascontiguousarray(walls, dtype=np.float32), cb_spec.objects[0][1])] + list(cb_spec.objects[1:])
    return spec


def tilted_wall(cb_spec):
    """The Cornell box with its far wall leaning back by 10 units at the top: the halves still share a box and the diagonal,
    but not r1, and the plane is not axis-aligned -- no corner of theirs may be exchanged for another, so they stay unpaired."""
    walls = cb_spec.objects[0][0].copy()
    far = walls[2:4]
    far[..., 2] = np.where(far[..., 1] == 1000.0, 1010.0, 1000.0)
    return _with_walls(cb_spec, walls)


def swapped_halves(cb_spec):
    """The Cornell box with the halves of the left wall authored in the other order."""
    walls = cb_spec.objects[0][0].copy()
    walls[[4, 5]] = walls[[5, 4]]
    return _with_walls(cb_spec, walls)


def _sphere_under(quads, mats):
    from opencl_path_tracer_amd import scenes
    sph = scenes.uv_sphere((0.0, 50.0, 0.0), 20.0, 8, 4)
    return scenes.SceneSpec(materials=list(scenes.BUILTIN_MATERIALS),
                            objects=[(np.asarray(quads, dtype=np.float32), np.asarray(mats, dtype=np.uint16)),
                                     (sph, np.full(sph.shape[0], 2, dtype=np.uint16))], name="wallpair")


def one_quad():
    """A floor quad (two big triangles, listed) under a small sphere (the tree)."""
    a, b, c, d = (-500.0, 0.0, -500.0), (-500.0, 0.0, 500.0), (500.0, 0.0, 500.0), (500.0, 0.0, -500.0)
    return _sphere_under([(a, b, c), (c, d, a)], [2, 2])


def lone_triangle():
    a, b, c = (-500.0, 0.0, -500.0), (-500.0, 0.0, 500.0), (500.0, 0.0, 500.0)
    return _sphere_under([(a, b, c)], [2])


def load_host_only(api, spec, perturb_normal_of=None):
    """A host-only context with `spec` built; perturb_normal_of = k: triangle k of the first object gets the largest component
    of its normal moved by one ulp before it is added."""
    sc = api.Scene(32, 32, device=None)
    for m in spec.materials:
        sc.add_Material(*m)
    for k, (verts, mati) in enumerate(spec.objects):
        recs = api.triangles_from_vertices(verts, mati)
        if k == 0 and perturb_normal_of is not None:
            n = recs["N"][perturb_normal_of]
            j = int(np.argmax(np.abs(n[:3])))
            n[j] = np.nextafter(n[j], np.float32(0.0))
        sc.add_Triangles(recs)
        sc.end_Obj()
    sc.upload_Triangles()
    sc.upload_Materials()
    return sc


def host_cases(cb_spec):
    """name -> (spec, triangle whose normal is perturbed or None)"""
    return {"cornell": (cb_spec, None), "tilted": (tilted_wall(cb_spec), None), "swapped": (swapped_halves(cb_spec), None),
            "quad": (one_quad(), None), "quad_ulp": (one_quad(), 1), "lone": (lone_triangle(), None)}


def packed_list(sc):
    nf = int(sc.stat("flat_triangles"))
    _, tris, meta, orig = sc.debug_bvh()
    return {"n_flat": np.int64(nf), "tris": tris[:nf].copy(), "meta": meta.copy(), "orig": orig.copy()}


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(HERE))
    from opencl_path_tracer_amd import api, scenes
    out = {}
    for name, (spec, pert) in host_cases(scenes.cornell_box()).items():
        for k, v in packed_list(load_host_only(api, spec, pert)).items():
            out["%s_%s" % (name, k)] = v
    np.savez_compressed(GOLDEN, **out)
    print({k: v.shape for k, v in out.items()})
