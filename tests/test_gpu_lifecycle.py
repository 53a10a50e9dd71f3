"""-m gpu: the life cycle of a context's device arrays (csrc/pt_devbuf.hpp owns them; pt_destroy frees none by hand).

  (a) one context renders a scene, a larger one, and the larger one uploaded again: the shading records, the packed vertex normals and
      the packed uvs grow at the second upload and are reused at the third; every frame equals, bit for bit, the frame of a fresh
      context that saw only that scene.  Authoring only appends (no call removes a triangle), so a context cannot go back to the
      smaller scene: the third upload is of the same size, which is the path that keeps the arrays it has.
  (b) a context touches every array that is allocated on first use, renders into torch tensors bound with bind_framebuffer and is
      destroyed, four times in one process; the tensors outlive it with the last frame in them.

All frames 16 x 16, 4 samples, 3 iterations."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = H = 16
SPP, BOUNCES = 4, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def small_box(scenes):
    return scenes.cornell_box(segments=8, rings=4, smooth=True, textured=True)


def extra_sphere(scenes):
    """What the second upload adds: a diffuse sphere with its analytic normals and uvs, more triangles than the box has."""
    centre, radius, seg, rings = (500.0, 650.0, 100.0), 150.0, 16, 8
    verts = scenes.uv_sphere(centre, radius, seg, rings)
    return (verts, np.full(verts.shape[0], scenes.WHITE_DIFFUSE, dtype=np.uint16), scenes.uv_sphere_normals(centre, radius, seg, rings),
            scenes.uv_sphere_uvs(rings, seg))


def larger_box(scenes):
    spec = small_box(scenes)
    verts, mati, normals, uvs = extra_sphere(scenes)
    spec.objects.append((verts, mati))
    spec.normals = list(spec.normals) + [normals]
    spec.uvs = list(spec.uvs) + [uvs]
    return spec


def frame(sc, nee):
    """The same seeds and a new frame for every render."""
    sc.seed_default()
    sc.current_sample = 0
    sc.iterations = BOUNCES
    if nee:
        sc.render_nee(SPP, "mis")
    else:
        sc.render(SPP)
    return sc.read_colors().copy(), sc.read_rnds().copy()


@pytest.mark.parametrize("nee", [False, True])
def test_uploads_grow_and_reuse_the_scene_arrays(api, nee):
    from opencl_path_tracer_amd import scenes

    def context():
        sc = api.Scene(W, H)
        if nee:
            sc.set_option("smooth_normals", 1)
            sc.set_option("textures", 1)
        return sc

    want = {}
    for name, spec in (("small", small_box(scenes)), ("larger", larger_box(scenes))):
        with context().load(spec) as fresh:
            want[name] = frame(fresh, nee)
    assert not same_bits(want["small"][0], want["larger"][0])      # (the sphere is in view: the two scenes are told apart)

    with context().load(small_box(scenes)) as sc:
        n_small = small_box(scenes).ntris
        got = frame(sc, nee)
        assert same_bits(got[0], want["small"][0]) and np.array_equal(got[1], want["small"][1])
        verts, mati, normals, uvs = extra_sphere(scenes)
        assert verts.shape[0] > n_small
        sc.add_Triangles(api.triangles_from_vertices(verts, mati))
        sc.end_Obj()
        sc.set_vertex_normals(normals, first=n_small)
        sc.set_vertex_uvs(uvs, first=n_small)
        sc.upload_Triangles()                                        # every per-triangle array grows
        sc.upload_Materials()
        got = frame(sc, nee)
        assert same_bits(got[0], want["larger"][0]) and np.array_equal(got[1], want["larger"][1])
        sc.upload_Triangles()                                        # the same size again: rebuilt in the arrays that are there
        sc.upload_Materials()
        got = frame(sc, nee)
        assert same_bits(got[0], want["larger"][0]) and np.array_equal(got[1], want["larger"][1])


_LAZY_CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np, torch
from opencl_path_tracer_amd import api, scenes
W = H = 16
SPP, BOUNCES = 4, 3
torch.cuda.init()
kept = []
for cycle in range(4):
    spec = scenes.cornell_box(segments=8, rings=4, smooth=True, textured=True)
    nee = scenes.cornell_box(segments=8, rings=4, fog=1e-3, density=scenes.smoke_plume(8), tint=(0.8, 0.9, 0.7))
    sc = api.Scene(W, H).load(spec)
    sc.iterations = BOUNCES
    sc.set_option("moments", 1)
    sc.set_option("count_work", 1)                       # the per-tile cost array
    sc.set_option("chunk_spp", 2)                        # chained passes: the per-tile pass counters
    sc.render(SPP)
    sc.debug_tile_cost()
    sc.render_aovs()                                     # guides, then every filter and read-out that allocates on first use
    sc.denoise()
    sc.read_variance()
    sc.denoise_variance()
    sc.temporal_accumulate()
    sc.denoise_temporal()
    sc.resolve_ldr(0)
    sc.current_sample = 0
    sc.render_adaptive(2, 8, 0.05)                       # an adaptive frame (with its half-way snapshot)
    sc.current_sample = 0
    sc.set_option("variant", 1)                          # the wavefront variant: path state, queues, counters
    sc.render(SPP)
    sc.set_option("variant", 0)
    sc.set_option("smooth_normals", 1)                   # and what only the NEE path reads
    sc.set_option("textures", 1)
    sc.set_option("light_tree", 1)
    sc.set_environment(scenes.sun_and_sky(width=16, height=8))
    sc.set_lights([api.point_light((500.0, 900.0, 0.0), (3e5, 3e5, 3e5))], select=0.4)
    sc.set_medium(**nee.medium)
    sc.set_medium_density(nee.medium_density)
    for material, kw in nee.interiors.items():
        sc.set_material_interior(material, **kw)
    sc.current_sample = 0
    sc.render_nee(SPP, "mis")
    assert sc.stat("nee_family") >= 0
    colors = torch.zeros((sc.slab_pixels, 4), dtype=torch.float32, device="cuda:0")
    rnds = torch.zeros((sc.slab_pixels,), dtype=torch.int32, device="cuda:0")
    sc.bind_framebuffer(colors.data_ptr(), rnds.data_ptr())
    sc.current_sample = 0
    sc.render_nee(SPP, "mis")                            # the last frame, into the caller's arrays
    last_c, last_r = sc.read_colors().copy(), sc.read_rnds().copy()
    assert float(np.abs(last_c[:, :3]).sum()) > 0
    sc.close()                                           # must not free what it borrowed
    torch.cuda.synchronize()
    kept.append((colors, rnds, last_c, last_r))
for colors, rnds, last_c, last_r in kept:                # every cycle's tensors, after every context is gone
    assert np.array_equal(colors.cpu().numpy().view(np.uint32), last_c.view(np.uint32))
    assert np.array_equal(rnds.cpu().numpy(), last_r)
print("LIFECYCLE_OK")
"""


def test_lazy_arrays_and_a_borrowed_framebuffer_over_four_contexts():
    """In a child process, as the other tests that put torch next to the library do."""
    out = subprocess.run([sys.executable, "-c", _LAZY_CHILD % {"root": ROOT}], capture_output=True, text=True, timeout=300)
    assert "LIFECYCLE_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
