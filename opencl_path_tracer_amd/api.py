"""Host-side mirror of the reference's `Scene` class (main.cpp:363-742) over the C ABI of
libptamd.so (include/pt_api.h).  Same method names, same call order, same argument meaning:

    scene = Scene(width, height)            # Scene::init_Scene
    m = scene.add_Material(kd, ks, emission, N, K, shininess, type)
    scene.add_Triangle(r1, r2, r3, m); ...; scene.end_Obj()
    scene.upload_Triangles(); scene.upload_Materials()
    scene.render()                          # generate_rays + trace_rays, current_sample++

The reference keeps its parameters in globals (iterations, global_fov/yaw/pitch/shift,
current_sample: main.cpp:27-39); here they are attributes of the Scene object.

There is no CPU path: if libptamd.so is missing this module raises at import, and a Scene on a
machine without a gfx950 device raises at construction (device=None asks for a host-only
context that can author scenes and build the BVH but cannot render).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PTAMD_LIB: an A/B build of the same library (`make ab`), for kernel experiments only
_LIB_PATH = os.environ.get("PTAMD_LIB") or os.path.join(_HERE, "libptamd.so")

PT_OK, PT_EINVAL, PT_ENODEVICE, PT_EHIP, PT_ESCENE, PT_EIO, PT_ECOMM = 0, -1, -2, -3, -4, -5, -6
PT_COMM_ID_BYTES = 128

MATERIAL = np.dtype([("kd", "<f4", 4), ("ks", "<f4", 4), ("emission", "<f4", 4), ("F0", "<f4", 4),
                     ("n", "<f4"), ("shininess", "<f4"), ("type", "<i4"), ("_pad", "<i4")])
RAY = np.dtype([("P", "<f4", 4), ("D", "<f4", 4)])
# Node4q (csrc/pt_internal.hpp): byte k of a q word is child k's plane on the node's grid, plane = origin + q * 2^(exp - 127)
WIDE_NODE = np.dtype([("origin", "<f4", 3), ("exp", "u1", 3), ("nchild", "u1"), ("q", "u1", (6, 4)), ("spare", "<u4", 2), ("ref", "<i4", 4)])
assert WIDE_NODE.itemsize == 64
TRIANGLE = np.dtype([("r1", "<f4", 4), ("r2", "<f4", 4), ("r3", "<f4", 4), ("N", "<f4", 4),
                     ("mati", "<u2"), ("_pad", "u1", 14)])
CAMERA = np.dtype([("eye", "<f4", 4), ("lookat", "<f4", 4), ("up", "<f4", 4), ("right", "<f4", 4),
                   ("XM", "<f4"), ("YM", "<f4"), ("_pad", "<f4", 2)])
assert MATERIAL.itemsize == 80 and RAY.itemsize == 32 and TRIANGLE.itemsize == 80 and CAMERA.itemsize == 80

# every symbol include/pt_api.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "pt_material_init", "pt_triangle_init", "pt_triangles_init", "pt_camera_init", "pt_camera_move", "pt_create", "pt_create_tiled", "pt_destroy",
    "pt_last_error", "pt_device_info", "pt_add_material", "pt_add_triangle", "pt_add_triangles", "pt_end_obj",
    "pt_add_obj", "pt_upload_triangles", "pt_upload_materials", "pt_seed_default", "pt_upload_seeds",
    "pt_generate_rays", "pt_trace_rays", "pt_render", "pt_render_adaptive", "pt_adaptive_defaults", "pt_render_adaptive_ex", "pt_read_sample_counts", "pt_read_tile_state", "pt_adaptive_rounds",
    "pt_set_current_sample", "pt_get_current_sample", "pt_sync",
    "pt_render_nee", "pt_nee_rand", "pt_debug_light_table",
    "pt_set_vertex_normals", "pt_clear_vertex_normals", "pt_compute_vertex_normals", "pt_debug_vertex_normals", "pt_debug_shading_normal",
    "pt_texture_defaults", "pt_add_texture", "pt_clear_textures", "pt_set_material_texture", "pt_debug_texture",
    "pt_set_vertex_uvs", "pt_clear_vertex_uvs", "pt_debug_vertex_uvs", "pt_debug_albedo", "pt_image_read_ppm",
    "pt_material_roughness", "pt_debug_glossy", "pt_debug_coated", "pt_debug_frosted",
    "pt_lens_defaults", "pt_set_lens", "pt_clear_lens", "pt_focus_at", "pt_debug_lens",
    "pt_environment_defaults", "pt_set_environment", "pt_clear_environment", "pt_env_lookup", "pt_debug_environment", "pt_image_read_pfm",
    "pt_lights_defaults", "pt_set_lights", "pt_clear_lights", "pt_debug_lights",
    "pt_area_lights_defaults", "pt_set_area_lights", "pt_clear_area_lights", "pt_debug_area_lights", "pt_debug_area_light_eval",
    "pt_medium_defaults", "pt_set_medium", "pt_clear_medium", "pt_get_medium", "pt_debug_medium",
    "pt_set_medium_density", "pt_clear_medium_density", "pt_debug_medium_density", "pt_debug_grid",
    "pt_interior_defaults", "pt_set_material_interior", "pt_clear_material_interiors", "pt_get_material_interior", "pt_debug_interior",
    "pt_debug_light_tree", "pt_debug_light_tree_eval",
    "pt_read_variance", "pt_device_variance", "pt_denoise_variance_defaults", "pt_denoise_variance",
    "pt_temporal_defaults", "pt_temporal_accumulate", "pt_read_temporal", "pt_device_temporal", "pt_denoise_temporal", "pt_debug_reproject",
    "pt_despeckle_defaults", "pt_despeckle", "pt_read_despeckled", "pt_device_despeckled", "pt_denoise_despeckled", "pt_debug_despeckle",
    "pt_display_defaults", "pt_display", "pt_read_display", "pt_device_display", "pt_display_info", "pt_debug_display_histogram",
    "pt_display_reset", "pt_write_display_ppm", "pt_debug_display",
    "pt_render_aovs", "pt_read_aovs", "pt_aov_defaults", "pt_render_aovs_ex", "pt_denoise_defaults", "pt_denoise", "pt_read_denoised", "pt_device_denoised",
    "pt_local_pixel_count", "pt_local_pixel_ids", "pt_read_colors", "pt_read_rnds", "pt_read_rays",
    "pt_resolve_ldr", "pt_bind_framebuffer", "pt_device_colors", "pt_device_rnds", "pt_set_stream",
    "pt_set_option", "pt_get_stat", "pt_debug_bvh_sizes", "pt_debug_bvh_copy", "pt_debug_wide_nodes", "pt_debug_flat_list", "pt_debug_encounter_rank", "pt_debug_tile_cost", "pt_debug_adaptive_list", "pt_debug_launch_plan",
    "pt_debug_scene_sizes", "pt_debug_scene_copy", "pt_debug_closest_hit", "pt_debug_math", "pt_debug_spec", "pt_debug_shade",
    "pt_slab_pixel_count", "pt_frame_size", "pt_comm_available", "pt_comm_unique_id", "pt_comm_init", "pt_gather_frame", "pt_device_frame", "pt_read_frame",
    "pt_write_pfm", "pt_write_ppm", "pt_image_write_pfm", "pt_image_write_ppm", "pt_debug_gather_index", "pt_debug_deinterleave",
]


class PtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libptamd: %s (code %d)" % (msg, code))
        self.code = code


def _load():
    if not os.path.exists(_LIB_PATH):
        raise ImportError("libptamd.so is not built (run `make` or __graft_entry__.build()); "
                          "there is no fallback implementation")
    L = C.CDLL(_LIB_PATH)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    fp = C.POINTER(C.c_float)

    def sig(name, res, *args):
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = list(args)

    sig("pt_material_init", None, vp, fp, fp, fp, fp, fp, f32, i32)
    sig("pt_triangle_init", None, vp, fp, fp, fp, C.c_uint16)
    sig("pt_triangles_init", None, vp, vp, vp, i64)
    sig("pt_camera_init", None, vp, f32, f32, f32, fp, i32, i32)
    sig("pt_camera_move", None, fp, f32, f32, f32, f32, f32)
    sig("pt_create", C.c_int, C.c_int, i32, i32, C.POINTER(vp))
    sig("pt_create_tiled", C.c_int, C.c_int, i32, i32, i32, i32, i32, C.POINTER(vp))
    sig("pt_destroy", None, vp)
    sig("pt_last_error", C.c_char_p, vp)
    sig("pt_device_info", C.c_int, vp, C.c_char_p, i32)
    sig("pt_add_material", C.c_int, vp, vp)
    sig("pt_add_triangle", C.c_int, vp, vp)
    sig("pt_add_triangles", C.c_int, vp, vp, i64)
    sig("pt_end_obj", C.c_int, vp)
    sig("pt_add_obj", C.c_int, vp, C.c_char_p, fp, fp, f32, f32)
    sig("pt_upload_triangles", C.c_int, vp)
    sig("pt_upload_materials", C.c_int, vp)
    sig("pt_seed_default", C.c_int, vp)
    sig("pt_upload_seeds", C.c_int, vp, vp, i64)
    sig("pt_generate_rays", C.c_int, vp, vp)
    sig("pt_trace_rays", C.c_int, vp, vp, i32, i32)
    sig("pt_render", C.c_int, vp, vp, i32, i32)
    sig("pt_render_adaptive", C.c_int, vp, vp, i32, i32, i32, f32)
    sig("pt_adaptive_defaults", None, vp)
    sig("pt_render_adaptive_ex", C.c_int, vp, vp, i32, vp)
    sig("pt_read_sample_counts", C.c_int, vp, vp, i64)
    sig("pt_read_tile_state", C.c_int, vp, vp, vp, i64)
    sig("pt_adaptive_rounds", C.c_int, i32, i32, vp, i32, C.POINTER(i32))
    sig("pt_render_nee", C.c_int, vp, vp, i32, i32, i32)
    sig("pt_nee_rand", C.c_uint32, C.c_uint32, i32, i32)
    sig("pt_debug_light_table", C.c_int, vp, vp, vp, i64, C.POINTER(i64))
    sig("pt_set_vertex_normals", C.c_int, vp, i64, i64, vp)
    sig("pt_clear_vertex_normals", C.c_int, vp)
    sig("pt_compute_vertex_normals", C.c_int, vp, i32, f32)
    sig("pt_debug_vertex_normals", C.c_int, vp, vp, vp)
    sig("pt_debug_shading_normal", C.c_int, vp, vp, i64, vp, vp)
    sig("pt_texture_defaults", None, vp)
    sig("pt_add_texture", C.c_int, vp, vp, i32, i32, vp)
    sig("pt_clear_textures", C.c_int, vp)
    sig("pt_set_material_texture", C.c_int, vp, i32, i32)
    sig("pt_debug_texture", C.c_int, vp, i32, vp, i64, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32))
    sig("pt_set_vertex_uvs", C.c_int, vp, i64, i64, vp)
    sig("pt_clear_vertex_uvs", C.c_int, vp)
    sig("pt_debug_vertex_uvs", C.c_int, vp, vp, vp)
    sig("pt_debug_albedo", C.c_int, vp, vp, i64, vp, vp)
    sig("pt_image_read_ppm", C.c_int, C.c_char_p, vp, i64, C.POINTER(i32), C.POINTER(i32))
    sig("pt_material_roughness", f32, f32)
    sig("pt_debug_glossy", C.c_int, vp, i64, vp, vp)
    sig("pt_debug_coated", C.c_int, vp, i64, vp, vp)
    sig("pt_debug_frosted", C.c_int, vp, i64, vp, vp)
    sig("pt_lens_defaults", None, vp)
    sig("pt_set_lens", C.c_int, vp, vp)
    sig("pt_clear_lens", C.c_int, vp)
    sig("pt_focus_at", C.c_int, vp, vp, i32, i32, fp)
    sig("pt_debug_lens", C.c_int, vp, vp, vp, i64, vp, vp)
    sig("pt_environment_defaults", None, vp)
    sig("pt_set_environment", C.c_int, vp, vp, i32, i32, vp)
    sig("pt_clear_environment", C.c_int, vp)
    sig("pt_env_lookup", C.c_int, i32, i32, f32, fp, C.POINTER(i32), C.POINTER(i32))
    sig("pt_debug_environment", C.c_int, vp, C.POINTER(i32), C.POINTER(i32), vp, vp, vp, i64, fp)
    sig("pt_lights_defaults", None, vp)
    sig("pt_set_lights", C.c_int, vp, vp, i32, vp)
    sig("pt_clear_lights", C.c_int, vp)
    sig("pt_debug_lights", C.c_int, vp, vp, vp, vp, i64, C.POINTER(i64), fp)
    sig("pt_area_lights_defaults", None, vp)
    sig("pt_set_area_lights", C.c_int, vp, vp, i32, vp)
    sig("pt_clear_area_lights", C.c_int, vp)
    sig("pt_debug_area_lights", C.c_int, vp, vp, vp, vp, vp, i64, C.POINTER(i64), C.POINTER(i32), fp)
    sig("pt_debug_area_light_eval", C.c_int, vp, vp, vp, vp, i64, vp, vp, i64, vp)
    sig("pt_medium_defaults", None, vp)
    sig("pt_set_medium", C.c_int, vp, vp)
    sig("pt_clear_medium", C.c_int, vp)
    sig("pt_get_medium", C.c_int, vp, vp)
    sig("pt_debug_medium", C.c_int, vp, vp, i64, vp)
    sig("pt_set_medium_density", C.c_int, vp, vp, i32, i32, i32)
    sig("pt_clear_medium_density", C.c_int, vp)
    sig("pt_debug_medium_density", C.c_int, vp, vp, i64, vp)
    sig("pt_debug_grid", C.c_int, vp, vp, i64, vp)
    sig("pt_interior_defaults", None, vp)
    sig("pt_set_material_interior", C.c_int, vp, i32, vp)
    sig("pt_clear_material_interiors", C.c_int, vp)
    sig("pt_get_material_interior", C.c_int, vp, i32, vp)
    sig("pt_debug_interior", C.c_int, vp, vp, i64, vp)
    sig("pt_debug_light_tree", C.c_int, vp, vp, i64, C.POINTER(i64), vp, i64, C.POINTER(i64))
    sig("pt_debug_light_tree_eval", C.c_int, vp, vp, vp, vp, vp, i64, vp, i32)
    sig("pt_image_read_pfm", C.c_int, C.c_char_p, vp, i64, C.POINTER(i32), C.POINTER(i32))
    sig("pt_read_variance", C.c_int, vp, vp, i64)
    sig("pt_device_variance", vp, vp)
    sig("pt_denoise_variance_defaults", None, vp)
    sig("pt_denoise_variance", C.c_int, vp, vp)
    sig("pt_temporal_defaults", None, vp)
    sig("pt_temporal_accumulate", C.c_int, vp, vp)
    sig("pt_read_temporal", C.c_int, vp, vp, vp, i64)
    sig("pt_device_temporal", vp, vp)
    sig("pt_denoise_temporal", C.c_int, vp, vp)
    sig("pt_despeckle_defaults", None, vp)
    sig("pt_despeckle", C.c_int, vp, vp)
    sig("pt_read_despeckled", C.c_int, vp, vp, vp, i64)
    sig("pt_device_despeckled", vp, vp)
    sig("pt_denoise_despeckled", C.c_int, vp, vp)
    sig("pt_debug_despeckle", C.c_int, vp, vp, i32, i32, vp, vp, vp)
    sig("pt_display_defaults", None, vp)
    sig("pt_display", C.c_int, vp, vp)
    sig("pt_read_display", C.c_int, vp, vp, vp, i64)
    sig("pt_device_display", vp, vp)
    sig("pt_display_info", C.c_int, vp, vp)
    sig("pt_debug_display_histogram", C.c_int, vp, vp)
    sig("pt_display_reset", C.c_int, vp)
    sig("pt_write_display_ppm", C.c_int, vp, C.c_char_p)
    sig("pt_debug_display", C.c_int, vp, vp, i32, i32, vp, f32, vp, vp, vp, vp)
    sig("pt_debug_reproject", C.c_int, vp, vp, i32, i32, f32, fp)
    sig("pt_render_aovs", C.c_int, vp, vp, i32, i32)
    sig("pt_read_aovs", C.c_int, vp, vp, vp, i64)
    sig("pt_aov_defaults", None, vp)
    sig("pt_render_aovs_ex", C.c_int, vp, vp, vp)
    sig("pt_denoise_defaults", None, vp)
    sig("pt_denoise", C.c_int, vp, vp)
    sig("pt_read_denoised", C.c_int, vp, vp, i64)
    sig("pt_device_denoised", vp, vp)
    sig("pt_set_current_sample", C.c_int, vp, i32)
    sig("pt_get_current_sample", C.c_int, vp, C.POINTER(i32))
    sig("pt_sync", C.c_int, vp)
    sig("pt_local_pixel_count", C.c_int, vp, C.POINTER(i64))
    sig("pt_local_pixel_ids", C.c_int, vp, vp, i64)
    sig("pt_read_colors", C.c_int, vp, vp, i64)
    sig("pt_read_rnds", C.c_int, vp, vp, i64)
    sig("pt_read_rays", C.c_int, vp, vp, i64)
    sig("pt_resolve_ldr", C.c_int, vp, i32, vp, i64)
    sig("pt_bind_framebuffer", C.c_int, vp, vp, vp)
    sig("pt_device_colors", vp, vp)
    sig("pt_device_rnds", vp, vp)
    sig("pt_set_stream", C.c_int, vp, vp)
    sig("pt_set_option", C.c_int, vp, C.c_char_p, i64)
    sig("pt_get_stat", C.c_int, vp, C.c_char_p, C.POINTER(C.c_double))
    sig("pt_debug_bvh_sizes", C.c_int, vp, C.POINTER(i64), C.POINTER(i64))
    sig("pt_debug_bvh_copy", C.c_int, vp, vp, vp, vp, vp)
    sig("pt_debug_wide_nodes", C.c_int, vp, vp, i64, C.POINTER(i64))
    sig("pt_debug_flat_list", C.c_int, vp, vp, C.POINTER(C.c_uint32))
    sig("pt_debug_encounter_rank", C.c_int, vp, vp, i64)
    sig("pt_debug_tile_cost", C.c_int, vp, vp, i64)
    sig("pt_debug_adaptive_list", C.c_int, vp, vp, i64, C.POINTER(i64))
    sig("pt_debug_launch_plan", C.c_int, vp, i32, i32, vp)
    sig("pt_debug_scene_sizes", C.c_int, vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64))
    sig("pt_debug_scene_copy", C.c_int, vp, vp, vp, vp)
    sig("pt_debug_closest_hit", C.c_int, vp, vp, i64, vp, vp)
    sig("pt_slab_pixel_count", C.c_int, vp, C.POINTER(i64))
    sig("pt_frame_size", C.c_int, vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64))
    sig("pt_comm_available", C.c_int)
    sig("pt_comm_unique_id", C.c_int, vp)
    sig("pt_comm_init", C.c_int, vp, vp)
    sig("pt_gather_frame", C.c_int, vp)
    sig("pt_device_frame", vp, vp)
    sig("pt_read_frame", C.c_int, vp, vp, i64)
    sig("pt_write_pfm", C.c_int, vp, C.c_char_p)
    sig("pt_write_ppm", C.c_int, vp, C.c_char_p, i32)
    sig("pt_image_write_pfm", C.c_int, C.c_char_p, vp, i32, i32)
    sig("pt_image_write_ppm", C.c_int, C.c_char_p, vp, i32, i32)
    sig("pt_debug_gather_index", C.c_int, i32, i32, i32, i32, i64, vp)
    sig("pt_debug_math", C.c_int, vp, i32, i64, i64, vp, vp, i64)
    sig("pt_debug_spec", C.c_int, vp, i32, i64, vp, vp)
    sig("pt_debug_shade", C.c_int, vp, vp, i32, i32, i64, vp, vp)
    sig("pt_debug_deinterleave", C.c_int, vp, vp, i64, vp)
    return L


LIB = _load()


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def Material(kd, ks, emission, N, K, shininess, mtype):
    """Material(kd,ks,emission,N,K,shininess,type), main.cpp:101-111 -> 80-byte record."""
    m = np.zeros(1, dtype=MATERIAL)
    LIB.pt_material_init(_ptr(m), _f3(kd), _f3(ks), _f3(emission), _f3(N), _f3(K), float(shininess), int(mtype))
    return m


def Triangle(r1, r2, r3, mati):
    """Triangle(r1,r2,r3,mati), main.cpp:144-166 -> 80-byte record."""
    t = np.zeros(1, dtype=TRIANGLE)
    LIB.pt_triangle_init(_ptr(t), _f3(r1), _f3(r2), _f3(r3), int(mati))
    return t


def Camera(fov, yaw, pitch, shift, width, height):
    """Camera(), main.cpp:311-347, with the globals it reads passed in."""
    c = np.zeros(1, dtype=CAMERA)
    LIB.pt_camera_init(_ptr(c), float(fov), float(yaw), float(pitch), _f3(shift), int(width), int(height))
    return c


def camera_move(shift, yaw, pitch, forward, rightward, upward):
    """main.cpp:334-336: the movement the reference's Camera() adds into global_shift; returns the new shift (3 floats)."""
    v = (C.c_float * 3)(*[float(x) for x in shift])
    LIB.pt_camera_move(v, float(yaw), float(pitch), float(forward), float(rightward), float(upward))
    return (v[0], v[1], v[2])


def triangles_from_vertices(verts, mati):
    """(n,3,3) float32 vertices + (n,) material indices -> (n,) TRIANGLE records."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 9)
    mati = np.ascontiguousarray(mati, dtype=np.uint16)
    out = np.zeros(verts.shape[0], dtype=TRIANGLE)
    LIB.pt_triangles_init(_ptr(out), _ptr(verts), _ptr(mati), verts.shape[0])
    return out


def adaptive_rounds(min_spp, max_spp):
    """The sample-count boundaries of Scene.render_adaptive(min_spp, max_spp, ...): min_spp/2, min_spp, 2*min_spp, ..., max_spp."""
    n = C.c_int32()
    rc = LIB.pt_adaptive_rounds(int(min_spp), int(max_spp), None, 0, C.byref(n))
    if rc != PT_OK:
        raise PtError(rc, (LIB.pt_last_error(None) or b"").decode())
    out = np.zeros(n.value, dtype=np.int32)
    rc = LIB.pt_adaptive_rounds(int(min_spp), int(max_spp), _ptr(out), n.value, C.byref(n))
    if rc != PT_OK:
        raise PtError(rc, (LIB.pt_last_error(None) or b"").decode())
    return [int(v) for v in out]


PT_NEE_BSDF, PT_NEE_LIGHT, PT_NEE_MIS = 0, 1, 2
PT_GRID_MAX_DIM = 256          # pt_set_medium_density: the largest dimension of a density grid
PT_MATH_SQRT, PT_MATH_RSQRT, PT_MATH_DIV_GRID, PT_MATH_DIV_RANDOM, PT_MATH_DIV_NORMAL, PT_MATH_LCG = 0, 1, 2, 3, 4, 5   # pt_debug_math enumerations
# pt_debug_spec functions, and the 32-bit words each takes and gives per item
(PT_SPEC_SINCOS, PT_SPEC_SINCOS_SK, PT_SPEC_POW, PT_SPEC_POW_SK, PT_SPEC_POW5, PT_SPEC_LCG, PT_SPEC_DIFFUSE, PT_SPEC_DIFFUSE_SK,
 PT_SPEC_DIFFUSE_REC, PT_SPEC_DIFFUSE_REC_SK, PT_SPEC_FRESNEL) = range(11)
SPEC_WORDS = {PT_SPEC_SINCOS: (1, 2), PT_SPEC_SINCOS_SK: (1, 2), PT_SPEC_POW: (2, 1), PT_SPEC_POW_SK: (2, 1), PT_SPEC_POW5: (1, 1),
              PT_SPEC_LCG: (1, 2), PT_SPEC_DIFFUSE: (8, 8), PT_SPEC_DIFFUSE_SK: (8, 8), PT_SPEC_DIFFUSE_REC: (8, 8),
              PT_SPEC_DIFFUSE_REC_SK: (8, 8), PT_SPEC_FRESNEL: (9, 3)}
# pt_debug_shade: instance bits, and the 32-bit words per item in and out
PT_SHADE_SK, PT_SHADE_REC = 1, 2
SHADE_WORDS_IN, SHADE_WORDS_OUT = 25, 23
NEE_STRATEGIES = {"bsdf": PT_NEE_BSDF, "light": PT_NEE_LIGHT, "mis": PT_NEE_MIS}


PT_ADAPT_HALF, PT_ADAPT_VARIANCE = 0, 1
PT_ADAPT_PATH_RENDER, PT_ADAPT_PATH_NEE = 0, 1
ADAPT_METRICS = {"half": PT_ADAPT_HALF, "variance": PT_ADAPT_VARIANCE}
ADAPT_PATHS = {"render": PT_ADAPT_PATH_RENDER, "nee": PT_ADAPT_PATH_NEE}


class AdaptiveParams(C.Structure):
    """pt_adaptive_params (include/pt_api.h)."""
    _fields_ = [("min_spp", C.c_int32), ("max_spp", C.c_int32), ("threshold", C.c_float), ("metric", C.c_int32), ("path", C.c_int32),
                ("strategy", C.c_int32), ("tonemapped", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def adaptive_defaults():
    """pt_adaptive_defaults as a dict: min_spp, max_spp, threshold, metric, path, strategy, tonemapped."""
    p = AdaptiveParams()
    LIB.pt_adaptive_defaults(C.byref(p))
    return p.as_dict()


def nee_rand(state, segment, dim):
    """pt_nee_rand: the counter-based hash the light samples of Scene.render_nee draw from (include/pt_api.h pins it)."""
    return int(LIB.pt_nee_rand(int(state) & 0xffffffff, int(segment), int(dim)))


def material_roughness(shininess):
    """pt_material_roughness: the GGX alpha a type-4 material of that shininess gets under option "glossy" (include/pt_api.h)."""
    return float(LIB.pt_material_roughness(float(shininess)))


class EnvironmentParams(C.Structure):
    """pt_environment_params (include/pt_api.h)."""
    _fields_ = [("scale", C.c_float), ("yaw_degrees", C.c_float), ("select", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def environment_defaults():
    """pt_environment_defaults as a dict: scale, yaw_degrees, select."""
    p = EnvironmentParams()
    LIB.pt_environment_defaults(C.byref(p))
    return p.as_dict()


LIGHT_POINT, LIGHT_DIRECTIONAL, LIGHTS_MAX = 0, 1, 4096


class Light(C.Structure):
    """pt_light (include/pt_api.h)."""
    _fields_ = [("type", C.c_int32), ("position", C.c_float * 3), ("direction", C.c_float * 3), ("intensity", C.c_float * 3),
                ("cos_inner", C.c_float), ("cos_outer", C.c_float), ("weight", C.c_float)]


class LightsParams(C.Structure):
    """pt_lights_params (include/pt_api.h)."""
    _fields_ = [("select", C.c_float)]


def lights_defaults():
    """pt_lights_defaults as a dict: select."""
    p = LightsParams()
    LIB.pt_lights_defaults(C.byref(p))
    return {"select": p.select}


def _light(ltype, position, direction, intensity, cos_inner, cos_outer, weight):
    return Light(int(ltype), (C.c_float * 3)(*[float(v) for v in position]), (C.c_float * 3)(*[float(v) for v in direction]),
                 (C.c_float * 3)(*[float(v) for v in intensity]), float(cos_inner), float(cos_outer), float(weight))


def point_light(position, intensity, weight=0):
    """An omnidirectional point light of radiant intensity `intensity` (rgb); weight 0: selected in proportion to r + g + b."""
    return _light(LIGHT_POINT, position, (0.0, 0.0, 0.0), intensity, -1.0, -1.0, weight)


def spot_light(position, direction, intensity, inner_degrees, outer_degrees, weight=0):
    """A point light with a cone around `direction` (the way it points): full strength within inner_degrees of the axis, nothing
    beyond outer_degrees, a smoothstep between."""
    return _light(LIGHT_POINT, position, direction, intensity, np.cos(np.radians(float(inner_degrees))), np.cos(np.radians(float(outer_degrees))), weight)


def directional_light(direction, irradiance, weight=0):
    """A light from infinity travelling along `direction`; irradiance (rgb) is what a surface facing it receives."""
    return _light(LIGHT_DIRECTIONAL, (0.0, 0.0, 0.0), direction, irradiance, -1.0, -1.0, weight)


def light_from(d):
    """A Light from its description as scenes.SceneSpec.lights holds it: dict(kind="point" | "spot" | "directional", ...) with the
    arguments of point_light / spot_light / directional_light."""
    d = dict(d)
    kind = d.pop("kind")
    make = {"point": point_light, "spot": spot_light, "directional": directional_light}
    if kind not in make:
        raise KeyError("a light's kind must be one of %s, not %r" % (", ".join(sorted(make)), kind))
    return make[kind](**d)


AREA_LIGHT_SPHERE, AREA_LIGHT_SUN, AREA_LIGHTS_MAX, AREA_KEY = 0, 1, 64, 0x9e3779b9


class AreaLight(C.Structure):
    """pt_area_light (include/pt_api.h), 48 bytes."""
    _fields_ = [("type", C.c_int32), ("position", C.c_float * 3), ("direction", C.c_float * 3), ("radiance", C.c_float * 3),
                ("size", C.c_float), ("weight", C.c_float)]


class AreaLightsParams(C.Structure):
    """pt_area_lights_params (include/pt_api.h)."""
    _fields_ = [("select", C.c_float)]


# pt_area_light_sample and pt_area_light_hit (include/pt_api.h)
AREA_LIGHT_SAMPLE = np.dtype([("w", np.float32, 3), ("p_omega", np.float32), ("t_s", np.float32), ("accept", np.int32)])
AREA_LIGHT_HIT = np.dtype([("sphere", np.int32), ("t", np.float32), ("suns", np.uint32, 2)])


def area_lights_defaults():
    """pt_area_lights_defaults as a dict: select."""
    p = AreaLightsParams()
    LIB.pt_area_lights_defaults(C.byref(p))
    return {"select": p.select}


def _rgb(v):
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    return np.repeat(v, 3) if v.size == 1 else v.reshape(3)


def _area_light(ltype, position, direction, radiance, size, weight):
    return AreaLight(int(ltype), (C.c_float * 3)(*[float(v) for v in position]), (C.c_float * 3)(*[float(v) for v in direction]),
                     (C.c_float * 3)(*[float(v) for v in radiance]), float(size), float(weight))


def sphere_light(center, radius, radiance=None, power=None, weight=0):
    """A sphere light of uniform radiance (rgb): give `radiance`, or the `power` it emits in all (a sphere of radius R and radiance L emits
    4 pi^2 R^2 L).  It casts soft shadows and is seen by the camera, in mirrors and through glass."""
    if (radiance is None) == (power is None):
        raise ValueError("sphere_light takes exactly one of radiance and power")
    if radiance is None:
        radiance = _rgb(power) / (4.0 * np.pi * np.pi * float(radius) * float(radius))
    return _area_light(AREA_LIGHT_SPHERE, center, (0.0, 0.0, 0.0), _rgb(radiance), radius, weight)


def sun_light(direction, angular_diameter_degrees, irradiance=None, radiance=None, weight=0):
    """A sun: a disc at infinity of the given angular diameter whose light travels along `direction`.  Give its `radiance`, or the
    `irradiance` E_perp a surface facing it receives: L = E_perp / (2 pi (1 - cos a)), a the angular radius."""
    if (radiance is None) == (irradiance is None):
        raise ValueError("sun_light takes exactly one of irradiance and radiance")
    a = np.radians(0.5 * float(angular_diameter_degrees))
    if radiance is None:
        radiance = _rgb(irradiance) / (2.0 * np.pi * (2.0 * np.sin(0.5 * a) ** 2))
    return _area_light(AREA_LIGHT_SUN, (0.0, 0.0, 0.0), direction, _rgb(radiance), a, weight)


def area_light_from(d):
    """An AreaLight from its description as scenes.SceneSpec.area_lights holds it: dict(kind="sphere" | "sun", ...) with the arguments of
    sphere_light / sun_light."""
    d = dict(d)
    kind = d.pop("kind")
    make = {"sphere": sphere_light, "sun": sun_light}
    if kind not in make:
        raise KeyError("an area light's kind must be one of %s, not %r" % (", ".join(sorted(make)), kind))
    return make[kind](**d)


class Medium(C.Structure):
    """pt_medium (include/pt_api.h): a homogeneous participating medium, 44 bytes."""
    _fields_ = [("sigma_t", C.c_float), ("albedo", C.c_float * 3), ("g", C.c_float), ("lo", C.c_float * 3), ("hi", C.c_float * 3)]

    def as_dict(self):
        return {"sigma_t": float(self.sigma_t), "albedo": tuple(self.albedo), "g": float(self.g), "lo": tuple(self.lo), "hi": tuple(self.hi)}


class Interior(C.Structure):
    """pt_interior (include/pt_api.h): the medium inside a type-2 or type-6 material, 20 bytes."""
    _fields_ = [("sigma_a", C.c_float * 3), ("sigma_s", C.c_float), ("g", C.c_float)]

    def as_dict(self):
        return dict(sigma_a=tuple(self.sigma_a), sigma_s=self.sigma_s, g=self.g)


def interior_defaults():
    """pt_interior_defaults as a dict: sigma_a (0, 0, 0), sigma_s 0, g 0."""
    p = Interior()
    LIB.pt_interior_defaults(C.byref(p))
    return p.as_dict()


def interior_from_tint(color, distance):
    """The sigma_a (rgb, float64) that tints white light to `color` over `distance` of travel inside: -ln(color) / distance per channel
    (Beer-Lambert).  color in (0, 1] per channel (1: no absorption), distance > 0."""
    c = np.asarray(color, dtype=np.float64).reshape(3)
    if not (np.all(c > 0.0) and np.all(c <= 1.0)) or not float(distance) > 0.0:
        raise ValueError("interior_from_tint: color must lie in (0, 1] per channel and distance must be > 0")
    return tuple(float(v) for v in (-np.log(c) / float(distance) + 0.0))


# a node of pt_debug_light_tree (8 words) and pt_light_tree_eval (include/pt_api.h)
LIGHT_TREE_NODE = np.dtype([("c", np.float32, 3), ("r", np.float32), ("phi", np.float32), ("first", np.int32), ("count", np.int32), ("right", np.int32)])
LIGHT_TREE_EVAL = np.dtype([("tri", np.int32), ("p", np.float32), ("p_weight", np.float32), ("slot", np.int32)])


def medium_defaults():
    """pt_medium_defaults as a dict: sigma_t 0, albedo (1, 1, 1), g 0, lo (-inf, -inf, -inf), hi (+inf, +inf, +inf)."""
    m = Medium()
    LIB.pt_medium_defaults(C.byref(m))
    return m.as_dict()


class LensParams(C.Structure):
    """pt_lens_params (include/pt_api.h): aperture = the lens radius (0: the pinhole), focus_distance along the optical axis."""
    _fields_ = [("aperture", C.c_float), ("focus_distance", C.c_float), ("_pad", C.c_float * 2)]

    def as_dict(self):
        return {"aperture": self.aperture, "focus_distance": self.focus_distance}


def lens_defaults():
    """pt_lens_defaults as a dict: aperture, focus_distance."""
    p = LensParams()
    LIB.pt_lens_defaults(C.byref(p))
    return p.as_dict()


class TextureParams(C.Structure):
    """pt_texture_params (include/pt_api.h): filter 0 nearest / 1 bilinear, srgb 1 = the texels are sRGB-encoded."""
    _fields_ = [("filter", C.c_int32), ("srgb", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def texture_defaults():
    """pt_texture_defaults as a dict: filter, srgb."""
    p = TextureParams()
    LIB.pt_texture_defaults(C.byref(p))
    return p.as_dict()


def env_lookup(w, h, yaw_degrees, direction):
    """pt_env_lookup: (row, col) of the texel a unit direction reads in a w x h lat-long map (include/pt_api.h pins the mapping)."""
    row, col = C.c_int32(), C.c_int32()
    rc = LIB.pt_env_lookup(int(w), int(h), float(yaw_degrees), _f3(direction), C.byref(row), C.byref(col))
    if rc != PT_OK:
        raise PtError(rc, (LIB.pt_last_error(None) or b"").decode())
    return row.value, col.value


class DenoiseParams(C.Structure):
    """pt_denoise_params (include/pt_api.h)."""
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("demodulate", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DenoiseVarianceParams(C.Structure):
    """pt_denoise_variance_params (include/pt_api.h)."""
    _fields_ = [("iterations", C.c_int32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_depth", C.c_float),
                ("demodulate", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


PT_AOV_GEOMETRIC, PT_AOV_SHADED = 0, 1
AOV_SHADING = {"geometric": PT_AOV_GEOMETRIC, "shaded": PT_AOV_SHADED}


class AovParams(C.Structure):
    """pt_aov_params (include/pt_api.h)."""
    _fields_ = [("subpixels", C.c_int32), ("specular_depth", C.c_int32), ("shading", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def aov_defaults():
    """pt_aov_defaults as a dict: subpixels, specular_depth, shading."""
    p = AovParams()
    LIB.pt_aov_defaults(C.byref(p))
    return p.as_dict()


def denoise_variance_defaults():
    """pt_denoise_variance_defaults as a dict: iterations, sigma_luminance, sigma_normal, sigma_depth, demodulate."""
    p = DenoiseVarianceParams()
    LIB.pt_denoise_variance_defaults(C.byref(p))
    return p.as_dict()


def denoise_defaults():
    """pt_denoise_defaults as a dict: iterations, sigma_color, sigma_normal, sigma_depth, demodulate."""
    p = DenoiseParams()
    LIB.pt_denoise_defaults(C.byref(p))
    return p.as_dict()


class TemporalParams(C.Structure):
    """pt_temporal_params (include/pt_api.h)."""
    _fields_ = [("max_history", C.c_int32), ("normal_cos", C.c_float), ("depth_tolerance", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def temporal_defaults():
    """pt_temporal_defaults as a dict: max_history, normal_cos, depth_tolerance."""
    p = TemporalParams()
    LIB.pt_temporal_defaults(C.byref(p))
    return p.as_dict()


PT_DESPECKLE_FRAME, PT_DESPECKLE_TEMPORAL = 0, 1
DESPECKLE_SOURCE = {"frame": PT_DESPECKLE_FRAME, "temporal": PT_DESPECKLE_TEMPORAL}


class DespeckleParams(C.Structure):
    """pt_despeckle_params (include/pt_api.h)."""
    _fields_ = [("source", C.c_int32), ("radius", C.c_int32), ("rank", C.c_int32), ("threshold", C.c_float), ("floor", C.c_float),
                ("min_rel_sigma", C.c_float), ("spread", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def despeckle_defaults():
    """pt_despeckle_defaults as a dict: source, radius, rank, threshold, floor, min_rel_sigma, spread."""
    p = DespeckleParams()
    LIB.pt_despeckle_defaults(C.byref(p))
    return p.as_dict()


def _despeckle_params(who, params):
    p = DespeckleParams(**despeckle_defaults())
    for k, v in params.items():
        if k not in p.as_dict():
            raise TypeError("unknown %s parameter %r" % (who, k))
        setattr(p, k, DESPECKLE_SOURCE.get(v, v) if k == "source" and isinstance(v, str) else v)
    return p


PT_DISPLAY_FRAME, PT_DISPLAY_DENOISED, PT_DISPLAY_TEMPORAL, PT_DISPLAY_DESPECKLED = range(4)
PT_METER_MANUAL, PT_METER_AUTO = 0, 1
PT_CURVE_LINEAR, PT_CURVE_REINHARD, PT_CURVE_ACES = range(3)
PT_ENCODE_SRGB, PT_ENCODE_LINEAR = 0, 1
DISPLAY_NAMES = {
    "source": {"frame": PT_DISPLAY_FRAME, "denoised": PT_DISPLAY_DENOISED, "temporal": PT_DISPLAY_TEMPORAL, "despeckled": PT_DISPLAY_DESPECKLED},
    "metering": {"manual": PT_METER_MANUAL, "auto": PT_METER_AUTO},
    "curve": {"linear": PT_CURVE_LINEAR, "reinhard": PT_CURVE_REINHARD, "aces": PT_CURVE_ACES},
    "encoding": {"srgb": PT_ENCODE_SRGB, "linear": PT_ENCODE_LINEAR},
}


class DisplayParams(C.Structure):
    """pt_display_params (include/pt_api.h)."""
    _fields_ = [("source", C.c_int32), ("metering", C.c_int32), ("ev", C.c_float), ("key", C.c_float), ("low_permille", C.c_int32),
                ("high_permille", C.c_int32), ("min_ev", C.c_float), ("max_ev", C.c_float), ("adapt", C.c_float), ("bloom_levels", C.c_int32),
                ("bloom_threshold", C.c_float), ("bloom_intensity", C.c_float), ("curve", C.c_int32), ("white", C.c_float),
                ("encoding", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DisplayInfo(C.Structure):
    """struct pt_display_info (include/pt_api.h)."""
    _fields_ = [("exposure", C.c_float), ("mean_log2", C.c_float), ("n_metered", C.c_uint32), ("n_dark", C.c_uint32),
                ("n_nonfinite", C.c_uint32), ("levels", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def display_defaults():
    """pt_display_defaults as a dict (the fields of pt_display_params)."""
    p = DisplayParams()
    LIB.pt_display_defaults(C.byref(p))
    return p.as_dict()


def _display_params(who, params):
    p = DisplayParams(**display_defaults())
    for k, v in params.items():
        if k not in p.as_dict():
            raise TypeError("unknown %s parameter %r" % (who, k))
        setattr(p, k, DISPLAY_NAMES[k][v] if isinstance(v, str) else v)
    return p


def debug_reproject(cur, prev, x, y, depth):
    """pt_debug_reproject: pixel (x, y) of CAMERA record cur at `depth`, in CAMERA record prev's view -> (x', y', distance to prev's
    eye); raises PtError(PT_EINVAL) when the point is not in front of prev."""
    out = (C.c_float * 3)()
    rc = LIB.pt_debug_reproject(_ptr(cur), _ptr(prev), int(x), int(y), float(depth), out)
    if rc != PT_OK:
        raise PtError(rc, (LIB.pt_last_error(None) or b"").decode())
    return (out[0], out[1], out[2])


def comm_available():
    """(True, "") if librccl is bound in this process, else (False, why).  No collective is touched."""
    rc = LIB.pt_comm_available()
    return (True, "") if rc == PT_OK else (False, (LIB.pt_last_error(None) or b"").decode())


def comm_unique_id():
    """ncclGetUniqueId through the C ABI: 128 bytes for rank 0 to hand to every rank."""
    buf = (C.c_ubyte * PT_COMM_ID_BYTES)()
    rc = LIB.pt_comm_unique_id(C.cast(buf, C.c_void_p))
    if rc != PT_OK:
        raise PtError(rc, (LIB.pt_last_error(None) or b"").decode())
    return bytes(buf)


def gather_index(width, height, world, rows_per_block, slab_stride):
    out = np.empty(width * height, dtype=np.int64)
    rc = LIB.pt_debug_gather_index(width, height, world, rows_per_block, slab_stride, _ptr(out))
    if rc != PT_OK:
        raise PtError(rc, "pt_debug_gather_index")
    return out


def write_pfm(path, rgba, width, height):
    rgba = np.ascontiguousarray(rgba, dtype=np.float32).reshape(width * height, 4)
    rc = LIB.pt_image_write_pfm(os.fsencode(path), _ptr(rgba), width, height)
    if rc != PT_OK:
        raise PtError(rc, "cannot write %s" % path)


def read_pfm(path):
    """pt_image_read_pfm: (height, width, 4) float32 in the file's row order -- row 0 is the bottom of an image write_pfm wrote; a
    lat-long map for Scene.set_environment wants its top row first: read_pfm(path)[::-1, :, :3]."""
    w, h = C.c_int32(), C.c_int32()
    rc = LIB.pt_image_read_pfm(os.fsencode(path), None, 0, C.byref(w), C.byref(h))
    if rc != PT_OK:
        raise PtError(rc, "cannot read %s" % path)
    out = np.empty((h.value, w.value, 4), dtype=np.float32)
    rc = LIB.pt_image_read_pfm(os.fsencode(path), _ptr(out), w.value * h.value, C.byref(w), C.byref(h))
    if rc != PT_OK:
        raise PtError(rc, "cannot read %s" % path)
    return out


def read_ppm(path):
    """pt_image_read_ppm: (height, width, 3) float32, sample / maxval, top row first (what Scene.add_texture takes; srgb=1 for an
    8-bit picture)."""
    w, h = C.c_int32(), C.c_int32()
    rc = LIB.pt_image_read_ppm(os.fsencode(path), None, 0, C.byref(w), C.byref(h))
    if rc != PT_OK:
        raise PtError(rc, "cannot read %s" % path)
    out = np.empty((h.value, w.value, 3), dtype=np.float32)
    rc = LIB.pt_image_read_ppm(os.fsencode(path), _ptr(out), w.value * h.value, C.byref(w), C.byref(h))
    if rc != PT_OK:
        raise PtError(rc, "cannot read %s" % path)
    return out


def write_ppm(path, rgba, width, height):
    rgba = np.ascontiguousarray(rgba, dtype=np.float32).reshape(width * height, 4)
    rc = LIB.pt_image_write_ppm(os.fsencode(path), _ptr(rgba), width, height)
    if rc != PT_OK:
        raise PtError(rc, "cannot write %s" % path)


class Scene:
    """The reference's Scene (main.cpp:363-742) on one MI355X.

    device=None -> host-only context (authoring + BVH build only).  rank/world/rows_per_block
    select this context's interleaved row blocks of the global frame (multi-GPU tiling)."""

    def __init__(self, width, height, device=0, rank=0, world=1, rows_per_block=8):
        self.width, self.height = int(width), int(height)
        self.rank, self.world, self.rows_per_block = rank, world, rows_per_block
        # the reference's mutable globals (main.cpp:27-39), shipped defaults replaced by the
        # "canonical" view it keeps in comments (main.cpp:33-35, 40)
        self.iterations = 1
        self.fov, self.yaw, self.pitch, self.shift = 60.0, 0.0, 0.0, (0.0, 0.0, 0.0)
        self._h = C.c_void_p()
        dev = -1 if device is None else int(device)
        self._host_only = device is None
        rc = LIB.pt_create_tiled(dev, self.width, self.height, rank, world, rows_per_block, C.byref(self._h))
        if rc != PT_OK:
            raise PtError(rc, (LIB.pt_last_error(None) or b"").decode())
        self.camera = Camera(self.fov, self.yaw, self.pitch, self.shift, self.width, self.height)

    # -- plumbing
    def _ck(self, rc):
        if rc < 0:
            raise PtError(rc, (LIB.pt_last_error(self._h) or b"").decode())
        return rc

    def close(self):
        if getattr(self, "_h", None):
            LIB.pt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def list_info(self):                                   # Scene::list_info, main.cpp:389-455
        buf = C.create_string_buffer(256)
        self._ck(LIB.pt_device_info(self._h, buf, 256))
        return buf.value.decode()

    # -- authoring (main.cpp:529-617)
    def add_Material(self, *args):
        m = args[0] if len(args) == 1 else Material(*args)
        return self._ck(LIB.pt_add_material(self._h, _ptr(m)))

    def add_Triangle(self, *args):
        t = args[0] if len(args) == 1 else Triangle(*args)
        self._ck(LIB.pt_add_triangle(self._h, _ptr(t)))

    def add_Triangles(self, tris):
        tris = np.ascontiguousarray(tris, dtype=TRIANGLE)
        self._ck(LIB.pt_add_triangles(self._h, _ptr(tris), tris.shape[0]))

    def end_Obj(self):
        self._ck(LIB.pt_end_obj(self._h))

    def add_Obj(self, file, pos, scale, pitch, yaw):
        self._ck(LIB.pt_add_obj(self._h, os.fsencode(file), _f3(pos), _f3(scale), float(pitch), float(yaw)))

    # -- vertex normals (option "smooth_normals"; authoring calls: host data, no BVH rebuild, packed for the device at the next
    #    render_nee / render_adaptive(path="nee") / debug_shading_normals)
    def set_vertex_normals(self, normals, first=0):
        """normals (n, 3, 3): n1 n2 n3 of triangles [first, first + n) in add order; a triangle with a zero or non-finite normal has none."""
        nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 9)
        self._ck(LIB.pt_set_vertex_normals(self._h, int(first), nrm.shape[0], _ptr(nrm)))

    def clear_vertex_normals(self):
        self._ck(LIB.pt_clear_vertex_normals(self._h))

    def compute_vertex_normals(self, crease_degrees, obj=-1):
        """Angle-weighted normals per corner over the triangles of the same object that share the position and lie within crease_degrees."""
        self._ck(LIB.pt_compute_vertex_normals(self._h, int(obj), float(crease_degrees)))

    def debug_vertex_normals(self):
        """(normals (n, 3, 3) as recorded, has (n,) bool) per added triangle."""
        nt = C.c_int64()
        self._ck(LIB.pt_debug_scene_sizes(self._h, C.byref(nt), None, None))
        nrm = np.zeros((nt.value, 3, 3), dtype=np.float32)
        has = np.zeros(nt.value, dtype=np.int32)
        self._ck(LIB.pt_debug_vertex_normals(self._h, _ptr(nrm), _ptr(has)))
        return nrm, has.astype(bool)

    def debug_shading_normals(self, rays):
        """pt_debug_shading_normal: (add-order triangle or -1, (n, 4) float32 {Ns.xyz, t}) of each ray's closest hit."""
        rays = np.ascontiguousarray(rays, dtype=RAY)
        tri = np.empty(rays.shape[0], dtype=np.int32)
        ns = np.empty((rays.shape[0], 4), dtype=np.float32)
        self._ck(LIB.pt_debug_shading_normal(self._h, _ptr(rays), rays.shape[0], _ptr(tri), _ptr(ns)))
        return tri, ns

    # -- albedo textures and uvs (option "textures"; authoring calls: host data, no BVH rebuild, copied to the device at the next
    #    render_nee / render_adaptive(path="nee") / debug_albedo)
    def add_texture(self, rgb, **params):
        """pt_add_texture: rgb (h, w, 3) float, row 0 at the top; params override pt_texture_defaults (filter, srgb).  Returns the index."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError("rgb must have shape (h, w, 3)")
        p = TextureParams(**texture_defaults())
        for k, v in params.items():
            if k not in ("filter", "srgb"):
                raise TypeError("unknown texture parameter %r" % k)
            setattr(p, k, int(v))
        return self._ck(LIB.pt_add_texture(self._h, _ptr(rgb), rgb.shape[1], rgb.shape[0], C.byref(p)))

    def clear_textures(self):
        self._ck(LIB.pt_clear_textures(self._h))

    def set_material_texture(self, material, texture):
        """Bind texture (an index of add_texture, or -1 / None: none) to a material; only a type-0 material reads it."""
        self._ck(LIB.pt_set_material_texture(self._h, int(material), -1 if texture is None else int(texture)))

    def debug_texture(self, texture):
        """pt_debug_texture: ((h, w, 3) float32 of the stored halves, filter)."""
        w, h, f = C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(LIB.pt_debug_texture(self._h, int(texture), None, 0, C.byref(w), C.byref(h), C.byref(f)))
        out = np.empty((h.value, w.value, 3), dtype=np.float32)
        self._ck(LIB.pt_debug_texture(self._h, int(texture), _ptr(out), w.value * h.value, None, None, None))
        return out, f.value

    def set_vertex_uvs(self, uvs, first=0):
        """uvs (n, 3, 2): (u, v) of the corners of triangles [first, first + n) in add order; a triangle with a non-finite value or one
        above 65536 in magnitude has none."""
        uv = np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1, 6)
        self._ck(LIB.pt_set_vertex_uvs(self._h, int(first), uv.shape[0], _ptr(uv)))

    def clear_vertex_uvs(self):
        self._ck(LIB.pt_clear_vertex_uvs(self._h))

    def debug_vertex_uvs(self):
        """(uvs (n, 3, 2) as recorded, 0 where a triangle has none, has (n,) bool) per added triangle."""
        nt = C.c_int64()
        self._ck(LIB.pt_debug_scene_sizes(self._h, C.byref(nt), None, None))
        uv = np.zeros((nt.value, 3, 2), dtype=np.float32)
        has = np.zeros(nt.value, dtype=np.int32)
        self._ck(LIB.pt_debug_vertex_uvs(self._h, _ptr(uv), _ptr(has)))
        return uv, has.astype(bool)

    def debug_albedo(self, rays):
        """pt_debug_albedo: (add-order triangle or -1, (n, 4) float32 {kd'.rgb, t}) of each ray's closest hit."""
        rays = np.ascontiguousarray(rays, dtype=RAY)
        tri = np.empty(rays.shape[0], dtype=np.int32)
        out = np.empty((rays.shape[0], 4), dtype=np.float32)
        self._ck(LIB.pt_debug_albedo(self._h, _ptr(rays), rays.shape[0], _ptr(tri), _ptr(out)))
        return tri, out

    # -- the rough metal of material type 4 (option "glossy")
    def debug_glossy(self, items):
        """pt_debug_glossy: items (n, 9) float32 {N, D, alpha, rnd1, rnd2} -> (n, 8) float32 {w before normalisation (world), p_b as
        sampled, G1(w), F.x with F0 = 0.04, p_b evaluated again from w, o.z}, by the device functions the glossy k_nee instances call."""
        items = np.ascontiguousarray(items, dtype=np.float32).reshape(-1, 9)
        out = np.empty((items.shape[0], 8), dtype=np.float32)
        self._ck(LIB.pt_debug_glossy(self._h, items.shape[0], _ptr(items), _ptr(out)))
        return out

    # -- the coated diffuse of material type 5 (option "coated")
    def debug_coated(self, items):
        """pt_debug_coated: items (n, 12) float32 {N, D, alpha, F0, kd, rnd1, rnd2, u_sel} -> (n, 10) float32 {w before normalisation
        (world), ps, 1 if the coat lobe drew w else 0, p_b as sampled, g.x as sampled, p_b and g.x evaluated again from w, o.z}, by the
        device functions the coated k_nee instances call."""
        items = np.ascontiguousarray(items, dtype=np.float32).reshape(-1, 12)
        out = np.empty((items.shape[0], 10), dtype=np.float32)
        self._ck(LIB.pt_debug_coated(self._h, items.shape[0], _ptr(items), _ptr(out)))
        return out

    # -- the thin lens of render_nee and render_adaptive(path="nee") (include/pt_api.h pins the lens ray)
    def set_lens(self, aperture, focus_distance):
        """pt_set_lens: aperture = the lens radius in scene units (0: the pinhole, today's kernels and bits), focus_distance = the distance
        of the plane in focus from the eye along the optical axis.  While aperture > 0 only render_nee and render_adaptive(path="nee")
        render; the guide buffers keep the pinhole view."""
        p = LensParams(float(aperture), float(focus_distance))
        self._ck(LIB.pt_set_lens(self._h, C.byref(p)))

    def clear_lens(self):
        self._ck(LIB.pt_clear_lens(self._h))

    def focus_at(self, x, y):
        """pt_focus_at: the axial distance of the first hit of pixel (x, y)'s centre ray under the current camera, +inf on a miss."""
        d = C.c_float()
        self._ck(LIB.pt_focus_at(self._h, _ptr(self.camera), int(x), int(y), C.byref(d)))
        return float(d.value)

    def debug_lens(self, aperture, focus_distance, items, camera=None):
        """pt_debug_lens: items (n, 2) int32 {gid, S} -> (n, 6) float32 {P, D}, the lens ray of the sample of pixel gid that starts at LCG
        state S, by the device function the lens instances of k_nee call (camera: a CAMERA record, default the scene's)."""
        items = np.ascontiguousarray(items, dtype=np.int32).reshape(-1, 2)
        out = np.empty((items.shape[0], 6), dtype=np.float32)
        p = LensParams(float(aperture), float(focus_distance))
        cam = self.camera if camera is None else np.ascontiguousarray(camera, dtype=CAMERA)
        self._ck(LIB.pt_debug_lens(self._h, _ptr(cam), C.byref(p), items.shape[0], _ptr(items), _ptr(out)))
        return out

    # -- the homogeneous medium of render_nee and render_adaptive(path="nee") (include/pt_api.h pins the free flight and the scatter vertex)
    def set_medium(self, sigma_t, albedo=(1, 1, 1), g=0.0, bounds=None):
        """pt_set_medium: fog of extinction sigma_t per unit length (0: none, today's kernels and bits), single-scattering albedo (rgb or a
        number) and Henyey-Greenstein asymmetry g, inside bounds = (lo, hi), two corners of an axis-aligned box (None: everywhere; -inf /
        +inf leave a side open).  While sigma_t > 0 only render_nee and render_adaptive(path="nee") render; the guide buffers keep the
        fog-free view.  An unbounded medium hides the sky and directional lights from the light samples: give it a box to let a sun in."""
        m = Medium()
        LIB.pt_medium_defaults(C.byref(m))
        m.sigma_t, m.g = float(sigma_t), float(g)
        m.albedo = (C.c_float * 3)(*[float(v) for v in (albedo if np.ndim(albedo) else (albedo,) * 3)])
        if bounds is not None:
            lo, hi = bounds
            m.lo = (C.c_float * 3)(*[float(v) for v in lo])
            m.hi = (C.c_float * 3)(*[float(v) for v in hi])
        self._ck(LIB.pt_set_medium(self._h, C.byref(m)))

    def clear_medium(self):
        self._ck(LIB.pt_clear_medium(self._h))

    def medium(self):
        """pt_get_medium: the held medium as a dict (medium_defaults()'s keys), or None when none is held."""
        m = Medium()
        rc = LIB.pt_get_medium(self._h, C.byref(m))
        if rc < 0:
            self._ck(rc)
        return m.as_dict() if rc == 1 else None

    def debug_medium(self, items):
        """pt_debug_medium: items (n, 12) float32 {P, D (unit), t, u, u1, u2, limit, spare} -> (n, 10) float32 {a, b of the clip of [0, t]
        to the box, 1 if the segment scatters else 0, the free-flight distance d, the new direction from (u1, u2) around D (unit), its
        p_b, T over [0, limit], 0}, by the device functions the medium k_nee instances call on the held medium."""
        items = np.ascontiguousarray(items, dtype=np.float32).reshape(-1, 12)
        out = np.empty((items.shape[0], 10), dtype=np.float32)
        self._ck(LIB.pt_debug_medium(self._h, _ptr(items), items.shape[0], _ptr(out)))
        return out

    # -- the medium's voxel density (include/pt_api.h pins the walk)
    def set_medium_density(self, density):
        """pt_set_medium_density: density (nz, ny, nx), finite and >= 0, each dimension in [1, PT_GRID_MAX_DIM]: the extinction in voxel
        (i, j, k) of nx x ny x nz equal cells of the medium's box is sigma_t x density[k, j, i].  Kept as float32; live while a medium
        with sigma_t > 0 is held, whose box must then be finite to render."""
        d = np.asarray(density)
        if d.ndim != 3:
            raise ValueError("set_medium_density: density must have shape (nz, ny, nx)")
        d = np.ascontiguousarray(d, dtype=np.float32)
        self._ck(LIB.pt_set_medium_density(self._h, _ptr(d), d.shape[2], d.shape[1], d.shape[0]))

    def clear_medium_density(self):
        self._ck(LIB.pt_clear_medium_density(self._h))

    def medium_density(self):
        """pt_debug_medium_density: the held grid as (nz, ny, nx) float32, or None when none is held."""
        dims = (C.c_int32 * 3)()
        rc = LIB.pt_debug_medium_density(self._h, None, 0, dims)
        if rc < 0:
            self._ck(rc)
        if rc != 1:
            return None
        out = np.empty((dims[2], dims[1], dims[0]), dtype=np.float32)
        self._ck(LIB.pt_debug_medium_density(self._h, _ptr(out), out.size, dims))
        return out

    def debug_grid(self, items):
        """pt_debug_grid: items (n, 12) float32 {P, D (unit), t, u, limit, 3 spare} -> (n, 8) float32 {a, b of the clip of [0, t] to the
        box, 1 if the free flight of u scatters else 0, its distance s (-1 without), the optical depth over [0, t], T over [0, limit],
        the voxels visited, the linear voxel index of the scatter (-1 without)}, by the walk the grid k_nee instances call."""
        items = np.ascontiguousarray(items, dtype=np.float32).reshape(-1, 12)
        out = np.empty((items.shape[0], 8), dtype=np.float32)
        self._ck(LIB.pt_debug_grid(self._h, _ptr(items), items.shape[0], _ptr(out)))
        return out

    # -- interiors of dielectrics (include/pt_api.h pins the free flight, the absorption factor and the scatter vertex)
    def set_material_interior(self, material, sigma_a=(0, 0, 0), sigma_s=0.0, g=0.0):
        """pt_set_material_interior: the medium inside `material` (type 2, or 6 under option frosted): absorption sigma_a per unit length (rgb
        or a number; interior_from_tint gives it from a colour), grey scattering sigma_s and Henyey-Greenstein g.  Live as soon as it is
        bound, an all-zero one too: only render_nee and render_adaptive(path="nee") render then; the guide buffers keep the interior-free
        view.  Kept across uploads, like a texture binding."""
        p = Interior()
        p.sigma_a = (C.c_float * 3)(*[float(v) for v in (sigma_a if np.ndim(sigma_a) else (sigma_a,) * 3)])
        p.sigma_s, p.g = float(sigma_s), float(g)
        self._ck(LIB.pt_set_material_interior(self._h, int(material), C.byref(p)))

    def clear_material_interiors(self):
        self._ck(LIB.pt_clear_material_interiors(self._h))

    def material_interior(self, material):
        """pt_get_material_interior: the binding of `material` as a dict (interior_defaults()'s keys), or None when it holds none."""
        p = Interior()
        rc = LIB.pt_get_material_interior(self._h, int(material), C.byref(p))
        if rc < 0:
            raise PtError(rc, "pt_get_material_interior: material must be the index of a material added so far")
        return p.as_dict() if rc == 1 else None

    def debug_interior(self, items):
        """pt_debug_interior: items (n, 12) float32 {sigma_a.rgb, sigma_s, g, t, u, u1, u2, D (unit)} -> (n, 10) float32 {the free-flight
        distance d (-1 when sigma_s is 0), 1 if the segment scatters (d < t) else 0, the length l absorbed over, the absorption factor
        rgb, the new direction from (u1, u2) around D (unit), 0}, by the device functions the interior k_nee instances call."""
        items = np.ascontiguousarray(items, dtype=np.float32).reshape(-1, 12)
        out = np.empty((items.shape[0], 10), dtype=np.float32)
        self._ck(LIB.pt_debug_interior(self._h, _ptr(items), items.shape[0], _ptr(out)))
        return out

    # -- the rough dielectric of material type 6 (option "frosted")
    def debug_frosted(self, items):
        """pt_debug_frosted: items (n, 12) float32 {N, D, alpha, F0, eta, rnd1, rnd2, u_sel} -> (n, 10) float32 {w before normalisation
        (world), Fm, 1 if the vertex reflects else 0, p_b as sampled (0 for a refraction), g.x as sampled, p_b and g.x evaluated again from
        w the way a light sample does (0, 0 for a refraction), o.z}, by the device functions the frosted k_nee instances call."""
        items = np.ascontiguousarray(items, dtype=np.float32).reshape(-1, 12)
        out = np.empty((items.shape[0], 10), dtype=np.float32)
        self._ck(LIB.pt_debug_frosted(self._h, items.shape[0], _ptr(items), _ptr(out)))
        return out

    def upload_Triangles(self):
        self._ck(LIB.pt_upload_triangles(self._h))

    def upload_Materials(self):
        self._ck(LIB.pt_upload_materials(self._h))

    def load(self, spec):
        """Author a scenes.SceneSpec: materials, then one object per entry, then upload."""
        nm = C.c_int64()
        self._ck(LIB.pt_debug_scene_sizes(self._h, None, C.byref(nm), None))
        for m in spec.materials:
            self.add_Material(*m)
        # optional: textures (rgb, or (rgb, dict(filter=, srgb=))), material_textures {index into spec.materials: index into
        # spec.textures}, uvs per object ((n, 3, 2) or None)
        tex = []
        for t in getattr(spec, "textures", None) or []:
            rgb, params = t if isinstance(t, tuple) else (t, {})
            tex.append(self.add_texture(rgb, **params))
        for mi, ti in (getattr(spec, "material_textures", None) or {}).items():
            self.set_material_texture(nm.value + int(mi), tex[int(ti)])
        first = 0
        normals = getattr(spec, "normals", None) or []
        uvs = getattr(spec, "uvs", None) or []
        for k, (verts, mati) in enumerate(spec.objects):
            self.add_Triangles(triangles_from_vertices(verts, mati))
            self.end_Obj()
            if k < len(normals) and normals[k] is not None:      # the object's vertex normals (n, 3, 3)
                self.set_vertex_normals(normals[k], first=first)
            if k < len(uvs) and uvs[k] is not None:              # the object's uvs (n, 3, 2)
                self.set_vertex_uvs(uvs[k], first=first)
            first += int(np.asarray(verts).shape[0])
        self.upload_Triangles()
        self.upload_Materials()
        if getattr(spec, "lights", None):                       # optional: what set_lights takes, with spec.lights_select
            self.set_lights(spec.lights, select=getattr(spec, "lights_select", 0.5))
        if getattr(spec, "area_lights", None):                  # optional: what set_area_lights takes, with spec.area_lights_select
            self.set_area_lights(spec.area_lights, select=getattr(spec, "area_lights_select", 0.5))
        if getattr(spec, "medium", None):                       # optional: set_medium's arguments as a dict
            self.set_medium(**spec.medium)
        if getattr(spec, "medium_density", None) is not None:   # optional: set_medium_density's array
            self.set_medium_density(spec.medium_density)
        for mi, kw in (getattr(spec, "interiors", None) or {}).items():      # optional: {index into spec.materials: set_material_interior's arguments}
            self.set_material_interior(nm.value + int(mi), **kw)
        self.set_view(spec.fov, spec.yaw, spec.pitch, spec.shift)
        return self

    # -- camera / globals
    def set_view(self, fov, yaw, pitch, shift):
        self.fov, self.yaw, self.pitch, self.shift = fov, yaw, pitch, tuple(shift)
        self.camera = Camera(fov, yaw, pitch, shift, self.width, self.height)

    @property
    def current_sample(self):
        v = C.c_int32()
        self._ck(LIB.pt_get_current_sample(self._h, C.byref(v)))
        return v.value

    @current_sample.setter
    def current_sample(self, v):
        self._ck(LIB.pt_set_current_sample(self._h, int(v)))

    # -- the hot path (main.cpp:635-687)
    def generate_rays(self):
        self.camera = Camera(self.fov, self.yaw, self.pitch, self.shift, self.width, self.height)   # main.cpp:636
        self._ck(LIB.pt_generate_rays(self._h, _ptr(self.camera)))

    def trace_rays(self):
        self._ck(LIB.pt_trace_rays(self._h, _ptr(self.camera), self.iterations, self.current_sample))

    def render(self, nsamples=1, fused=True):
        """nsamples x Scene::render().  fused=False issues the reference's two launches per
        sample (generate_rays, trace_rays); fused=True is one persistent launch."""
        if fused:
            self._ck(LIB.pt_render(self._h, _ptr(self.camera), self.iterations, int(nsamples)))
        else:
            for _ in range(int(nsamples)):
                self.generate_rays()
                self.trace_rays()
                self.current_sample = self.current_sample + 1                                        # main.cpp:686

    def render_adaptive(self, min_spp, max_spp, threshold, **params):
        """One adaptive frame (current_sample must be 0): pt_render_adaptive, or pt_render_adaptive_ex when any of metric= ("half" /
        "variance"), path= ("render" / "nee"), strategy= ("bsdf" / "light" / "mis") or tonemapped= is given (or the PT_* codes); what
        is not given is pt_adaptive_defaults'.  Returns {"rounds": the boundaries whose round ran, "active_tiles": tiles rendered in
        each of those rounds, "samples": samples spent on the frame}."""
        if params:
            p = AdaptiveParams(**adaptive_defaults())
            p.min_spp, p.max_spp, p.threshold = int(min_spp), int(max_spp), float(threshold)
            names = {"metric": ADAPT_METRICS, "path": ADAPT_PATHS, "strategy": NEE_STRATEGIES, "tonemapped": None}
            for k, v in params.items():
                if k not in names:
                    raise TypeError("unknown adaptive parameter %r" % k)
                if isinstance(v, str):
                    if names[k] is None:
                        raise TypeError("%s must be a number, not %r" % (k, v))
                    if v not in names[k]:
                        raise KeyError("%s must be one of %s (or the PT_* code), not %r" % (k, ", ".join(sorted(names[k])), v))
                    v = names[k][v]
                setattr(p, k, int(v))
            self._ck(LIB.pt_render_adaptive_ex(self._h, _ptr(self.camera), self.iterations, C.byref(p)))
        else:
            self._ck(LIB.pt_render_adaptive(self._h, _ptr(self.camera), self.iterations, int(min_spp), int(max_spp), float(threshold)))
        spp, _ = self.tile_state()
        bounds = adaptive_rounds(min_spp, max_spp)
        active = [int((spp >= b).sum()) for b in bounds]
        ran = [k for k in range(len(bounds)) if active[k] > 0]
        return {"rounds": [bounds[k] for k in ran], "active_tiles": [active[k] for k in ran],
                "samples": int(self.sample_counts().sum(dtype=np.int64))}

    def sample_counts(self):
        """Per local pixel (local_rows x width, int32): the number of samples its colour is the mean of."""
        out = np.empty(self.local_pixels, dtype=np.int32)
        self._ck(LIB.pt_read_sample_counts(self._h, _ptr(out), out.size))
        return out.reshape(-1, self.width)

    def tile_state(self):
        """Per 8x8 tile of the local frame, raster order: (samples rendered int32, last noise estimate float32, +inf: none)."""
        n = ((self.width + 7) // 8) * ((self.local_pixels // self.width + 7) // 8)
        spp = np.empty(n, dtype=np.int32)
        err = np.empty(n, dtype=np.float32)
        self._ck(LIB.pt_read_tile_state(self._h, _ptr(spp), _ptr(err), n))
        return spp, err

    # -- next-event estimation with MIS (include/pt_api.h pins the estimator)
    def render_nee(self, nsamples=1, strategy="mis"):
        """nsamples samples of pt_render's estimator with explicit light sampling (pt_render_nee), into the same running mean.
        strategy: "bsdf" (exactly render()), "light" or "mis" (or PT_NEE_*).  rnds and rays end as render() leaves them."""
        code = NEE_STRATEGIES[strategy] if isinstance(strategy, str) else int(strategy)
        self._ck(LIB.pt_render_nee(self._h, _ptr(self.camera), self.iterations, int(nsamples), code))

    def debug_light_table(self):
        """(orig_tri int32, cdf float32): the lights pt_render_nee samples, in packed order, with their add-order triangle index."""
        n = C.c_int64()
        self._ck(LIB.pt_debug_light_table(self._h, None, None, 0, C.byref(n)))
        tri = np.zeros(n.value, dtype=np.int32)
        cdf = np.zeros(n.value, dtype=np.float32)
        self._ck(LIB.pt_debug_light_table(self._h, _ptr(tri), _ptr(cdf), n.value, C.byref(n)))
        return tri, cdf

    # -- the light hierarchy of render_nee (option "light_tree"; include/pt_api.h pins the tree, the walk and the probabilities)
    def debug_light_tree(self):
        """pt_debug_light_tree: (nodes, orig_tri).  nodes is a structured array, one record per node in depth-first order, with the fields
        c (3 float32), r, phi (float32) and first, count, right (int32): the sphere around the node's lights, their summed weight, its range
        [first, first + count) of tree-order lights and its right child (the left one is the next node; count 1: a leaf).  orig_tri: the
        add-order triangle index of every light in tree order.  Host only; works on a host-only context."""
        nn, nl = C.c_int64(), C.c_int64()
        self._ck(LIB.pt_debug_light_tree(self._h, None, 0, C.byref(nn), None, 0, C.byref(nl)))
        nodes = np.zeros(nn.value, dtype=LIGHT_TREE_NODE)
        tri = np.zeros(nl.value, dtype=np.int32)
        self._ck(LIB.pt_debug_light_tree(self._h, _ptr(nodes), nn.value, C.byref(nn), _ptr(tri), nl.value, C.byref(nl)))
        return nodes, tri

    def debug_light_tree_eval(self, points, normals, u0, tris, on_device=False):
        """pt_debug_light_tree_eval: both walks of the light hierarchy per item -- points (n, 3) the origins o, normals (n, 3) the cull normals
        G (zero: nothing is culled), u0 (n,) in [0, 1), tris (n,) add-order triangle indices.  Returns a structured array with the fields
        tri (the add-order triangle the walk picks with u0), p (its probability P), p_weight (the weight walk's P of tris[i], 0 where that is
        no light) and slot (the pick's tree-order index).  on_device: by the kernel k_debug_light_tree instead of the library's host code."""
        points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        n = points.shape[0]
        normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(n, 3)
        u0 = np.ascontiguousarray(u0, dtype=np.float32).reshape(n)
        tris = np.ascontiguousarray(tris, dtype=np.int32).reshape(n)
        out = np.zeros(n, dtype=LIGHT_TREE_EVAL)
        self._ck(LIB.pt_debug_light_tree_eval(self._h, _ptr(points), _ptr(normals), _ptr(u0), _ptr(tris), n, _ptr(out), 1 if on_device else 0))
        return out

    # -- environment lighting for render_nee (include/pt_api.h pins the map, its distribution and the estimator)
    def set_environment(self, rgb, **params):
        """pt_set_environment: rgb (h, w, 3) float, row 0 at the +y pole; params override pt_environment_defaults (scale, yaw_degrees,
        select).  While it is set only render_nee renders."""
        rgb = np.ascontiguousarray(rgb, dtype=np.float32)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError("rgb must have shape (h, w, 3)")
        p = EnvironmentParams(**environment_defaults())
        for k, v in params.items():
            if k not in p.as_dict():
                raise TypeError("unknown environment parameter %r" % k)
            setattr(p, k, v)
        self._ck(LIB.pt_set_environment(self._h, _ptr(rgb), rgb.shape[1], rgb.shape[0], C.byref(p)))

    def clear_environment(self):
        self._ck(LIB.pt_clear_environment(self._h))

    def debug_environment(self):
        """The tables render_nee samples: {"row_cdf" (h,), "col_cdf" (h, w), "pdf" (h, w): p_env per texel, "P_env": the effective
        probability of choosing the sky at a lobe vertex}."""
        w, h, pe = C.c_int32(), C.c_int32(), C.c_float()
        self._ck(LIB.pt_debug_environment(self._h, C.byref(w), C.byref(h), None, None, None, 0, None))
        row = np.zeros(h.value, dtype=np.float32)
        col = np.zeros((h.value, w.value), dtype=np.float32)
        pdf = np.zeros((h.value, w.value), dtype=np.float32)
        self._ck(LIB.pt_debug_environment(self._h, C.byref(w), C.byref(h), _ptr(row), _ptr(col), _ptr(pdf), col.size, C.byref(pe)))
        return {"row_cdf": row, "col_cdf": col, "pdf": pdf, "P_env": float(pe.value)}

    # -- point, spot and directional lights for render_nee (include/pt_api.h pins the set, the selection and the estimator)
    def set_lights(self, lights, select=0.5):
        """pt_set_lights: replaces the whole set with `lights` (api.point_light / spot_light / directional_light, or their descriptions
        as light_from takes them; an empty list clears it); select = the probability a lobe vertex samples the set rather than the sky or an emitter.  While a pickable light is held
        only render_nee ("light" / "mis") and render_adaptive(path="nee") render."""
        lights = [l if isinstance(l, Light) else light_from(l) for l in lights]
        arr = (Light * max(len(lights), 1))(*lights)
        p = LightsParams(float(select))
        self._ck(LIB.pt_set_lights(self._h, arr, len(lights), C.byref(p)))

    def clear_lights(self):
        self._ck(LIB.pt_clear_lights(self._h))

    def debug_lights(self):
        """What render_nee samples: {"records" (n, 16) float32 as uploaded ({position, type bits}, {axis, cos_inner}, {intensity,
        cos_outer}, {P_light, 0, 0, 0}), "cdf" (n,), "P_light" (n,), "P_ana": the effective probability of choosing the set at a lobe
        vertex of the scene as uploaded}."""
        n, pa = C.c_int64(), C.c_float()
        self._ck(LIB.pt_debug_lights(self._h, None, None, None, 0, C.byref(n), None))
        rec = np.zeros((n.value, 16), dtype=np.float32)
        cdf = np.zeros(n.value, dtype=np.float32)
        pl = np.zeros(n.value, dtype=np.float32)
        self._ck(LIB.pt_debug_lights(self._h, _ptr(rec), _ptr(cdf), _ptr(pl), n.value, C.byref(n), C.byref(pa)))
        return {"records": rec, "cdf": cdf, "P_light": pl, "P_ana": float(pa.value)}

    # -- sphere lights and suns for render_nee (include/pt_api.h pins the set, the selection and the estimator)
    def set_area_lights(self, lights, select=0.5):
        """pt_set_area_lights: replaces the whole set with `lights` (api.sphere_light / sun_light, or their descriptions as area_light_from
        takes them; an empty list clears it); select = the probability a lobe vertex samples the set rather than anything else.  While a
        pickable light is held only render_nee (every strategy) and render_adaptive(path="nee") render."""
        lights = [l if isinstance(l, AreaLight) else area_light_from(l) for l in lights]
        arr = (AreaLight * max(len(lights), 1))(*lights)
        p = AreaLightsParams(float(select))
        self._ck(LIB.pt_set_area_lights(self._h, arr, len(lights), C.byref(p)))

    def clear_area_lights(self):
        self._ck(LIB.pt_clear_area_lights(self._h))

    def debug_area_lights(self):
        """What render_nee samples, in table order (spheres first): {"records" (n, 12) float32 as uploaded, "order" (n,) each light's index
        in the list that was set, "cdf" (n,), "P_light" (n,), "n_sphere", "P_area": the effective probability of choosing the set for the
        scene as uploaded}."""
        n, ns, pa = C.c_int64(), C.c_int32(), C.c_float()
        self._ck(LIB.pt_debug_area_lights(self._h, None, None, None, None, 0, C.byref(n), None, None))
        rec = np.zeros((n.value, 12), dtype=np.float32)
        order = np.zeros(n.value, dtype=np.int32)
        cdf = np.zeros(n.value, dtype=np.float32)
        pl = np.zeros(n.value, dtype=np.float32)
        self._ck(LIB.pt_debug_area_lights(self._h, _ptr(rec), _ptr(order), _ptr(cdf), _ptr(pl), n.value, C.byref(n), C.byref(ns), C.byref(pa)))
        return {"records": rec, "order": order, "cdf": cdf, "P_light": pl, "n_sphere": int(ns.value), "P_area": float(pa.value)}

    def debug_area_light_eval(self, origins=None, lights=None, u=None, rays=None):
        """pt_debug_area_light_eval: the device's sample function on origins (n, 3), lights (n,) in table order and u (n, 2), and its hit
        function on rays (m, 7) {origin, unit direction, t_max}.  Returns (samples, hits) as arrays of AREA_LIGHT_SAMPLE / AREA_LIGHT_HIT."""
        origins = np.ascontiguousarray(np.zeros((0, 3)) if origins is None else origins, dtype=np.float32).reshape(-1, 3)
        lights = np.ascontiguousarray(np.zeros(0) if lights is None else lights, dtype=np.int32).reshape(-1)
        u = np.ascontiguousarray(np.zeros((0, 2)) if u is None else u, dtype=np.float32).reshape(-1, 2)
        rays = np.ascontiguousarray(np.zeros((0, 7)) if rays is None else rays, dtype=np.float32).reshape(-1, 7)
        n, m = origins.shape[0], rays.shape[0]
        if lights.shape[0] != n or u.shape[0] != n:
            raise ValueError("debug_area_light_eval: origins, lights and u must have one entry per sample item")
        samples = np.zeros(n, dtype=AREA_LIGHT_SAMPLE)
        hits = np.zeros(m, dtype=AREA_LIGHT_HIT)
        self._ck(LIB.pt_debug_area_light_eval(self._h, _ptr(origins) if n else None, _ptr(lights) if n else None, _ptr(u) if n else None, n,
                                              _ptr(samples) if n else None, _ptr(rays) if m else None, m, _ptr(hits) if m else None))
        return samples, hits

    # -- per-pixel variance of the mean luminance (option "moments"; include/pt_api.h pins both the fold and the read-out)
    def read_variance(self):
        """Per local pixel (local_rows x width, float32): the variance of its mean luminance, +inf below two samples.
        The frame must have been rendered with set_option("moments", 1) from its first sample."""
        out = np.empty(self.local_pixels, dtype=np.float32)
        self._ck(LIB.pt_read_variance(self._h, _ptr(out), out.size))
        return out.reshape(-1, self.width)

    def device_variance(self):
        """Device pointer of the same read-out (4 B per local pixel), computed on the context's stream; raises like read_variance
        (PT_ENODEVICE on a host-only context, PT_EINVAL when the frame's moments are not valid)."""
        ptr = LIB.pt_device_variance(self._h)
        if not ptr:
            raise PtError(PT_ENODEVICE if self._host_only else PT_EINVAL, (LIB.pt_last_error(self._h) or b"").decode())
        return ptr

    # -- guide buffers + a-trous denoiser (include/pt_api.h pins both)
    def render_aovs(self, subpixels=1, specular_depth=4, shading="geometric"):
        """Guide buffers of the current view: albedo, normal, depth per local pixel; touches no render state.  shading="geometric"
        (pt_render_aovs): the geometric normal and the material's kd; "shaded" (pt_render_aovs_ex, PT_AOV_SHADED): the shading normal and
        the textured albedo of the NEE path under options "smooth_normals" / "textures" as they are now.  With set_option("aov_lights", 1)
        and an area set with a non-black light held, either form also sees the sphere lights and the suns (stat "aov_lights")."""
        if shading not in AOV_SHADING:
            raise ValueError("shading must be 'geometric' or 'shaded', not %r" % (shading,))
        if AOV_SHADING[shading] == PT_AOV_GEOMETRIC:
            self._ck(LIB.pt_render_aovs(self._h, _ptr(self.camera), int(subpixels), int(specular_depth)))
            return
        p = AovParams(int(subpixels), int(specular_depth), PT_AOV_SHADED)
        self._ck(LIB.pt_render_aovs_ex(self._h, _ptr(self.camera), C.byref(p)))

    def read_aovs(self):
        """(albedo_rgbm, normal_depth), each (local_pixels, 4) float32: {r, g, b, material or -1}, {nx, ny, nz, depth or -1}.  The material
        is the index of the first sub-pixel's terminal hit, -1 for a miss, and in lit guides (option "aov_lights") -2 - j where that chain
        ended on the sphere light or under the sun of record j of debug_area_lights()."""
        alb = np.empty((self.local_pixels, 4), dtype=np.float32)
        nd = np.empty((self.local_pixels, 4), dtype=np.float32)
        self._ck(LIB.pt_read_aovs(self._h, _ptr(alb), _ptr(nd), alb.shape[0]))
        return alb, nd

    def denoise(self, **params):
        """pt_denoise with pt_denoise_defaults overridden by params; returns the denoised frame like read_colors()."""
        p = DenoiseParams(**denoise_defaults())
        for k, v in params.items():
            if k not in p.as_dict():
                raise TypeError("unknown denoise parameter %r" % k)
            setattr(p, k, v)
        self._ck(LIB.pt_denoise(self._h, C.byref(p)))
        return self.read_denoised()

    def denoise_variance(self, **params):
        """pt_denoise_variance with pt_denoise_variance_defaults overridden by params; returns the filtered frame like read_colors(),
        with the filtered variance in column 3.  Needs guides (render_aovs) and a frame rendered with set_option("moments", 1)."""
        p = DenoiseVarianceParams(**denoise_variance_defaults())
        for k, v in params.items():
            if k not in p.as_dict():
                raise TypeError("unknown denoise_variance parameter %r" % k)
            setattr(p, k, v)
        self._ck(LIB.pt_denoise_variance(self._h, C.byref(p)))
        return self.read_denoised()

    # -- temporal accumulation with reprojection (include/pt_api.h pins it)
    def temporal_accumulate(self, **params):
        """pt_temporal_accumulate with pt_temporal_defaults overridden by params: blends this frame (rendered with set_option("moments", 1),
        guides from render_aovs with the frame's camera) into the reprojected history.  Returns rgbv like read_temporal()."""
        p = TemporalParams(**temporal_defaults())
        for k, v in params.items():
            if k not in p.as_dict():
                raise TypeError("unknown temporal parameter %r" % k)
            setattr(p, k, v)
        self._ck(LIB.pt_temporal_accumulate(self._h, C.byref(p)))
        return self.read_temporal()[0]

    def read_temporal(self):
        """(rgbv (local_pixels, 4) float32 {r, g, b, variance of the mean}, n (local_pixels,) float32 samples behind it) of the last
        temporal_accumulate."""
        rgbv = np.empty((self.local_pixels, 4), dtype=np.float32)
        n = np.empty(self.local_pixels, dtype=np.float32)
        self._ck(LIB.pt_read_temporal(self._h, _ptr(rgbv), _ptr(n), n.size))
        return rgbv, n

    def device_temporal(self):
        """Device pointer of the last temporal_accumulate's colour, {r, g, b, m2} per local pixel (None before the first)."""
        return LIB.pt_device_temporal(self._h)

    def denoise_temporal(self, **params):
        """denoise_variance's filter (same params) on the last temporal_accumulate's colour and variance; returns like denoise_variance."""
        p = DenoiseVarianceParams(**denoise_variance_defaults())
        for k, v in params.items():
            if k not in p.as_dict():
                raise TypeError("unknown denoise_temporal parameter %r" % k)
            setattr(p, k, v)
        self._ck(LIB.pt_denoise_temporal(self._h, C.byref(p)))
        return self.read_denoised()

    # -- variance-gated firefly filter (include/pt_api.h pins it)
    def despeckle(self, **params):
        """pt_despeckle with pt_despeckle_defaults overridden by params (source: PT_DESPECKLE_FRAME / PT_DESPECKLE_TEMPORAL or "frame" /
        "temporal"): clips the pixels that stand out of their neighbourhood and whose own variance confirms it, and with spread hands
        the clipped energy to the window around them.  Returns (rgbv, flags) like read_despeckled()."""
        p = _despeckle_params("despeckle", params)
        self._ck(LIB.pt_despeckle(self._h, C.byref(p)))
        return self.read_despeckled()

    def read_despeckled(self):
        """(rgbv (local_pixels, 4) float32 {r, g, b, variance of the mean}, flags (local_pixels,) int32: 0 kept, 1 clipped, 2 not live)
        of the last despeckle."""
        rgbv = np.empty((self.local_pixels, 4), dtype=np.float32)
        flags = np.empty(self.local_pixels, dtype=np.int32)
        self._ck(LIB.pt_read_despeckled(self._h, _ptr(rgbv), _ptr(flags), flags.size))
        return rgbv, flags

    def device_despeckled(self):
        """Device pointer of the last despeckle's {r, g, b, v} per local pixel (None before the first)."""
        return LIB.pt_device_despeckled(self._h)

    def denoise_despeckled(self, **params):
        """denoise_variance's filter (same params) on the last despeckle's colour and variance; returns like denoise_variance."""
        p = DenoiseVarianceParams(**denoise_variance_defaults())
        for k, v in params.items():
            if k not in p.as_dict():
                raise TypeError("unknown denoise_despeckled parameter %r" % k)
            setattr(p, k, v)
        self._ck(LIB.pt_denoise_despeckled(self._h, C.byref(p)))
        return self.read_denoised()

    def debug_despeckle(self, rgbv, **params):
        """pt_debug_despeckle: the despeckle kernel on a caller's frame rgbv (h, w, 4) float32 {r, g, b, v}; source is ignored.
        Returns (rgbv (h, w, 4), flags (h, w))."""
        a = np.ascontiguousarray(rgbv, dtype=np.float32)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError("rgbv must have shape (h, w, 4)")
        p = _despeckle_params("debug_despeckle", params)
        out = np.empty_like(a)
        flags = np.empty(a.shape[:2], dtype=np.int32)
        self._ck(LIB.pt_debug_despeckle(self._h, _ptr(a), a.shape[1], a.shape[0], C.byref(p), _ptr(out), _ptr(flags)))
        return out, flags

    # -- display stage (include/pt_api.h pins it)
    def display(self, **params):
        """pt_display with pt_display_defaults overridden by params (source, metering, curve and encoding also by name: "frame" /
        "denoised" / "temporal" / "despeckled", "manual" / "auto", "linear" / "reinhard" / "aces", "srgb" / "linear"): exposure, bloom,
        tone curve and encoding of one of the HDR results, on the device.  Nothing is read back: read_display(), display_info()."""
        p = _display_params("display", params)
        self._ck(LIB.pt_display(self._h, C.byref(p)))

    def read_display(self):
        """(rgba (local_pixels, 4) float32 {r, g, b, 1}, row 0 the bottom; rgb8 (H, W, 3) uint8, top row first) of the last display."""
        rgba = np.empty((self.local_pixels, 4), dtype=np.float32)
        rgb8 = np.empty((rgba.shape[0] // self.width, self.width, 3), dtype=np.uint8)
        self._ck(LIB.pt_read_display(self._h, _ptr(rgba), _ptr(rgb8), rgba.shape[0]))
        return rgba, rgb8

    def device_display(self):
        """Device pointer of the last display's {r, g, b, 1} per local pixel, the bytes right behind (None before the first)."""
        return LIB.pt_device_display(self._h)

    def display_info(self):
        """pt_display_info as a dict: exposure, mean_log2, n_metered, n_dark, n_nonfinite, levels.  Synchronises."""
        info = DisplayInfo()
        self._ck(LIB.pt_display_info(self._h, C.byref(info)))
        return info.as_dict()

    def display_histogram(self):
        """The 256 luminance bins of the last display (uint32)."""
        out = np.empty(256, dtype=np.uint32)
        self._ck(LIB.pt_debug_display_histogram(self._h, _ptr(out)))
        return out

    def display_reset(self):
        """pt_display_reset: the next display adapts from nothing."""
        self._ck(LIB.pt_display_reset(self._h))

    def write_display_ppm(self, path):
        """The last display's bytes as a binary P6 file."""
        self._ck(LIB.pt_write_display_ppm(self._h, os.fsencode(path)))

    def debug_display(self, frame, prev_exposure=None, **params):
        """pt_debug_display: the display kernels on a caller's frame (h, w, 4) float32 {r, g, b, .}; source is ignored, prev_exposure
        stands in for the remembered exposure.  Returns (rgba (h, w, 4), rgb8 (h, w, 3) top row first, hist (256,), info dict)."""
        a = np.ascontiguousarray(frame, dtype=np.float32)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError("frame must have shape (h, w, 4)")
        p = _display_params("debug_display", params)
        out = np.empty_like(a)
        rgb8 = np.empty(a.shape[:2] + (3,), dtype=np.uint8)
        hist = np.empty(256, dtype=np.uint32)
        info = DisplayInfo()
        self._ck(LIB.pt_debug_display(self._h, _ptr(a), a.shape[1], a.shape[0], C.byref(p), 0.0 if prev_exposure is None else float(prev_exposure),
                                      _ptr(out), _ptr(rgb8), _ptr(hist), C.byref(info)))
        return out, rgb8, hist, info.as_dict()

    def read_denoised(self):
        out = np.empty((self.local_pixels, 4), dtype=np.float32)
        self._ck(LIB.pt_read_denoised(self._h, _ptr(out), out.shape[0]))
        return out

    def device_denoised(self):
        """Device pointer of the last pt_denoise result (None before the first)."""
        return LIB.pt_device_denoised(self._h)

    def sync(self):
        self._ck(LIB.pt_sync(self._h))

    # -- seeds
    def seed_default(self):
        self._ck(LIB.pt_seed_default(self._h))

    def upload_seeds(self, seeds):
        seeds = np.ascontiguousarray(seeds, dtype=np.int32)
        self._ck(LIB.pt_upload_seeds(self._h, _ptr(seeds), seeds.size))

    # -- readback
    @property
    def local_pixels(self):
        v = C.c_int64()
        self._ck(LIB.pt_local_pixel_count(self._h, C.byref(v)))
        return v.value

    def local_pixel_ids(self):
        out = np.empty(self.local_pixels, dtype=np.int32)
        self._ck(LIB.pt_local_pixel_ids(self._h, _ptr(out), out.size))
        return out

    def read_colors(self):
        out = np.empty((self.local_pixels, 4), dtype=np.float32)
        self._ck(LIB.pt_read_colors(self._h, _ptr(out), out.shape[0]))
        return out

    def read_rnds(self):
        out = np.empty(self.local_pixels, dtype=np.int32)
        self._ck(LIB.pt_read_rnds(self._h, _ptr(out), out.size))
        return out

    def read_rays(self):
        out = np.empty(self.local_pixels, dtype=RAY)
        self._ck(LIB.pt_read_rays(self._h, _ptr(out), out.size))
        return out

    # -- frame assembly over RCCL (one process per GPU; the 128-byte id travels by the host's own means)
    @property
    def slab_pixels(self):
        v = C.c_int64()
        self._ck(LIB.pt_slab_pixel_count(self._h, C.byref(v)))
        return v.value

    def comm_init(self, id_bytes):
        buf = (C.c_ubyte * PT_COMM_ID_BYTES).from_buffer_copy(bytes(id_bytes))
        self._ck(LIB.pt_comm_init(self._h, C.cast(buf, C.c_void_p)))

    def gather_frame(self):
        self._ck(LIB.pt_gather_frame(self._h))

    def device_frame(self):
        return LIB.pt_device_frame(self._h)

    def read_frame(self):
        out = np.empty((self.width * self.height, 4), dtype=np.float32)
        self._ck(LIB.pt_read_frame(self._h, _ptr(out), out.shape[0]))
        return out

    # -- image files (what the reference shows through its GL blit, main.cpp:1019-1039)
    def write_pfm(self, path):
        self._ck(LIB.pt_write_pfm(self._h, os.fsencode(path)))

    def write_ppm(self, path, which=0):
        self._ck(LIB.pt_write_ppm(self._h, os.fsencode(path), int(which)))

    def debug_deinterleave(self, gathered):
        gathered = np.ascontiguousarray(gathered, dtype=np.float32).reshape(-1, 4)
        out = np.empty((self.width * self.height, 4), dtype=np.float32)
        self._ck(LIB.pt_debug_deinterleave(self._h, _ptr(gathered), gathered.shape[0], _ptr(out)))
        return out

    def resolve_ldr(self, which=0):
        out = np.empty((self.local_pixels, 4), dtype=np.float32)
        self._ck(LIB.pt_resolve_ldr(self._h, int(which), _ptr(out), out.shape[0]))
        return out

    # -- options / stats / device plumbing
    def set_option(self, key, value):
        self._ck(LIB.pt_set_option(self._h, key.encode(), int(value)))

    def stat(self, key):
        v = C.c_double()
        self._ck(LIB.pt_get_stat(self._h, key.encode(), C.byref(v)))
        return v.value

    def bind_framebuffer(self, colors_ptr, rnds_ptr):
        self._ck(LIB.pt_bind_framebuffer(self._h, C.c_void_p(colors_ptr), C.c_void_p(rnds_ptr)))

    def set_stream(self, stream_ptr):
        self._ck(LIB.pt_set_stream(self._h, C.c_void_p(stream_ptr)))

    def device_colors(self):
        return LIB.pt_device_colors(self._h)

    def device_rnds(self):
        return LIB.pt_device_rnds(self._h)

    # -- introspection (host data)
    def debug_bvh(self):
        nn, nt = C.c_int64(), C.c_int64()
        self._ck(LIB.pt_debug_bvh_sizes(self._h, C.byref(nn), C.byref(nt)))
        nodes = np.zeros((nn.value, 16), dtype=np.float32)
        tris = np.zeros((nt.value, 12), dtype=np.float32)
        meta = np.zeros((nt.value, 2), dtype=np.int32)
        orig = np.zeros(nt.value, dtype=np.int32)
        self._ck(LIB.pt_debug_bvh_copy(self._h, _ptr(nodes), _ptr(tris), _ptr(meta), _ptr(orig)))
        return nodes, tris, meta, orig

    def debug_flat_list(self):
        """The big-triangle list as the traversal tests it: (packets (n, 12) float32, pair mask) -- bit i of the mask: entries i
        and i + 1 are tested as one pair."""
        n = int(self.stat("flat_triangles"))
        pk = np.zeros((n, 12), dtype=np.float32)
        m = C.c_uint32()
        self._ck(LIB.pt_debug_flat_list(self._h, _ptr(pk), C.byref(m)))
        return pk, m.value

    def debug_wide_nodes(self):
        """The 4-wide quantised nodes (pt_wide.cpp) as a structured array; empty when they were not built."""
        n = C.c_int64()
        self._ck(LIB.pt_debug_wide_nodes(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=WIDE_NODE)
        if n.value:
            self._ck(LIB.pt_debug_wide_nodes(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def debug_scene(self):
        nt, nm, no = C.c_int64(), C.c_int64(), C.c_int64()
        self._ck(LIB.pt_debug_scene_sizes(self._h, C.byref(nt), C.byref(nm), C.byref(no)))
        tris = np.zeros(nt.value, dtype=TRIANGLE)
        mats = np.zeros(nm.value, dtype=MATERIAL)
        objs = np.zeros(no.value, dtype=np.int32)
        self._ck(LIB.pt_debug_scene_copy(self._h, _ptr(tris), _ptr(mats), _ptr(objs)))
        return tris, mats, objs

    def debug_closest_hit(self, rays):
        rays = np.ascontiguousarray(rays, dtype=RAY)
        t = np.empty(rays.shape[0], dtype=np.float32)
        tri = np.empty(rays.shape[0], dtype=np.int32)
        self._ck(LIB.pt_debug_closest_hit(self._h, _ptr(rays), rays.shape[0], _ptr(t), _ptr(tri)))
        return t, tri

    def debug_math(self, fn, first, n, bad_cap=8):
        """pt_debug_math: (mismatches, inputs inside the fast path's window, uint32 [k, 2] bit patterns of the first mismatches)."""
        out = np.zeros(3, dtype=np.int64)
        bad = np.zeros((max(int(bad_cap), 1), 2), dtype=np.uint32)
        self._ck(LIB.pt_debug_math(self._h, int(fn), int(first), int(n), _ptr(out), _ptr(bad), int(bad_cap)))
        return int(out[0]), int(out[1]), bad[:min(int(out[2]), int(bad_cap))]

    def debug_spec(self, fn, items):
        """pt_debug_spec: function fn (PT_SPEC_*) of the kernels' spec math on items, an (n, SPEC_WORDS[fn][0]) array of 32-bit words
        (float32 items are passed as their bit patterns) -> (n, SPEC_WORDS[fn][1]) uint32; view it as float32 or int32 as the function's
        columns ask.  Item i runs on lane i % 64 of wave i / 64."""
        wi, wo = SPEC_WORDS[int(fn)]
        items = np.ascontiguousarray(items)
        if items.dtype.itemsize != 4:
            raise ValueError("debug_spec: items must be 32-bit words")
        items = items.view(np.uint32).reshape(-1, wi)
        out = np.empty((items.shape[0], wo), dtype=np.uint32)
        self._ck(LIB.pt_debug_spec(self._h, int(fn), items.shape[0], _ptr(items), _ptr(out)))
        return out

    def debug_shade(self, instance, items, iterations=None):
        """pt_debug_shade: shade_hit<SK, REC> (instance = PT_SHADE_SK | PT_SHADE_REC bits) on items, an (n, SHADE_WORDS_IN) array of
        32-bit words {P.xyz, D.xyz, t, packed ti, seed, inside, L, B, S, R, colour} -> (n, SHADE_WORDS_OUT) uint32 {P.xyz, D.xyz, seed,
        inside, L, B, S, R, colour}, with the context's scene, self.camera and iterations (default self.iterations).  Item i runs on lane
        i % 64 of wave i / 64."""
        items = np.ascontiguousarray(items)
        if items.dtype.itemsize != 4:
            raise ValueError("debug_shade: items must be 32-bit words")
        items = items.view(np.uint32).reshape(-1, SHADE_WORDS_IN)
        out = np.empty((items.shape[0], SHADE_WORDS_OUT), dtype=np.uint32)
        self._ck(LIB.pt_debug_shade(self._h, _ptr(self.camera), int(self.iterations if iterations is None else iterations), int(instance),
                                    items.shape[0], _ptr(items), _ptr(out)))
        return out

    def debug_encounter_rank(self, n):
        out = np.empty(n, dtype=np.int32)
        self._ck(LIB.pt_debug_encounter_rank(self._h, _ptr(out), n))
        return out

    def debug_launch_plan(self, nsamples, cu_count=0):
        """What render(nsamples) would launch on a device of cu_count compute units (host-only contexts too)."""
        out = np.zeros(8, dtype=np.int64)
        self._ck(LIB.pt_debug_launch_plan(self._h, int(nsamples), int(cu_count), _ptr(out)))
        keys = ("block", "waves_per_simd", "schedule", "chunk_spp", "resident_waves", "tiles", "node_mode", "lds_bytes")
        return dict(zip(keys, (int(v) for v in out)))

    def debug_adaptive_list(self):
        """The active tiles the last decision of the held adaptive frame left, in the order the next round would render them."""
        n = C.c_int64()
        self._ck(LIB.pt_debug_adaptive_list(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.int32)
        if n.value:
            self._ck(LIB.pt_debug_adaptive_list(self._h, _ptr(out), n.value, C.byref(n)))
        return out

    def debug_tile_cost(self):
        """After set_option("count_work", 1) + render(n): per 8x8 tile of the local frame, the shader-clock cycles / 64 its wave spent on it."""
        local_rows = self.local_pixels // self.width
        n = ((self.width + 7) // 8) * ((local_rows + 7) // 8)
        out = np.empty(n, dtype=np.uint32)
        self._ck(LIB.pt_debug_tile_cost(self._h, _ptr(out), n))
        return out
