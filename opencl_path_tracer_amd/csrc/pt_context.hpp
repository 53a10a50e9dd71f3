// pt_context.hpp -- what the host-side translation units of libptamd.so share: the context behind the opaque pt_context* of
// include/pt_api.h, the error / HIP-call conventions, the host thread pool, and the functions that cross file boundaries.
//   pt_host.cpp     the C ABI: constructors, context life cycle, authoring, read-back, options, statistics, debug entry points; the
//                   NEE launch path (light table, the kernel family a launch takes, pt_render_nee)
//   pt_builder.cpp  scene -> tree: encounter ranks of end_Obj, the binned-SAH builder (host) and its orchestration on the device,
//                   big-triangle list, packets, cost boxes; pt_end_obj, pt_upload_triangles
//   pt_launch.cpp   tree -> launches: node placement (LDS / treelet / 4-wide), stack sizing, kernel parameters, the launch policy
//                   (instance, schedule, pass length), the wavefront chains; pt_generate_rays, pt_trace_rays, pt_render, pt_sync
//   pt_post.cpp     the post-process chain: guides, a-trous, variance, variance-guided a-trous, temporal, despeckle, display, and
//                   the one place that says what makes their results stale
//   pt_smooth.cpp, pt_texture.cpp, pt_lens.cpp, pt_env.cpp, pt_lights.cpp, pt_arealights.cpp, pt_medium.cpp, pt_interior.cpp,
//   pt_lighttree.cpp    one scene feature each: its authoring calls, its device copies (*_prepare), its debug entry points
//   pt_obj.cpp, pt_image.cpp, pt_wide.cpp    the OBJ / MTL loader, the image files, the 4-wide collapse on the host
// Internal: not part of the ABI.  (`using namespace ptamd` below is deliberate: these files ARE the library.)
#pragma once

#include "pt_devbuf.hpp"
#include "pt_internal.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <numeric>
#include <queue>
#include <thread>

using namespace ptamd;

namespace ptamd {
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
};
// Device memory.  Every device array a context holds is a DeviceArray field of pt_context: it is freed when the context is deleted
// (pt_destroy synchronises the device first), and replaced or grown through replace / reserve / move-assignment, never by hand.  A
// failed allocation leaves the field empty and its hipError_t in HipAlloc::last (PT_ALLOC below reports it).
#pragma GCC visibility push(hidden)
struct HipAlloc {
    static inline thread_local hipError_t last = hipSuccess;
    static bool alloc(void** p, size_t bytes) { return (last = hipMalloc(p, bytes)) == hipSuccess; }
    static void free(void* p) { (void)hipFree(p); }
};
template <class T>
using DeviceArray = DevBuf<T, HipAlloc>;
// the untyped temporary of the debug entry points and the staging copies: at least 16 bytes, freed on every exit path
struct DeviceBuf {
    void* p = nullptr;
    ~DeviceBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 16)); }
};
#pragma GCC visibility pop
}  // namespace ptamd

struct pt_context {
    int device = -1;
    bool has_device = false;
    int32_t W = 0, H = 0;
    int32_t rank = 0, world = 1, rows_per_block = 8;
    int32_t local_rows = 0;
    int64_t npix = 0;  // local pixels
    int64_t slab_pix = 0;  // max over ranks of the local pixel count: what every rank contributes to the all-gather

    // ---- frame assembly (pt_comm.hip)
    void* comm = nullptr;          // ncclComm_t
    DeviceArray<float4> d_gathered;  // world x slab_pix
    DeviceArray<float4> d_frame;     // W x H
    uint64_t render_epoch = 0;     // bumped by every call that writes colors
    uint64_t frame_epoch = ~0ull;  // render_epoch at the last pt_gather_frame: d_frame is served only while they are equal

    // ---- authoring state (Scene members, main.cpp:365-372)
    std::vector<pt_triangle> tris;  // add order
    std::vector<int32_t> obj_begin;
    int32_t tri_shift = 0;
    std::vector<pt_material> mats;
    std::vector<int32_t> enc_rank;  // per add-order triangle
    int32_t next_rank = 0;
    bool tris_uploaded = false, mats_uploaded = false;

    // ---- packed scene (host copies kept for the debug getters)
    std::vector<Node64> nodes;
    std::vector<Node4q> nodes4;   // the same tree collapsed to 4-wide quantised nodes (empty: not built), pt_wide.cpp
    int wide_pending = 0;         // most entries a wide traversal can have pushed when it visits an interior node
    std::vector<TriPacket> packets;
    bool host_packets_stale = false;   // device-built tree: packets / meta behind the big-triangle list live on the device only until a debug getter asks
    std::vector<TriMeta> meta;
    std::vector<int32_t> orig;
    int bvh_depth = 0;
    int interior_depth = 0;   // depth of the deepest interior node of the packed tree (root: 0): sizes the traversal stacks
    int n_flat = 0;             // packed triangles [0, n_flat): the big-triangle list tested before the tree
    int n_fbox = 0;             // its distinct bounding boxes: representative packet and the listed triangles each one covers
    uint8_t fbox_rep[32] = {};
    uint32_t fbox_mask[32] = {};
    uint32_t fpair_mask = 0;    // bit i: listed triangles i and i + 1 are the halves of one wall, tested once (plan_flat_pairs)
    uint32_t fpair_canon = 0;   // bit i: the zero components of listed triangle i's N are +0 in the test copy
    uint64_t fpair_rot = 0;     // two bits per listed triangle: cyclic rotation of its corners in the list's TEST copy (0: as authored)

    // ---- device buffers
    DeviceArray<float4> d_nodes;
    DeviceArray<float4> d_nodes4;
    DeviceArray<uint32_t> d_stack_ovf;   // kNodesWide: stack entries past the LDS part, [entry][lane of the grid]
    size_t stack_ovf_lanes = 0;
    DeviceArray<float4> d_tris;
    DeviceArray<TriMeta> d_meta;
    DeviceArray<pt_material> d_mats;
    // per-triangle shading records (ShadeRec): built from d_tris, d_meta and d_mats at the next render launch that reads them after
    // any of the three was written (every writer sets shaderec_dirty; ensure_shade_records, pt_launch.cpp)
    DeviceArray<ShadeRec> d_shaderec;
    bool shaderec_dirty = true;
    int32_t mats_on_device = 0;        // materials d_mats holds (ctx->mats can run ahead of it until the next pt_upload_materials)
    // the framebuffer: the kernels read d_rnds / d_colors, which point into rnds_own / colors_own until pt_bind_framebuffer binds the
    // caller's arrays; a bound (borrowed) array is never freed here, and its owner is empty from then on
    int32_t* d_rnds = nullptr;
    float4* d_colors = nullptr;
    DeviceArray<int32_t> rnds_own;
    DeviceArray<float4> colors_own;
    DeviceArray<pt_ray> d_rays;
    DeviceArray<float4> d_ldr;
    DeviceArray<unsigned long long> d_stats;
    // wavefront variant: path state + queues (allocated on first use)
    DeviceArray<float4> d_wf_state;   // per local pixel: 4 float4 worth of path factors + colour (5 x 12 B), 8 + 4 float4 of ray streams (rsA, rsB; rsC), 2 float2 of hits
    DeviceArray<int32_t> d_wf_queues; // 3 x npix int32 (class queues)
    std::vector<float> cost_boxes;  // 6 floats per complex object (wavefront cost classes)
    DeviceArray<uint32_t> d_wf_counters;   // kWfMaxChains x (kWfMaxBounces + 4) rows
    hipStream_t wf_stream[kWfMaxChains] = {};   // chains 1.. of the wavefront variant (chain 0 runs on `stream`)
    hipEvent_t wf_event[kWfMaxChains] = {};
    int poll_timeout_ms = 10000;         // chained passes: a wave gives a tile's previous pass this long before it reports the hand-over lost
    int debug_stall_tile = -1;           // tests: pass 0 of this tile is never published
    bool counters_suspect = false;
    bool launched_since_check = false;   // a persistent launch has been enqueued since the work counter's error word was last read       // a launch failed or lost a hand-over: word 0 / 1 of d_tile_counter may not be back at zero
    int wf_streams = -1;                 // option wf_streams: chains of the wavefront variant (-1: kWfDefaultChains)
    hipStream_t stream = nullptr;

    int32_t current_sample = 0;  // main.cpp:28

    // ---- options
    int variant = 0;
    int lds_scene = 2;   // 2: stage BVH nodes in LDS -- the whole tree when it fits next to two 512-thread blocks per
                         // CU, otherwise its top (`treelet`); 0: every node through L1/L2
    int treelet = 0;     // nodes of a large tree to stage in LDS: 0 none (default: with the big-triangle list in place the
                         // treelet no longer pays, profiles/r02/s_*), -1 what fits one 1,024-thread block per CU, n
    int treelet_nodes = 0;   // decided at upload: nodes [0, treelet_nodes) are the re-indexed top of the tree
    int timing = 0;
    int count_work = 0;
    int bvh_on_device = 0;
    int bvh_median_splits = 0;   // ranges the host builder split at the median in the last upload (what the device SAH builder hands back)
    double bvh_build_ms = 0.0;
    int cu_count = 256;
    int persistent = 1;   // 1: megakernel waves pull tiles from a counter (grid = what fits the chip)
    DeviceArray<uint32_t> d_tile_counter;
    DeviceArray<uint32_t> d_tile_done;
    DeviceArray<uint32_t> d_tile_cost;   // count_work: per tile, cycles / 64 its waves spent on it in the last launch (pt_debug_tile_cost)
    // adaptive frames (pt_render_adaptive; allocated on first use): per local pixel the colour at half the tile's samples; per tile of
    // the local frame the samples rendered, the last noise estimate and the active flag; the active tiles in ascending order + their count
    DeviceArray<float4> d_adapt_snap;
    DeviceArray<int32_t> d_adapt_spp;
    DeviceArray<float> d_adapt_err;
    DeviceArray<uint8_t> d_adapt_active;
    DeviceArray<int32_t> d_adapt_list;   // n_tiles entries, then the count word
    int32_t* h_adapt_count = nullptr;  // pinned
    bool adaptive_frame = false;       // an adaptive frame is held: pt_render / pt_trace_rays / pt_render_adaptive refuse until pt_set_current_sample(0)
    // ---- the post-process chain (pt_post.cpp).  What says whether a stage's result is current -- aov_valid / shaded / lit / serial / cam,
    // temporal_history, despeckle_valid, display_ran / has_prev -- is written by pt_post.cpp alone: the other files report an upload or
    // an authoring call through post_scene_uploaded, post_shading_inputs_changed and post_area_lights_changed below
    // guide buffers (pt_render_aovs) and the a-trous filter (pt_denoise), allocated on first use: per local pixel albedo_rgbm then
    // normal_depth (2 x npix float4); two ping-pong frames (2 x npix float4); d_denoised points at the one the last pt_denoise left
    DeviceArray<float4> d_aov;
    DeviceArray<float4> d_dn;
    float4* d_denoised = nullptr;
    bool aov_valid = false;            // pt_render_aovs ran and no pt_upload_triangles / pt_upload_materials has made its guides stale
    bool aov_shaded = false;           // the guides are shaded ones (pt_render_aovs_ex, PT_AOV_SHADED): the authoring calls for vertex normals,
                                       // uvs, textures and bindings make them stale too (post_shading_inputs_changed)
    int aov_lights = 0;                // option "aov_lights": guides rendered while an area set with a non-black light is held see its lights
    bool aov_lit = false;              // the last guide launch used a lit instance (stat "aov_lights"): pt_set_area_lights and
                                       // pt_clear_area_lights make such guides stale too
    // option "moments": render launches fold the second moment into colors[].w; moments_valid = every launch of the current frame did
    // (note_moments); the variance read-out (pt_read_variance, pt_denoise_variance) lives in d_variance, allocated on first use
    int moments = 0;
    bool moments_valid = false;
    DeviceArray<float> d_variance;
    // temporal accumulation (pt_temporal_accumulate).  Every frame start bumps frame_serial and records the frame's camera (note_frame;
    // frame_cam_same while every launch of the frame used it byte for byte); pt_render_aovs records its camera and bumps aov_serial.
    // Two history sets in d_temporal, allocated on first use: per set and local pixel {r, g, b, m2}, {nx, ny, nz, depth} of the guides
    // it was made with, {n, material} (40 B; the float4 arrays of both sets, then the float2 ones), and the variance of the mean of the
    // last result in d_temporal_var.  temporal_out: the set the last accumulate wrote (-1: none yet)
    uint64_t frame_serial = 0;
    pt_camera frame_cam = {};
    bool frame_cam_same = false;
    uint64_t aov_serial = 0;
    pt_camera aov_cam = {};
    DeviceArray<float4> d_temporal;
    DeviceArray<float> d_temporal_var;
    int temporal_out = -1;
    bool temporal_history = false;      // set temporal_out is the history of the next accumulate (dropped when the scene is uploaded)
    pt_camera temporal_cam = {};        // the camera of that history
    uint64_t temporal_frame = ~0ull;    // frame_serial of the last accumulate
    uint64_t temporal_aov = ~0ull;      // aov_serial of the guides it used
    // the firefly filter (pt_despeckle), allocated on first use: per local pixel {r, g, b, v}, then v once more as a float array (the
    // variance-guided filter's input), then the flags (24 B).  The result is current (pt_denoise_despeckled) while despeckle_valid --
    // pt_upload_triangles / pt_upload_materials clear it -- and the three serials below are what they were
    DeviceArray<float4> d_despeckle;
    bool despeckle_valid = false;
    int32_t despeckle_source = 0;
    uint64_t despeckle_epoch = 0;            // render_epoch: no launch has written colors since
    uint64_t despeckle_frame = 0;            // frame_serial: no frame has started since
    uint64_t despeckle_temporal = 0;         // temporal_frame (source PT_DESPECKLE_TEMPORAL): no newer accumulate ran
    // the display stage (pt_display), allocated on first use: {r, g, b, 1} per local pixel with the 3 B per pixel right behind it; the
    // bloom pyramid (grown when a call asks for more levels); the histogram and the metering's numbers (DisplayStat), where the
    // exposure of the last call also waits as the next call's E_prev while display_has_prev -- pt_display_reset, pt_upload_triangles
    // and pt_upload_materials clear it
    DeviceArray<float4> d_display;
    DeviceArray<float4> d_display_pyr;
    DeviceArray<DisplayStat> d_display_stat;
    bool display_ran = false;
    bool display_has_prev = false;
    int32_t display_levels = 0;              // bloom levels the last call ran
    // next-event estimation (pt_render_nee): the light table, built on the host at first use after an upload (nee_valid).  Packed
    // triangle index and cdf per light; P_sel / area per packed triangle (0 for non-lights).  Device copies allocated with it.
    std::vector<int32_t> nee_tri;
    std::vector<float> nee_cdf;
    std::vector<float> nee_pdf_area;
    bool nee_valid = false;
    DeviceArray<int32_t> d_nee_tri;
    DeviceArray<float> d_nee_cdf;
    DeviceArray<float> d_nee_pdf_area;
    bool nee_uploaded = false;         // the device copies hold the current table
    std::vector<double> nee_phi, nee_area;     // per light, in table order: area x (E.r + E.g + E.b) and the area, as the table summed them
    // the light hierarchy over that table (option light_tree, pt_lighttree.cpp; pinned in include/pt_api.h): built on the host at first use
    // after the table (lt_valid; a new table invalidates it).  Eight floats per node; packed triangle and (float)(1 / area) per light in tree
    // order; the tree-order index per packed triangle (-1 for non-lights)
    int light_tree = 0;                // option light_tree
    std::vector<float> lt_nodes;
    std::vector<int32_t> lt_tri, lt_slot;
    std::vector<float> lt_inv_area;
    int32_t lt_depth = 0;
    bool lt_valid = false, lt_uploaded = false;
    DeviceArray<float4> d_lt_nodes;
    DeviceArray<int32_t> d_lt_tri;
    DeviceArray<int32_t> d_lt_slot;
    DeviceArray<float> d_lt_inv_area;
    // the environment of pt_render_nee (pt_set_environment, pt_env.cpp): the map with p_env = P(texel) / Omega(row) in .w, the row
    // marginal cdf [h] and the per-row column cdfs [h][w]; env_dist: some weight is non-zero.  Device copies made by pt_set_environment.
    bool env_set = false, env_dist = false;
    int32_t env_w = 0, env_h = 0;
    float env_scale = 1.0f, env_yaw = 0.0f, env_select = 0.5f;   // yaw in radians
    std::vector<float4> env_texels;
    std::vector<float> env_row_cdf, env_col_cdf;
    DeviceArray<float4> d_env_texels;
    DeviceArray<float> d_env_row_cdf;
    DeviceArray<float> d_env_col_cdf;
    // smooth shading (option smooth_normals, pt_set_vertex_normals; pinned in include/pt_api.h): 9 floats per add-order triangle as
    // recorded, all zero where a triangle has none (shorter than tris: the rest has none).  d_vnormals: 3 float4 per packed triangle,
    // packed by k_pack_vertex_normals (pt_smooth.hip) at the first smooth launch after the normals or the uploaded triangles changed
    int smooth_normals = 0;
    std::vector<float> vnormals;
    bool vnormals_dirty = true;
    DeviceArray<float4> d_vnormals;
    // albedo textures (option textures, pt_add_texture / pt_set_vertex_uvs / pt_set_material_texture; pinned in include/pt_api.h).
    // Host: every texture's texels back to back (8 B each: three halves r g b and 16 zero bits) with one descriptor per texture, the
    // binding per material (-1: none; shorter than mats: the rest has none) and 6 floats per add-order triangle (NaN where a triangle
    // has no uvs; shorter than tris: the rest has none).  The device copies are made by texture_prepare (pt_texture.cpp) at the first
    // textured launch after any of them, the uploaded triangles or the uploaded materials changed; d_vuvs: 2 float4 per packed
    // triangle (k_pack_vertex_uvs, pt_texture.hip); d_mat_tex: per material on the device the binding, -1 where its type is not 0
    int textures = 0;
    std::vector<uint64_t> tex_texels;
    std::vector<TexDesc> tex_desc;
    std::vector<int32_t> mat_tex;
    std::vector<float> vuvs;
    bool tex_dirty = true, vuvs_dirty = true;      // textures / bindings / materials; uvs / triangles
    DeviceArray<uint2> d_tex_texels;
    DeviceArray<TexDesc> d_tex_desc;
    DeviceArray<int32_t> d_mat_tex;
    DeviceArray<float4> d_vuvs;
    int obj_textures_loaded = 0, obj_textures_skipped = 0;      // map_Kd lines of the last pt_add_obj
    int obj_pieces = 0;                                         // pieces its parse cut the file into
    // rough metal (option glossy; pinned in include/pt_api.h): material type 4 is a GGX lobe vertex in pt_render_nee.  The glossy k_nee
    // instances run only when the option is on AND the materials uploaded last hold a type-4 one; every other frame is today's launch
    int glossy = 0;
    bool glossy_mats = false;          // pt_upload_materials saw a material of type 4
    // coated diffuse (option coated; pinned in include/pt_api.h): material type 5 is a two-lobe vertex in pt_render_nee.  The coated k_nee
    // instances run only when the option is on AND the materials uploaded last hold a type-5 one; every other frame is today's launch
    int coated = 0;
    bool coated_mats = false;          // pt_upload_materials saw a material of type 5
    // rough dielectric (option frosted; pinned in include/pt_api.h): material type 6 is a reflecting / refracting lobe vertex in
    // pt_render_nee.  The frosted k_nee instances run only when the option is on AND the materials uploaded last hold a type-6 one
    int frosted = 0;
    bool frosted_mats = false;         // pt_upload_materials saw a material of type 6
    // thin lens (pt_set_lens; pinned in include/pt_api.h): pt_render_nee and the NEE path of pt_render_adaptive_ex start their paths on the
    // lens ray while lens_set && lens_aperture > 0 (the lens instances of k_nee); every other frame is today's launch
    bool lens_set = false;
    float lens_aperture = 0.0f, lens_focus = 1.0f;
    // analytic lights (pt_set_lights, pt_lights.cpp; pinned in include/pt_api.h): the set as validated, and what the kernel samples -- per
    // light a 16-float record (LightsView, pt_internal.hpp), the float cdf and P_light by the counting rule.  lights_pickable: some
    // P_light > 0; only then do pt_render_nee and the NEE path of pt_render_adaptive_ex launch the lights instances of k_nee, and do the
    // other paths refuse.  Device copies made by pt_set_lights
    std::vector<pt_light> lights;
    std::vector<float> lights_rec, lights_cdf, lights_plight;
    float lights_select = 0.5f;
    bool lights_pickable = false;
    DeviceArray<float4> d_lights_rec;
    DeviceArray<float> d_lights_cdf;
    // area lights (pt_set_area_lights, pt_arealights.cpp; pinned in include/pt_api.h): the set as validated, and what the kernel samples in
    // table order (spheres first) -- per light a 12-float record (AreaLightsView, pt_internal.hpp), its index in the set, the float cdf and
    // P_light by the counting rule.  area_pickable: some P_light > 0; only then do the NEE launches take the area-light instances of k_nee,
    // and do the other paths refuse.  Device copies made by pt_set_area_lights
    std::vector<pt_area_light> area_lights;
    std::vector<float> area_rec, area_cdf, area_plight;
    std::vector<int32_t> area_order;
    int32_t area_spheres = 0;
    float area_select = 0.5f;
    bool area_pickable = false;
    DeviceArray<float4> d_area_rec;
    DeviceArray<float> d_area_cdf;
    // the homogeneous medium (pt_set_medium, pt_medium.cpp; pinned in include/pt_api.h): the record as validated (the defaults when none is
    // set).  Only while sigma_t > 0 do pt_render_nee and the NEE path of pt_render_adaptive_ex launch the medium instances of k_nee, and do
    // the other paths refuse.  Not part of the scene: uploads keep it
    pt_medium medium = {0.0f, {1.0f, 1.0f, 1.0f}, 0.0f, {-std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()},
                        {std::numeric_limits<float>::infinity(), std::numeric_limits<float>::infinity(), std::numeric_limits<float>::infinity()}};
    bool medium_set = false;
    // the medium's density grid (pt_set_medium_density, pt_medium.cpp): float32 as validated, density[(k * ny + j) * nx + i]; live only while a
    // medium with sigma_t > 0 is held too (grid_on).  Like the medium it is not part of the scene.  The device copy is made when it is set
    std::vector<float> grid;
    int32_t grid_n[3] = {0, 0, 0};
    bool grid_set = false;
    DeviceArray<float> d_grid;
    // interiors of dielectrics (pt_set_material_interior, pt_interior.cpp): per material index the record and whether one is bound, kept like a
    // texture binding -- across uploads, on a host-only context too, not part of the scene.  interior_live counts the bindings; the device table
    // (two float4 per material on the device, bound only where its type is 2 or 6) is rebuilt by interior_prepare when a binding or the
    // materials changed
    std::vector<pt_interior> interiors;
    std::vector<uint8_t> interior_bound;
    int32_t interior_live = 0;
    bool interior_dirty = true;
    DeviceArray<float4> d_interior;
    int chunk_taper = -1;  // option chunk_taper: shortest pass of a launch whose last passes taper off (0: all passes chunk_spp long; -1 default)
    int chunk_spp = -1;   // persistent megakernel work items: > 0 (pass, tile) items of that many samples, 0 whole
                          // tiles, -1 automatic (4 when the context has clearly more tiles than resident waves)
    int sah_visit_cost = 10;   // tenths of a triangle test (option sah_visit_cost)
    int flat_list = 16;        // at most this many big triangles go to the flat list (option flat_list; 0: none)
    int schedule = -1;     // megakernel: 0 lockstep per sample, 1 restart + tail suspension, -1 by the number of tiles per resident wave
    int suspend_lanes = -1; // tail suspension threshold of schedule 1 (-1: 24)
    int migrate_lanes = -1;                         // option migrate_lanes (kSchedMigrate; -1: 1)
    int node_min_lanes = -1, leaf_min_lanes = -1;   // phase switching of the while-while rounds (-1: by node path, fill_params)
    int lbvh_ploc = 16;     // device-built trees: PLOC search radius (8 / 16 / 32); 0: Karras' radix tree over the Morton codes
    int lbvh_cluster = 64;  // device-built trees: the top above clusters of this many triangles is rebuilt with the host SAH (0: not)
    int build_threads = 0; // host SAH builder: threads (0: the machine's, at most 16); the tree is the same for any number
    int wide_nodes = 1;    // 4-wide quantised nodes: 0 never, 1 for trees that do not fit LDS, 2 for every tree (tests)
    int wide_lds_entries = kWideLdsEntries;   // 4-wide traversal: stack entries per lane kept in LDS (tests lower it to force the global part)
    int lds_block = -1;      // whole tree in LDS: threads per workgroup of k_render: -1 768 where two such workgroups fit a CU, 512 (tests)
    int waves_per_simd = -1; // nodes from global memory: register budget for 4 / 5 / 6 / 7 waves per SIMD (-1: the most the LDS stacks allow)
    int debug_repeat = 0; // pt_debug_closest_hit: extra timed launches
    int cost_binning = 1; // wavefront: separate ray queues for rays that touch a complex object's box
    int bvh_policy = 0;   // 0/1 host SAH with SAH leaf termination, 2 leaves of <= 4, 3 leaves of <= 8, 4 device LBVH, 5 the SAH tree built on the device
    int sah_grain = 256;  // device SAH builder: ranges of at most this many triangles are finished by one wave each
    int wide_on_device = 1;  // device-built trees: the 4-wide collapse runs on the device too (0: on the host)
    int bvh_device = -1;     // SAH policies 0..3: build on the device (the same tree)?  -1: scenes of >= kDeviceBuildFrom triangles, 0 never, 1 always

    // ---- statistics
    std::vector<EventPair> events;
    size_t events_used = 0;
    double kernel_ms_acc = 0.0;
    int64_t kernel_launches = 0;
    size_t last_lds_bytes = 0;
    int last_waves_per_simd = 4;
    int nee_family = -1, nee_form = -1, nee_block = -1;      // what the last NEE launch took (launch_nee_noted); -1: none yet

    std::string err;
    char info[256] = {0};
};

namespace ptamd {

constexpr size_t kLdsPerCu = 160 * 1024;
// next to the stacks and the staged nodes: the big-triangle list (96 B each) and, in wf_intersect, one class byte per ray
// of a trip (16 waves x 256) + the compaction counters
constexpr size_t kLdsSlack = 32 * 100 + 4096 + 1024 + 256;

int fail(pt_context* ctx, int code, const std::string& msg);      // pt_host.cpp: records the text behind pt_last_error
int light_table_ready(pt_context* ctx);                            // pt_host.cpp: builds the light table of the uploaded scene if it is stale
float env_select(const pt_context* ctx, bool no_lights);           // pt_env.cpp: the effective P_env
// pt_host.cpp: the light table on the device and the environment's view (*sky: a map with a distribution is set) for a launch_nee
int nee_prepare(pt_context* ctx, int32_t strategy, NeeTable* lt, EnvView* env, bool* sky);
// pt_lights.cpp: the effective P_ana (no_other: the light table is empty and no environment with a distribution is set)
float lights_select(const pt_context* ctx, bool no_other);
// a light set with a pickable light is held: only pt_render_nee (LIGHT, MIS) and the NEE path of pt_render_adaptive_ex render; the text the
// other paths refuse with
inline bool lights_on(const pt_context* ctx) { return ctx->lights_pickable; }
inline std::string lights_refusal(const std::string& who) {
    return who + ": a light set is held and only pt_render_nee with PT_NEE_LIGHT or PT_NEE_MIS samples analytic lights (pt_clear_lights removes it)";
}
// pt_arealights.cpp: an area set with a pickable light is held: only pt_render_nee (every strategy) and the NEE path of pt_render_adaptive_ex
// render; the effective P_area (no_other: nothing else is pickable); the view of the device copies; the text the other paths refuse with
inline bool area_on(const pt_context* ctx) { return ctx->area_pickable; }
float area_select(const pt_context* ctx, bool no_other);
AreaLightsView area_view(const pt_context* ctx, bool no_other);
inline std::string area_refusal(const std::string& who) {
    return who + ": an area-light set is held and only pt_render_nee renders sphere lights and suns (pt_clear_area_lights removes it)";
}
// pt_medium.cpp: a medium with sigma_t > 0 is held: only pt_render_nee (every strategy) and the NEE path of pt_render_adaptive_ex render; the
// view the kernels read; the text the other paths refuse with
inline bool medium_on(const pt_context* ctx) { return ctx->medium_set && ctx->medium.sigma_t > 0.0f; }
MediumView medium_view(const pt_context* ctx);
// a density grid is live: the NEE launches take kNeeGrid; the view the kernels read (the box must be finite: grid_unbounded names the bound that
// is not, or is empty)
inline bool grid_on(const pt_context* ctx) { return medium_on(ctx) && ctx->grid_set; }
GridView grid_view(const pt_context* ctx);
std::string grid_unbounded(const pt_context* ctx);
// an interior binding is live (even an all-zero one): the NEE launches take kNeeInterior; the table the kernels read, made on the device when stale;
// the text the other paths refuse with
inline bool interior_on(const pt_context* ctx) { return ctx->interior_live > 0; }
int interior_prepare(pt_context* ctx, InteriorView* iv);
inline std::string interior_refusal(const std::string& who) {
    return who + ": a material holds an interior and only pt_render_nee renders it (pt_clear_material_interiors removes every binding)";
}
// the light hierarchy (pt_lighttree.cpp): built for the current light table (light_tree_ready, which makes the table first; host only), then
// the view of its device copies, made when stale (light_tree_prepare); light_tree_host is the same view over the host arrays
int light_tree_ready(pt_context* ctx);
int light_tree_prepare(pt_context* ctx, LightTreeView* v);
LightTreeView light_tree_host(const pt_context* ctx);
inline std::string medium_refusal(const std::string& who) {
    return who + ": a medium with sigma_t > 0 is held and only pt_render_nee renders it (pt_clear_medium removes it)";
}
// a lens with aperture > 0 is set: only pt_render_nee and the NEE path of pt_render_adaptive_ex render
inline bool lens_on(const pt_context* ctx) { return ctx->lens_set && ctx->lens_aperture > 0.0f; }
// pt_smooth.cpp: the packed vertex normals on the device for a smooth launch (repacked if stale); *vn = null when the option is off, unless force
int smooth_prepare(pt_context* ctx, const float4** vn, bool force = false);
// pt_texture.cpp: the textures, bindings and packed uvs on the device for a textured launch (refreshed if stale); tv->uv = null when the
// option is off, unless force
int texture_prepare(pt_context* ctx, TexView* tv, bool force = false);
// pt_host.cpp: the NEE launch the context's options, materials and lens ask for (NeeLaunch, pt_internal.hpp), with the vertex normals and
// textures prepared on the device; nee_on = false (no NEE launch will follow): nothing is prepared.  env and tiled are left clear: the caller sets them
int nee_launch_for(pt_context* ctx, const pt_camera* cam, bool nee_on, NeeLaunch* nl);
// pt_host.cpp: launch_nee on the context's stream; what the launch took -- the family, the form (bit 0 an environment is drawn, bit 1
// tiled) and the workgroup size the launcher chose -- is kept for pt_get_stat ("nee_family", "nee_form", "nee_block")
hipError_t launch_nee_noted(pt_context* ctx, const RenderParams& p, const NeeTable& lt, const NeeLaunch& nl);
int host_threads(const pt_context* ctx);                        // threads of the host-side scene path (option build_threads)
int read_back(pt_context* ctx, void* dst, const void* src, size_t bytes);      // pt_host.cpp: sync_and_check, then device -> host
// pt_post.cpp: what the rest of the library tells the post-process chain.  The scene was uploaded (guides, the despeckled frame and the
// remembered exposure are stale); an input of shaded guides changed (vertex normals, uvs, textures, bindings: shaded guides are stale);
// the area set changed (lit guides are stale)
void post_scene_uploaded(pt_context* ctx);
void post_shading_inputs_changed(pt_context* ctx);
void post_area_lights_changed(pt_context* ctx);

#define PT_HIP(ctx, call)                                                                   \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(ctx, PT_EHIP, std::string(#call) + ": " + hipGetErrorString(e_));   \
    } while (0)
// a DeviceArray allocation (reserve / replace) that must succeed
#define PT_ALLOC(ctx, call)                                                                 \
    do {                                                                                    \
        if (!(call))                                                                        \
            return fail(ctx, PT_EHIP, std::string(#call) + ": " + hipGetErrorString(HipAlloc::last)); \
    } while (0)

// a render launch of samples [first_sample, ...) through cam was enqueued: a frame starts at sample 0, and stays valid for pt_read_variance
// while every launch of it has folded the second moment (option "moments"), and for pt_temporal_accumulate while every launch of it used
// the camera it started with
inline void note_frame(pt_context* ctx, int32_t first_sample, const pt_camera* cam) {
    ctx->moments_valid = (first_sample == 0 || ctx->moments_valid) && ctx->moments != 0;
    if (first_sample == 0) {
        ++ctx->frame_serial;
        ctx->frame_cam = *cam;
        ctx->frame_cam_same = true;
    } else if (std::memcmp(cam, &ctx->frame_cam, sizeof(pt_camera)) != 0) {
        ctx->frame_cam_same = false;
    }
}

#define PT_NEED_DEVICE(ctx)                                                                 \
    do {                                                                                    \
        if (!(ctx)) return PT_EINVAL;                                                       \
        if (!(ctx)->has_device)                                                             \
            return fail(ctx, PT_ENODEVICE, "context was created without a HIP device (host-only); no CPU render path exists"); \
    } while (0)
// A small persistent pool for the host-side scene path: the threaded builders issue hundreds of short parallel regions
// (a 1M-triangle SAH build: ~150 at the top of the tree), and spawning 15 threads for each cost more than the regions did.
// One region at a time; a second caller (another context on another host thread) simply runs its region on fresh threads.
class HostPool {
public:
    static HostPool& get() { static HostPool p; return p; }
    // fn(k) for k in [0, chunks), on up to `threads` threads including the caller
    template <class F>
    void run(size_t chunks, int threads, F fn) {
        if (chunks == 0) return;
        if (threads <= 1 || chunks == 1) { for (size_t k = 0; k < chunks; ++k) fn(k); return; }
        std::unique_lock<std::mutex> region(region_mu_, std::try_to_lock);
        if (!region.owns_lock()) {                       // pool busy: plain threads
            std::atomic<size_t> next(0);
            auto work = [&]() { for (size_t k = next.fetch_add(1); k < chunks; k = next.fetch_add(1)) fn(k); };
            std::vector<std::thread> th;
            for (int t = 1; t < std::min<int>(threads, (int)chunks); ++t) th.emplace_back(work);
            work();
            for (std::thread& t : th) t.join();
            return;
        }
        grow(std::min<int>(threads, (int)chunks) - 1);
        std::function<void(size_t)> f = fn;
        {
            std::lock_guard<std::mutex> lk(mu_);
            job_ = &f;
            chunks_ = chunks;
            next_.store(0);
            helpers_wanted_ = std::min<int>(threads, (int)chunks) - 1;
            helpers_in_ = 0;
            helpers_done_ = 0;
            ++generation_;
        }
        cv_.notify_all();
        for (size_t k = next_.fetch_add(1); k < chunks; k = next_.fetch_add(1)) fn(k);
        std::unique_lock<std::mutex> lk(mu_);
        job_ = nullptr;                                  // no helper may start on this job any more
        done_cv_.wait(lk, [&]() { return helpers_done_ == helpers_in_; });
    }
    ~HostPool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (std::thread& t : workers_) t.join();
    }

private:
    void grow(int n) {
        while ((int)workers_.size() < n) workers_.emplace_back([this]() { loop(); });
    }
    void loop() {
        unsigned long long seen = 0;
        for (;;) {
            std::function<void(size_t)>* job = nullptr;
            size_t chunks = 0;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&]() { return stop_ || (generation_ != seen && job_ != nullptr && helpers_in_ < helpers_wanted_); });
                if (stop_) return;
                seen = generation_;
                job = job_;
                chunks = chunks_;
                ++helpers_in_;
            }
            for (size_t k = next_.fetch_add(1); k < chunks; k = next_.fetch_add(1)) (*job)(k);
            {
                std::lock_guard<std::mutex> lk(mu_);
                ++helpers_done_;
            }
            done_cv_.notify_all();
        }
    }
    std::mutex region_mu_, mu_;
    std::condition_variable cv_, done_cv_;
    std::vector<std::thread> workers_;
    std::function<void(size_t)>* job_ = nullptr;
    size_t chunks_ = 0;
    std::atomic<size_t> next_{0};
    int helpers_wanted_ = 0, helpers_in_ = 0, helpers_done_ = 0;
    unsigned long long generation_ = 0;
    bool stop_ = false;
};

// fn(begin, end) over [0, n) on up to `threads` threads (element-wise work: any split gives the same result)
template <class F>
void parallel_for(size_t n, size_t grain, int threads, F fn) {
    const size_t nt = std::min<size_t>((size_t)std::max(threads, 1), (n + grain - 1) / std::max<size_t>(grain, 1));
    if (nt <= 1) { fn((size_t)0, n); return; }
    const size_t per = (n + nt - 1) / nt;
    HostPool::get().run(nt, (int)nt, [&](size_t k) {
        const size_t b = k * per, e = std::min(n, b + per);
        if (b < e) fn(b, e);
    });
}
// ---- pt_builder.cpp
int deepest_interior_node(const std::vector<Node64>& nodes);
int reindex_treelet(std::vector<Node64>& nodes, int interior_depth, int want);
void plan_flat_pairs(pt_context* ctx);
void flat_test_packet(const pt_context* ctx, int k, float out[12]);

// ---- pt_launch.cpp
int32_t count_local_rows(int32_t H, int32_t rank, int32_t world, int32_t rb);
int wide_stack_entries(int pending);
int stack_entries_for(int interior_depth);
bool whole_tree_fits_lds(size_t n_nodes, size_t n_tris, int interior_depth, int n_flat);
int plan_node_placement(pt_context* ctx, const float4* d_bvh2 = nullptr, bool* wide_on_device = nullptr);
int alloc_stack_overflow(pt_context* ctx);
int seed_upload(pt_context* ctx, const int32_t* global_seeds);
void fill_params(const pt_context* ctx, const pt_camera* cam, RenderParams* p);
int ensure_shade_records(pt_context* ctx, RenderParams* p);
int check_ready(pt_context* ctx, const pt_camera* cam);
int time_begin(pt_context* ctx, EventPair** ep);
int time_end(pt_context* ctx, EventPair* ep);
int time_collect(pt_context* ctx);
int sync_and_check(pt_context* ctx);
inline int32_t local_tiles(const pt_context* c) { return ((c->W + 7) / 8) * ((c->local_rows + 7) / 8); }
#pragma GCC visibility push(hidden)
// `bytes` of src in a fresh allocation of *buf (what it held is freed first)
template <class T>
int upload_vec(pt_context* ctx, DeviceArray<T>* buf, const void* src, size_t bytes) {
    PT_ALLOC(ctx, buf->replace((std::max<size_t>(bytes, 64) + sizeof(T) - 1) / sizeof(T)));
    // an (almost) empty array still has one readable, all-zero record: a zero packet can never be
    // hit, so a leaf reference into an empty scene (the wrapped root's ~0) stays harmless
    if (bytes < 64) PT_HIP(ctx, hipMemset(buf->get(), 0, 64));
    if (bytes) PT_HIP(ctx, hipMemcpy(buf->get(), src, bytes, hipMemcpyHostToDevice));
    return PT_OK;
}
// The round trip of a debug entry point: in_bytes of `in` to the device, launch(d_in, d_out) on the context's stream, out_bytes back
template <class F>
int debug_round_trip(pt_context* ctx, const void* in, size_t in_bytes, void* out, size_t out_bytes, F launch) {
    PT_HIP(ctx, hipSetDevice(ctx->device));
    DeviceBuf d_in, d_out;
    PT_HIP(ctx, d_in.alloc(in_bytes));
    PT_HIP(ctx, d_out.alloc(out_bytes));
    PT_HIP(ctx, hipMemcpy(d_in.p, in, in_bytes, hipMemcpyHostToDevice));
    PT_HIP(ctx, launch(d_in.p, d_out.p));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP(ctx, hipMemcpy(out, d_out.p, out_bytes, hipMemcpyDeviceToHost));
    return PT_OK;
}
#pragma GCC visibility pop

// kNodesWide: room for the stack entries past the LDS part, for every lane of the largest grid a traversal kernel of
// this context is launched with (256-thread workgroups: persistent <= 6 per CU, wf_intersect 2 x 8 per CU, the debug
// kernel 8 per CU, a non-persistent render one wave per tile)

}  // namespace ptamd
