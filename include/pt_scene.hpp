// pt_scene.hpp -- header-only C++ mirror of the reference's host interface over the C ABI
// (pt_api.h).  Same class names, method names, argument meaning and call order as
// /root/reference/main.cpp:92-182 (Material, Triangle), 306-348 (Camera) and 363-742 (Scene), so
// that the reference's onInitialization()/onIdle() bodies (main.cpp:749-1016, 1226) compile
// against it with `using namespace ptamd_dropin;` once cl_float3 is spelled pt_float3.
//
// Differences forced by leaving OpenCL/GLUT behind:
//   * the globals the reference's Camera() and trace_rays() read (screen_width/height,
//     iterations, current_sample, global_fov/yaw/pitch/shift and the per-frame movement
//     global_forward/rightward/upward: main.cpp:20-39) are members of Scene (`globals`);
//     Camera(Globals&) has the reference constructor's side effect -- it adds the movement into
//     global_shift along the rotated axes (main.cpp:334-336) -- so the key handlers of
//     main.cpp:1189-1224 move the camera exactly as they do there; init_Scene takes the frame size;
//   * failures throw std::runtime_error instead of exit(1) (main.cpp:502, 560);
//   * the radiance is read back with download_colors() instead of being blitted from a GL
//     texture (main.cpp:519, 1019-1039).
#pragma once

#include <stdexcept>
#include <string>
#include <vector>

#include "pt_api.h"

namespace ptamd_dropin {

typedef pt_float3 cl_float3;   // 16 bytes, like CL/cl_platform.h

struct Material : pt_material {                        // main.cpp:92-112
    Material() { type = -1; }
    Material(cl_float3 kd, cl_float3 ks, cl_float3 emission, cl_float3 N, cl_float3 K, float shininess, int type_) {
        pt_material_init(this, kd.s, ks.s, emission.s, N.s, K.s, shininess, type_);
    }
};

struct Triangle : pt_triangle {                        // main.cpp:139-182
    Triangle(cl_float3 r1_, cl_float3 r2_, cl_float3 r3_, unsigned short mati_) { pt_triangle_init(this, r1_.s, r2_.s, r3_.s, mati_); }
};

struct Globals {                                       // the shipped values of main.cpp:20-39
    int screen_width = 192 * 8, screen_height = 108 * 8;                                 // main.cpp:20-21
    int iterations = 1;                                                                  // main.cpp:27
    float global_fov = 75.0f;                                                            // main.cpp:30
    float global_yaw = (float)(-13.800002 - 50), global_pitch = (float)(5.599997 + 10);   // main.cpp:31-32 (double arithmetic, narrowed)
    float global_forward = 0, global_rightward = 0, global_upward = 0;                   // main.cpp:36-38: this frame's movement (speed * dt or 0, main.cpp:1189-1209)
    cl_float3 global_shift = {{265.055481f, 162.305969f, 360.414001f, 0.0f}};            // main.cpp:39
    // (the "canonical" view the reference keeps in comments, main.cpp:33-35,40: fov 60, yaw 0, pitch 0, shift 0)
};

struct Camera : pt_camera {                            // main.cpp:306-348
    Camera() { XM = YM = 0; }
    // the reference's Camera(): FIRST the movement accumulates into global_shift (main.cpp:334-336), then the eye is placed
    explicit Camera(Globals& g) {
        pt_camera_move(g.global_shift.s, g.global_yaw, g.global_pitch, g.global_forward, g.global_rightward, g.global_upward);
        pt_camera_init(this, g.global_fov, g.global_yaw, g.global_pitch, g.global_shift.s, g.screen_width, g.screen_height);
    }
    // a view of the globals as they stand (no movement applied)
    explicit Camera(const Globals& g) { pt_camera_init(this, g.global_fov, g.global_yaw, g.global_pitch, g.global_shift.s, g.screen_width, g.screen_height); }
};

class Scene {                                          // main.cpp:363-742
public:
    Globals globals;

    Scene() {}
    Scene(const Scene&) = delete;
    Scene& operator=(const Scene&) = delete;
    ~Scene() { if (ctx) pt_destroy(ctx); }

    std::string list_info() {                          // main.cpp:389-455
        char buf[256];
        ck(pt_device_info(ctx, buf, sizeof buf));
        return buf;
    }
    void init_Scene(int device = 0) {                  // main.cpp:456-528
        if (pt_create(device, globals.screen_width, globals.screen_height, &ctx) != PT_OK)
            throw std::runtime_error(std::string("init_Scene: ") + pt_last_error(nullptr));
    }
    void add_Triangle(const Triangle& tri) { ck(pt_add_triangle(ctx, &tri)); }                 // main.cpp:529
    int add_Material(const Material& mat) { return ck(pt_add_material(ctx, &mat)); }           // main.cpp:532
    void end_Obj() { ck(pt_end_obj(ctx)); }                                                    // main.cpp:536
    void add_Obj(const std::string& file, cl_float3 pos, cl_float3 scale, float pitch, float yaw) {   // main.cpp:552
        ck(pt_add_obj(ctx, file.c_str(), pos.s, scale.s, pitch, yaw));
    }
    void upload_Triangles() { ck(pt_upload_triangles(ctx)); }                                  // main.cpp:618
    void upload_Materials() { ck(pt_upload_materials(ctx)); }                                  // main.cpp:631
    void generate_rays() {                                                                     // main.cpp:635
        camera = Camera(globals);
        ck(pt_generate_rays(ctx, &camera));
    }
    void trace_rays() {                                                                        // main.cpp:645
        int32_t s = 0;
        ck(pt_get_current_sample(ctx, &s));
        ck(pt_trace_rays(ctx, &camera, globals.iterations, s));
    }
    void render() {                                                                            // main.cpp:683
        generate_rays();
        trace_rays();
        ck(pt_set_current_sample(ctx, current_sample() + 1));
    }
    // nsamples x render() as one persistent launch (same result, bit for bit, for a camera at rest; a moving camera -- a
    // non-zero global_forward / rightward / upward -- moves ONCE per call here, where n x render() would move it n times)
    void render(int nsamples) {
        camera = Camera(globals);
        ck(pt_render(ctx, &camera, globals.iterations, nsamples));
    }
    // one adaptive frame (pt_render_adaptive): min_spp to every tile, then doubling where the noise estimate is >= threshold
    void render_adaptive(int min_spp, int max_spp, float threshold) {
        camera = Camera(globals);
        ck(pt_render_adaptive(ctx, &camera, globals.iterations, min_spp, max_spp, threshold));
    }
    // the same with a choice of error measure and render path (pt_render_adaptive_ex; start from pt_adaptive_defaults)
    void render_adaptive(const pt_adaptive_params& params) {
        camera = Camera(globals);
        ck(pt_render_adaptive_ex(ctx, &camera, globals.iterations, &params));
    }
    // nsamples of render(n)'s estimator with next-event estimation (pt_render_nee; strategy PT_NEE_BSDF / _LIGHT / _MIS)
    void render_nee(int nsamples, int strategy = PT_NEE_MIS) {
        camera = Camera(globals);
        ck(pt_render_nee(ctx, &camera, globals.iterations, nsamples, strategy));
    }
    // a lat-long map lighting render_nee (pt_set_environment; rgb: w x h x 3 floats, row 0 at the +y pole; p = NULL: the defaults)
    void set_environment(const float* rgb, int w, int h, const pt_environment_params* p = nullptr) { ck(pt_set_environment(ctx, rgb, w, h, p)); }
    void clear_environment() { ck(pt_clear_environment(ctx)); }
    // point, spot and directional lights for render_nee (pt_set_lights replaces the whole set; p = NULL: the defaults).  While a pickable
    // light is held only render_nee with PT_NEE_LIGHT / PT_NEE_MIS and the NEE path of render_adaptive render
    void set_lights(const pt_light* lights, int32_t count, const pt_lights_params* p = nullptr) { ck(pt_set_lights(ctx, lights, count, p)); }
    void clear_lights() { ck(pt_clear_lights(ctx)); }
    // sphere lights and suns with an angular size for render_nee (pt_set_area_lights replaces the whole set; p = NULL: the defaults).  While a
    // non-black light is held only render_nee (every strategy) and the NEE path of render_adaptive render
    void set_area_lights(const pt_area_light* lights, int32_t count, const pt_area_lights_params* p = nullptr) { ck(pt_set_area_lights(ctx, lights, count, p)); }
    void clear_area_lights() { ck(pt_clear_area_lights(ctx)); }
    // a homogeneous medium (fog) for render_nee (pt_set_medium; start from pt_medium_defaults).  While one with sigma_t > 0 is held only
    // render_nee and the NEE path of render_adaptive render; uploads keep it
    void set_medium(const pt_medium& m) { ck(pt_set_medium(ctx, &m)); }
    void clear_medium() { ck(pt_clear_medium(ctx)); }
    // a voxel density for that medium (pt_set_medium_density): density[(k * ny + j) * nx + i] over nx x ny x nz equal cells of its box, which
    // must be finite to render; the extinction is sigma_t x density.  medium_density reads it back (returns whether one is held)
    void set_medium_density(const float* density, int32_t nx, int32_t ny, int32_t nz) { ck(pt_set_medium_density(ctx, density, nx, ny, nz)); }
    void clear_medium_density() { ck(pt_clear_medium_density(ctx)); }
    bool medium_density(float* out, int64_t cap, int32_t dims[3]) { return ck(pt_debug_medium_density(ctx, out, cap, dims)) == 1; }
    void debug_grid(const float* in, int64_t n, float* out) { ck(pt_debug_grid(ctx, in, n, out)); }
    // the medium inside a type-2 or type-6 material (pt_set_material_interior): chromatic absorption, grey scattering, a Henyey-Greenstein g; live
    // as soon as it is bound, kept across uploads like a texture binding.  material_interior reads it back (returns whether one is held)
    void set_material_interior(int32_t material, const pt_interior& in) { ck(pt_set_material_interior(ctx, material, &in)); }
    void clear_material_interiors() { ck(pt_clear_material_interiors(ctx)); }
    bool material_interior(int32_t material, pt_interior* out) { return ck(pt_get_material_interior(ctx, material, out)) == 1; }
    void debug_interior(const float* in, int64_t n, float* out) { ck(pt_debug_interior(ctx, in, n, out)); }
    // the light hierarchy of render_nee (set_option("light_tree", 1); pt_debug_light_tree, pt_debug_light_tree_eval): the nodes (8 floats each) and
    // the tree-order lights read back, and both walks evaluated per item by the host code or, on_device, by k_debug_light_tree
    void debug_light_tree(float* nodes, int64_t node_cap, int64_t* n_nodes, int32_t* orig_tri, int64_t light_cap, int64_t* n_lights) {
        ck(pt_debug_light_tree(ctx, nodes, node_cap, n_nodes, orig_tri, light_cap, n_lights));
    }
    void debug_light_tree_eval(const float* points, const float* normals, const float* u0, const int32_t* tris, int64_t n, pt_light_tree_eval* out,
                               bool on_device = false) {
        ck(pt_debug_light_tree_eval(ctx, points, normals, u0, tris, n, out, on_device ? 1 : 0));
    }
    // vertex normals for smooth shading (set_option("smooth_normals", 1); render_nee only): normals = count x 9 floats, n1 n2 n3 per
    // triangle in add order starting at first_triangle; compute_vertex_normals derives them per object (obj = -1: every object)
    void set_vertex_normals(const float* normals, int64_t count, int64_t first_triangle = 0) { ck(pt_set_vertex_normals(ctx, first_triangle, count, normals)); }
    void clear_vertex_normals() { ck(pt_clear_vertex_normals(ctx)); }
    void compute_vertex_normals(float crease_degrees, int32_t obj = -1) { ck(pt_compute_vertex_normals(ctx, obj, crease_degrees)); }
    // albedo textures (set_option("textures", 1); render_nee only): rgb = w x h x 3 floats, row 0 at the top (p = NULL: bilinear, linear);
    // a texture is bound to a type-0 material (texture = -1: none); uvs = count x 6 floats, u1 v1 u2 v2 u3 v3 per triangle in add order
    int add_texture(const float* rgb, int w, int h, const pt_texture_params* p = nullptr) { return ck(pt_add_texture(ctx, rgb, w, h, p)); }
    void clear_textures() { ck(pt_clear_textures(ctx)); }
    void set_material_texture(int32_t material, int32_t texture) { ck(pt_set_material_texture(ctx, material, texture)); }
    void set_vertex_uvs(const float* uvs, int64_t count, int64_t first_triangle = 0) { ck(pt_set_vertex_uvs(ctx, first_triangle, count, uvs)); }
    void clear_vertex_uvs() { ck(pt_clear_vertex_uvs(ctx)); }
    void debug_vertex_uvs(float* uvs, int32_t* has) { ck(pt_debug_vertex_uvs(ctx, uvs, has)); }
    void debug_texture(int32_t texture, float* rgb, int64_t cap, int32_t* w, int32_t* h, int32_t* filter) { ck(pt_debug_texture(ctx, texture, rgb, cap, w, h, filter)); }
    void debug_albedo(const pt_ray* rays, int64_t n, int32_t* out_tri, float* out_rgbt) { ck(pt_debug_albedo(ctx, rays, n, out_tri, out_rgbt)); }
    // the rough metal of material type 4 (set_option("glossy", 1); render_nee only): the device functions of the vertex, 9 floats in
    // (N, D, alpha, rnd1, rnd2) and 8 out per item (pt_debug_glossy)
    void debug_glossy(int64_t n, const float* N_D_alpha_rnd, float* out) { ck(pt_debug_glossy(ctx, n, N_D_alpha_rnd, out)); }
    // the coated diffuse of material type 5 (set_option("coated", 1); render_nee only): the device functions of the vertex, 12 floats in
    // (N, D, alpha, F0, kd, rnd1, rnd2, u_sel) and 10 out per item (pt_debug_coated)
    void debug_coated(int64_t n, const float* in, float* out) { ck(pt_debug_coated(ctx, n, in, out)); }
    // the rough dielectric of material type 6 (set_option("frosted", 1); render_nee only): the device functions of the vertex, 12 floats in
    // (N, D, alpha, F0, eta, rnd1, rnd2, u_sel) and 10 out per item (pt_debug_frosted)
    void debug_frosted(int64_t n, const float* in, float* out) { ck(pt_debug_frosted(ctx, n, in, out)); }
    // a thin lens for render_nee and the NEE path of render_adaptive (pt_set_lens; aperture = the lens radius, 0: the pinhole; focus_distance
    // along the optical axis).  While aperture > 0 only they render; the guides keep the pinhole view.  focus_at: the axial distance of the
    // first hit under pixel (x, y) of the last render's view, +inf on a miss; debug_lens: the device's lens ray of n items {gid, S}, 6 floats each
    void set_lens(float aperture, float focus_distance) {
        const pt_lens_params p = {aperture, focus_distance, {0.0f, 0.0f}};
        ck(pt_set_lens(ctx, &p));
    }
    void clear_lens() { ck(pt_clear_lens(ctx)); }
    float focus_at(int32_t x, int32_t y) {
        float d = 0.0f;
        ck(pt_focus_at(ctx, &camera, x, y, &d));
        return d;
    }
    void debug_lens(float aperture, float focus_distance, int64_t n, const int32_t* gid_state, float* out) {
        const pt_lens_params p = {aperture, focus_distance, {0.0f, 0.0f}};
        ck(pt_debug_lens(ctx, &camera, &p, n, gid_state, out));
    }
    // the spec math and sampling primitives of the kernels on n items of 32-bit words (pt_debug_spec; fn = PT_SPEC_*)
    void debug_spec(int32_t fn, int64_t n, const uint32_t* in, uint32_t* out) { ck(pt_debug_spec(ctx, fn, n, in, out)); }
    // one iteration body of the path (shade_hit) on n items of 32-bit words (pt_debug_shade; instance = PT_SHADE_* bits)
    void debug_shade(const pt_camera& cam, int32_t iterations, int32_t instance, int64_t n, const uint32_t* in, uint32_t* out) {
        ck(pt_debug_shade(ctx, &cam, iterations, instance, n, in, out));
    }
    // guide buffers of the current view (pt_render_aovs) and the a-trous filter over them (pt_denoise; p = NULL: the defaults)
    // (the view of the last render: a new Camera(globals) would move a moving camera once more)
    void render_aovs(int subpixels = 1, int specular_depth = 4) {
        ck(pt_render_aovs(ctx, &camera, subpixels, specular_depth));
    }
    // the same through pt_render_aovs_ex: p.shading = PT_AOV_SHADED writes the shading normal and the textured albedo of the NEE path
    void render_aovs(const pt_camera& cam, const pt_aov_params& p) { ck(pt_render_aovs_ex(ctx, &cam, &p)); }
    void denoise(const pt_denoise_params* p = nullptr) {
        pt_denoise_params d;
        pt_denoise_defaults(&d);
        ck(pt_denoise(ctx, p ? p : &d));
    }
    // per local pixel, the variance of its mean luminance (pt_read_variance: the frame was rendered with option "moments" = 1)
    std::vector<float> read_variance() {
        int64_t n = 0;
        ck(pt_local_pixel_count(ctx, &n));
        std::vector<float> out((size_t)n);
        ck(pt_read_variance(ctx, out.data(), n));
        return out;
    }
    void* device_variance() {                  // throws with pt_last_error's text (host-only context, or moments not valid)
        void* d = pt_device_variance(ctx);
        if (!d) ck(PT_EINVAL);
        return d;
    }
    // the variance-guided filter (pt_denoise_variance; p = NULL: the defaults); result: pt_read_denoised like denoise()
    void denoise_variance(const pt_denoise_variance_params* p = nullptr) {
        pt_denoise_variance_params d;
        pt_denoise_variance_defaults(&d);
        ck(pt_denoise_variance(ctx, p ? p : &d));
    }
    void set_option(const char* key, int64_t value) { ck(pt_set_option(ctx, key, value)); }   // pt_set_option, e.g. ("moments", 1), ("aov_lights", 1)
    // temporal accumulation with reprojection (pt_temporal_accumulate; p = NULL: the defaults): after a frame rendered with option
    // "moments" = 1 and render_aovs() of its camera
    void temporal_accumulate(const pt_temporal_params* p = nullptr) {
        pt_temporal_params d;
        pt_temporal_defaults(&d);
        ck(pt_temporal_accumulate(ctx, p ? p : &d));
    }
    // the last accumulate's {r, g, b, variance of the mean} per local pixel (rgbv: 4 floats each) and the samples behind it
    void read_temporal(std::vector<float>& rgbv, std::vector<float>& n) {
        int64_t np = 0;
        ck(pt_local_pixel_count(ctx, &np));
        rgbv.resize((size_t)np * 4);
        n.resize((size_t)np);
        ck(pt_read_temporal(ctx, rgbv.data(), n.data(), np));
    }
    void* device_temporal() { return pt_device_temporal(ctx); }   // {r, g, b, m2} per local pixel; NULL before an accumulate
    // the variance-guided filter on the accumulated colour and variance (pt_denoise_temporal); result: pt_read_denoised like denoise()
    void denoise_temporal(const pt_denoise_variance_params* p = nullptr) {
        pt_denoise_variance_params d;
        pt_denoise_variance_defaults(&d);
        ck(pt_denoise_temporal(ctx, p ? p : &d));
    }
    // the variance-gated firefly filter (pt_despeckle; p = NULL: the defaults) on the frame, or with p->source = PT_DESPECKLE_TEMPORAL on
    // the last accumulate; the result: pt_read_despeckled / pt_device_despeckled
    void despeckle(const pt_despeckle_params* p = nullptr) {
        pt_despeckle_params d;
        pt_despeckle_defaults(&d);
        ck(pt_despeckle(ctx, p ? p : &d));
    }
    // the variance-guided filter on the despeckled colour and variance (pt_denoise_despeckled); result: pt_read_denoised like denoise()
    void denoise_despeckled(const pt_denoise_variance_params* p = nullptr) {
        pt_denoise_variance_params d;
        pt_denoise_variance_defaults(&d);
        ck(pt_denoise_despeckled(ctx, p ? p : &d));
    }
    // the display stage (pt_display; p = NULL: the defaults): exposure, bloom, tone curve and encoding of p->source on the device, no
    // read-back; the result: pt_read_display / pt_device_display / pt_write_display_ppm, the metered numbers: display_info()
    void display(const pt_display_params* p = nullptr) {
        pt_display_params d;
        pt_display_defaults(&d);
        ck(pt_display(ctx, p ? p : &d));
    }
    struct pt_display_info display_info() { struct pt_display_info i = {}; ck(::pt_display_info(ctx, &i)); return i; }
    void display_reset() { ck(pt_display_reset(ctx)); }
    void write_display_ppm(const std::string& path) { ck(pt_write_display_ppm(ctx, path.c_str())); }
    int current_sample() { int32_t s = 0; ck(pt_get_current_sample(ctx, &s)); return s; }
    void reset_samples() { ck(pt_set_current_sample(ctx, 0)); }                                // main.cpp:1046
    void finish() { ck(pt_sync(ctx)); }                                                        // queue.finish(), main.cpp:675
    std::vector<cl_float3> download_colors() {                                                 // (commented out in the reference: main.cpp:727)
        int64_t n = 0;
        ck(pt_local_pixel_count(ctx, &n));
        std::vector<cl_float3> out((size_t)n);
        ck(pt_read_colors(ctx, &out[0].s[0], n));
        return out;
    }
    // what the reference shows through its GL blit (main.cpp:1019-1039), as files
    void write_ppm(const std::string& path, int which = 0) { ck(pt_write_ppm(ctx, path.c_str(), which)); }
    void write_pfm(const std::string& path) { ck(pt_write_pfm(ctx, path.c_str())); }
    // multi-GPU hosts: init_Scene_tiled instead of init_Scene, then comm_init with the
    // 128-byte id rank 0 obtained from Scene::comm_unique_id(), render as usual, gather_frame() + download_frame()
    void init_Scene_tiled(int device, int rank, int world, int rows_per_block = 8) {
        if (pt_create_tiled(device, globals.screen_width, globals.screen_height, rank, world, rows_per_block, &ctx) != PT_OK)
            throw std::runtime_error(std::string("init_Scene_tiled: ") + pt_last_error(nullptr));
    }
    static std::vector<unsigned char> comm_unique_id() {
        std::vector<unsigned char> id(PT_COMM_ID_BYTES);
        if (pt_comm_unique_id(id.data()) != PT_OK) throw std::runtime_error(std::string("comm_unique_id: ") + pt_last_error(nullptr));
        return id;
    }
    void comm_init(const std::vector<unsigned char>& id) { ck(pt_comm_init(ctx, id.data())); }
    void gather_frame() { ck(pt_gather_frame(ctx)); }
    std::vector<cl_float3> download_frame() {
        int64_t n = 0;
        ck(pt_frame_size(ctx, nullptr, nullptr, &n));
        std::vector<cl_float3> out((size_t)n);
        ck(pt_read_frame(ctx, &out[0].s[0], n));
        return out;
    }
    pt_context* handle() { return ctx; }

private:
    int ck(int rc) {
        if (rc < 0) throw std::runtime_error(std::string("libptamd: ") + pt_last_error(ctx));
        return rc;
    }
    pt_context* ctx = nullptr;
    Camera camera;
};

}  // namespace ptamd_dropin
