// pt_host.cpp -- host side of libptamd.so: the C ABI of include/pt_api.h (context, authoring, read-back, options, statistics).
//
// What lives here (all of it host work the reference also does on the host):
//   * value-type constructors            main.cpp:101-111, 144-166, 311-347
//   * context life cycle, Scene authoring (add_Material / add_Triangle), seeds, materials
//   * read-back, frame assembly entry points, options, statistics, debug getters
//   * the NEE launch path: the light table, the kernel family a launch takes (nee_launch_for), pt_render_nee
// Scene -> tree is pt_builder.cpp (pt_end_obj, pt_upload_triangles), tree -> launches pt_launch.cpp (pt_render ...), the post-process
// chain pt_post.cpp; each later feature has a host file of its own (the map is in pt_context.hpp, which is what they all share).
// There is no CPU render path in this library: every pt_render / pt_trace_rays / pt_generate_rays call launches HIP kernels or fails.
//
// Compiled with -ffp-contract=off: the reference's host arithmetic is plain x86-64 g++
// (no fused multiply-add), and the results of these constructors feed bit-exact parity tests.
#include <limits>

#include "pt_context.hpp"

namespace {
thread_local std::string g_create_error;
}  // namespace

namespace ptamd {

int fail(pt_context* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg; else g_create_error = msg;
    return code;
}

// threads of the host-side scene path (option build_threads; 0: the machine's, at most 16)
int host_threads(const pt_context* ctx) {
    const unsigned hw = std::thread::hardware_concurrency();
    return ctx->build_threads > 0 ? ctx->build_threads : (int)std::min(16u, std::max(1u, hw));
}

// `bytes` of a device array to the host, once the context's launches are through and their error word is clean
int read_back(pt_context* ctx, void* dst, const void* src, size_t bytes) {
    const int rc = sync_and_check(ctx);
    if (rc != PT_OK) return rc;
    if (bytes) PT_HIP(ctx, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return PT_OK;
}

int fail_ctx(pt_context* ctx, int code, const std::string& msg) { return fail(ctx, code, msg); }   // for pt_obj.cpp, pt_image.cpp
// pt_add_triangles without the copy, for pt_obj.cpp: n records are appended and returned for the caller to fill in place
// (every one of them, before anything else touches the context)
int append_triangles(pt_context* ctx, int64_t n, pt_triangle** tail) {
    if (!ctx || n < 0 || !tail) return PT_EINVAL;
    if ((int64_t)ctx->tris.size() + n > kMaxTriangles) return fail(ctx, PT_EINVAL, "more than 2^26 triangles");
    const size_t old = ctx->tris.size();
    ctx->tris.resize(old + (size_t)n);
    ctx->tris_uploaded = false;
    *tail = ctx->tris.data() + old;
    return PT_OK;
}
// pt_comm.hip
hipError_t launch_deinterleave(const float4* gathered, float4* frame, int W, int H, int world, int rb, long long slab_stride, hipStream_t stream);
void gather_source_index(int W, int H, int world, int rb, long long slab_stride, int64_t* out);
int comm_available(std::string* err);
int comm_unique_id(void* id128, std::string* err);
int comm_init(const void* id128, int rank, int world, void** comm_out, std::string* err);
void comm_destroy(void* comm);
int comm_all_gather(void* comm, const void* send, void* recv, size_t floats_per_rank, hipStream_t stream, std::string* err);

}  // namespace ptamd

extern "C" {

void pt_material_init(pt_material* m, const float kd[3], const float ks[3], const float emission[3],
                      const float N[3], const float K[3], float shininess, int32_t type) {
    std::memset(m, 0, sizeof *m);
    for (int i = 0; i < 3; ++i) { m->kd.s[i] = kd[i]; m->ks.s[i] = ks[i]; m->emission.s[i] = emission[i]; }
    m->shininess = shininess;
    m->type = type;
    m->n = (N[0] + N[1] + N[2]) / 3.0f;                       // main.cpp:103
    for (int i = 0; i < 3; ++i) {                              // main.cpp:105-109
        float a = (N[i] - 1) * (N[i] - 1);
        float b = (N[i] + 1) * (N[i] + 1);
        m->F0.s[i] = (K[i] * K[i] + a) / (K[i] * K[i] + b);
    }
}

float pt_material_roughness(float shininess) {
    if (!std::isfinite(shininess) || shininess < 0.0f) return 1.0f;
    return (float)std::min(1.0, std::max(0.03, std::sqrt(2.0 / ((double)shininess + 2.0))));
}

void pt_triangle_init(pt_triangle* t, const float r1[3], const float r2[3], const float r3[3], uint16_t mati) {
    std::memset(t, 0, sizeof *t);
    float v1[3], v2[3], n[3];
    for (int i = 0; i < 3; ++i) {
        t->r1.s[i] = r1[i]; t->r2.s[i] = r2[i]; t->r3.s[i] = r3[i];
        v1[i] = r2[i] - r1[i];
        v2[i] = r3[i] - r1[i];
    }
    t->mati = mati;
    n[0] = v1[1] * v2[2] - v1[2] * v2[1];
    n[1] = v1[2] * v2[0] - v1[0] * v2[2];
    n[2] = v1[0] * v2[1] - v1[1] * v2[0];
    // main.cpp:160: unqualified sqrt on a float -> the double routine, narrowed
    float length = (float)std::sqrt((double)(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]));
    for (int i = 0; i < 3; ++i) t->N.s[i] = n[i] / length;
}

void pt_triangles_init(pt_triangle* out, const float* verts, const uint16_t* mati, int64_t n) {
    for (int64_t i = 0; i < n; ++i) pt_triangle_init(&out[i], verts + 9 * i, verts + 9 * i + 3, verts + 9 * i + 6, mati[i]);
}

static void rotate_x_ref(float v[3], float gamma) {  // main.cpp:63-70 (trig in double)
    gamma = gamma / 180.0f * 3.141593f;
    const double c = std::cos((double)gamma), s = std::sin((double)gamma);
    const float r1 = (float)((double)v[1] * c - (double)v[2] * s);
    const float r2 = (float)((double)v[1] * s + (double)v[2] * c);
    v[1] = r1;
    v[2] = r2;
}
static void rotate_y_ref(float v[3], float beta) {  // main.cpp:55-62
    beta = beta / 180.0f * 3.141593f;
    const double c = std::cos((double)beta), s = std::sin((double)beta);
    const float r0 = (float)((double)v[0] * c + (double)v[2] * s);
    const float r2 = (float)(-(double)v[0] * s + (double)v[2] * c);
    v[0] = r0;
    v[2] = r2;
}

void pt_camera_init(pt_camera* c, float fov, float yaw, float pitch, const float shift[3], int32_t width, int32_t height) {
    std::memset(c, 0, sizeof *c);
    c->XM = (float)width;
    c->YM = (float)height;
    const float up_length = c->YM / 2.0f;
    const float right_length = c->XM / 2.0f;
    const float ahead_length = (float)((double)right_length / std::tan((double)(fov / 2.0f / 180.0f * 3.141593f)));
    float up[3] = {0.0f, 1.0f, 0.0f}, right[3] = {1.0f, 0.0f, 0.0f}, ahead[3] = {0.0f, 0.0f, 1.0f};
    rotate_x_ref(up, pitch); rotate_y_ref(up, yaw);
    rotate_x_ref(right, pitch); rotate_y_ref(right, yaw);
    rotate_x_ref(ahead, pitch); rotate_y_ref(ahead, yaw);
    for (int i = 0; i < 3; ++i) { up[i] *= up_length; right[i] *= right_length; ahead[i] *= ahead_length; }
    c->eye.s[0] = 500.0f + shift[0];
    c->eye.s[1] = 500.0f + shift[1];
    c->eye.s[2] = -1299.037842f + shift[2];
    for (int i = 0; i < 3; ++i) { c->up.s[i] = up[i]; c->right.s[i] = right[i]; c->lookat.s[i] = c->eye.s[i] + ahead[i]; }
}

// The side effect of the reference's Camera(): main.cpp:334-336 adds this frame's movement along the ROTATED unit axes into
// global_shift before the eye is placed (the key handlers of main.cpp:1189-1209 set global_forward / rightward / upward to
// speed * dt or 0).  Same rotations as pt_camera_init, float arithmetic in the reference's order, no fused operations.
void pt_camera_move(float shift[3], float yaw, float pitch, float forward, float rightward, float upward) {
    float up[3] = {0.0f, 1.0f, 0.0f}, right[3] = {1.0f, 0.0f, 0.0f}, ahead[3] = {0.0f, 0.0f, 1.0f};
    rotate_x_ref(up, pitch); rotate_y_ref(up, yaw);
    rotate_x_ref(right, pitch); rotate_y_ref(right, yaw);
    rotate_x_ref(ahead, pitch); rotate_y_ref(ahead, yaw);
    for (int i = 0; i < 3; ++i) {
        const float a = ahead[i] * forward, r = right[i] * rightward, u = up[i] * upward;
        shift[i] = ((shift[i] + a) + r) + u;
    }
}

int pt_create_tiled(int device, int32_t width, int32_t height, int32_t rank, int32_t world, int32_t rows_per_block, pt_context** out) {
    if (!out) return fail(nullptr, PT_EINVAL, "out is NULL");
    *out = nullptr;
    if (width <= 0 || height <= 0 || (int64_t)width * height > (int64_t)1 << 30) return fail(nullptr, PT_EINVAL, "bad frame size");
    if (width > 65535 || height > 65535) return fail(nullptr, PT_EINVAL, "bad frame size: at most 65,535 pixels per side (the kernels pack a pixel's coordinates into 2 x 16 bits)");
    if (world < 1 || rank < 0 || rank >= world || rows_per_block < 1) return fail(nullptr, PT_EINVAL, "bad rank/world/rows_per_block");
    pt_context* ctx = new pt_context();
    ctx->W = width;
    ctx->H = height;
    ctx->rank = rank;
    ctx->world = world;
    ctx->rows_per_block = rows_per_block;
    ctx->local_rows = count_local_rows(height, rank, world, rows_per_block);
    ctx->npix = (int64_t)ctx->local_rows * width;
    for (int32_t r = 0; r < world; ++r) ctx->slab_pix = std::max(ctx->slab_pix, (int64_t)count_local_rows(height, r, world, rows_per_block) * width);
    ctx->device = device;
    if (device < 0) {  // host-only context: authoring + BVH build + debug getters, nothing renders
        std::snprintf(ctx->info, sizeof ctx->info, "host-only context (no device)");
        *out = ctx;
        return PT_OK;
    }
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0 || device >= count) {
        delete ctx;
        return fail(nullptr, PT_ENODEVICE, std::string("no usable HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device index out of range"));
    }
    auto bail = [&](const char* what, hipError_t err) {
        std::string msg = std::string(what) + ": " + hipGetErrorString(err);
        pt_destroy(ctx);
        return fail(nullptr, PT_EHIP, msg);
    };
    if ((e = hipSetDevice(device)) != hipSuccess) return bail("hipSetDevice", e);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess) return bail("hipGetDeviceProperties", e);
    ctx->cu_count = prop.multiProcessorCount;
    std::snprintf(ctx->info, sizeof ctx->info, "%s (%s), %d CUs, %.1f GiB, wave %d", prop.name, prop.gcnArchName,
                  prop.multiProcessorCount, (double)prop.totalGlobalMem / (1024.0 * 1024.0 * 1024.0), prop.warpSize);
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        std::string msg = std::string("device is ") + prop.gcnArchName + ", this library carries gfx950 code only";
        pt_destroy(ctx);
        return fail(nullptr, PT_ENODEVICE, msg);
    }
    ctx->has_device = true;
    const size_t np = (size_t)std::max<int64_t>(ctx->npix, 1);
    const size_t nslab = (size_t)std::max<int64_t>(ctx->slab_pix, 1);      // colors is this rank's slab of the all-gather
    if (!ctx->d_rays.replace(np)) return bail("hipMalloc(rays)", HipAlloc::last);                                      // main.cpp:508
    if (!ctx->rnds_own.replace(np)) return bail("hipMalloc(rnds)", HipAlloc::last);                                    // main.cpp:509
    if (!ctx->colors_own.replace(nslab)) return bail("hipMalloc(colors)", HipAlloc::last);                             // main.cpp:520
    ctx->d_rnds = ctx->rnds_own;
    ctx->d_colors = ctx->colors_own;
    if (!ctx->d_stats.replace((size_t)kStatCols * kStatRows)) return bail("hipMalloc(stats)", HipAlloc::last);
    if (!ctx->d_tile_counter.replace(kTileCounterWords)) return bail("hipMalloc(tile counter)", HipAlloc::last);
    if ((e = hipMemset(ctx->d_tile_counter, 0, sizeof(uint32_t) * kTileCounterWords)) != hipSuccess) return bail("hipMemset", e);      // zeroed ONCE: the last wave of a launch leaves it zero (k_render)
    if ((e = hipMemset(ctx->d_rays, 0, sizeof(pt_ray) * np)) != hipSuccess) return bail("hipMemset", e);
    if ((e = hipMemset(ctx->d_colors, 0, sizeof(float4) * nslab)) != hipSuccess) return bail("hipMemset", e);
    if ((e = hipMemset(ctx->d_stats, 0, sizeof(unsigned long long) * kStatCols * kStatRows)) != hipSuccess) return bail("hipMemset", e);
    int rc = pt_seed_default(ctx);                                                                                    // main.cpp:522-527
    if (rc != PT_OK) {
        std::string msg = ctx->err;
        pt_destroy(ctx);
        return fail(nullptr, rc, msg);
    }
    *out = ctx;
    return PT_OK;
}

int pt_create(int device, int32_t width, int32_t height, pt_context** out) {
    return pt_create_tiled(device, width, height, 0, 1, 8, out);
}

void pt_destroy(pt_context* ctx) {
    if (!ctx) return;
    if (ctx->has_device) {
        (void)hipSetDevice(ctx->device);
        (void)hipDeviceSynchronize();
        for (auto& e : ctx->events) { if (e.a) (void)hipEventDestroy(e.a); if (e.b) (void)hipEventDestroy(e.b); }
        for (int c = 0; c < kWfMaxChains; ++c) {
            if (ctx->wf_stream[c]) (void)hipStreamDestroy(ctx->wf_stream[c]);
            if (ctx->wf_event[c]) (void)hipEventDestroy(ctx->wf_event[c]);
        }
        if (ctx->comm) comm_destroy(ctx->comm);
        if (ctx->h_adapt_count) (void)hipHostFree(ctx->h_adapt_count);
    }
    delete ctx;      // frees every device array the context owns (DeviceArray, pt_context.hpp): after the synchronise above
}

const char* pt_last_error(const pt_context* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int pt_device_info(const pt_context* ctx, char* buf, int32_t buflen) {
    if (!ctx || !buf || buflen <= 0) return PT_EINVAL;
    std::snprintf(buf, (size_t)buflen, "%s", ctx->info);
    return PT_OK;
}

int pt_add_material(pt_context* ctx, const pt_material* m) {
    if (!ctx || !m) return PT_EINVAL;
    if (ctx->mats.size() >= 65536) return fail(ctx, PT_EINVAL, "more than 65536 materials (mati is a ushort, prog.cl:20)");
    ctx->mats.push_back(*m);
    ctx->mats_uploaded = false;
    return (int)ctx->mats.size() - 1;
}

int pt_add_triangle(pt_context* ctx, const pt_triangle* t) { return pt_add_triangles(ctx, t, 1); }

int pt_add_triangles(pt_context* ctx, const pt_triangle* t, int64_t n) {
    if (!ctx || (!t && n) || n < 0) return PT_EINVAL;
    if ((int64_t)ctx->tris.size() + n > kMaxTriangles)      // checked before anything is read: 32-bit device offsets (pt_internal.hpp)
        return fail(ctx, PT_EINVAL, "more than 2^26 triangles");
    ctx->tris.insert(ctx->tris.end(), t, t + n);
    ctx->tris_uploaded = false;
    return PT_OK;
}

int pt_upload_materials(pt_context* ctx) {
    if (!ctx) return PT_EINVAL;
    post_scene_uploaded(ctx);        // guides, the despeckled frame and the remembered exposure describe the old scene
    ctx->nee_valid = false;          // the light table reads emission and type
    ctx->tex_dirty = true;           // and the bindings on the device the type
    ctx->interior_dirty = true;      // (the interiors' table too)
    for (const pt_triangle& t : ctx->tris)
        if (t.mati >= ctx->mats.size()) return fail(ctx, PT_EINVAL, "a triangle references a material index that was never added");
    ctx->glossy_mats = false;
    ctx->coated_mats = false;
    ctx->frosted_mats = false;
    for (const pt_material& m : ctx->mats) {
        ctx->glossy_mats = ctx->glossy_mats || m.type == 4;
        ctx->coated_mats = ctx->coated_mats || m.type == 5;
        ctx->frosted_mats = ctx->frosted_mats || m.type == 6;
    }
    if (ctx->has_device) {
        PT_HIP(ctx, hipSetDevice(ctx->device));
        // device copy: _pad marks materials whose specular lobe is identically zero (ks == 0, finite
        // shininess >= 0): the kernel then skips pow(), the product ks*pow being +0 either way
        std::vector<pt_material> dm(ctx->mats);
        // a type-4 or type-5 material carries its roughness in n, which only type 2 reads otherwise (options glossy, coated)
        for (pt_material& m : dm) {
            m._pad = (m.ks.s[0] == 0.0f && m.ks.s[1] == 0.0f && m.ks.s[2] == 0.0f && std::isfinite(m.shininess) && m.shininess >= 0.0f) ? 1 : 0;
            if (m.type == 4 || m.type == 5) m.n = pt_material_roughness(m.shininess);
            // a type-6 material keeps its index of refraction in n and carries its roughness in shininess, which only type 0 reads
            // otherwise (option frosted)
            if (m.type == 6) m.shininess = pt_material_roughness(m.shininess);
        }
        ctx->shaderec_dirty = true;
        int rc = upload_vec(ctx, &ctx->d_mats, dm.data(), sizeof(pt_material) * dm.size());
        if (rc != PT_OK) return rc;
        ctx->mats_on_device = (int32_t)dm.size();
    }
    ctx->mats_uploaded = true;
    return PT_OK;
}

int pt_seed_default(pt_context* ctx) {
    PT_NEED_DEVICE(ctx);
    // std::minstd_rand0, default seed 1, drawn in GLOBAL pixel order (main.cpp:45, 522-527)
    const size_t n = (size_t)ctx->W * (size_t)ctx->H;
    std::vector<int32_t> g(n);
    uint64_t x = 1;
    for (size_t i = 0; i < n; ++i) {
        x = (x * 16807ull) % 2147483647ull;
        g[i] = (int32_t)x;
    }
    return seed_upload(ctx, g.data());
}

int pt_upload_seeds(pt_context* ctx, const int32_t* seeds, int64_t n) {
    PT_NEED_DEVICE(ctx);
    if (!seeds || n != (int64_t)ctx->W * ctx->H) return fail(ctx, PT_EINVAL, "seeds must hold width*height ints (global frame)");
    return seed_upload(ctx, seeds);
}

int pt_local_pixel_count(const pt_context* ctx, int64_t* out) {
    if (!ctx || !out) return PT_EINVAL;
    *out = ctx->npix;
    return PT_OK;
}

int pt_slab_pixel_count(const pt_context* ctx, int64_t* out) {
    if (!ctx || !out) return PT_EINVAL;
    *out = ctx->slab_pix;
    return PT_OK;
}

int pt_frame_size(const pt_context* ctx, int32_t* width, int32_t* height, int64_t* npix) {
    if (!ctx) return PT_EINVAL;
    if (width) *width = ctx->W;
    if (height) *height = ctx->H;
    if (npix) *npix = (int64_t)ctx->W * ctx->H;
    return PT_OK;
}

// ---- frame assembly over RCCL (pt_comm.hip)
int pt_comm_available(void) {
    std::string err;
    const int rc = comm_available(&err);
    return rc == PT_OK ? rc : fail(nullptr, rc, err);
}

int pt_comm_unique_id(void* id128) {
    if (!id128) return PT_EINVAL;
    std::string err;
    const int rc = comm_unique_id(id128, &err);
    return rc == PT_OK ? rc : fail(nullptr, rc, err);
}

int pt_comm_init(pt_context* ctx, const void* id128) {
    PT_NEED_DEVICE(ctx);
    if (!id128) return fail(ctx, PT_EINVAL, "id is NULL");
    if (ctx->comm) return fail(ctx, PT_EINVAL, "the context already has a communicator");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    std::string err;
    const int rc = comm_init(id128, ctx->rank, ctx->world, &ctx->comm, &err);
    return rc == PT_OK ? rc : fail(ctx, rc, err);
}

int pt_gather_frame(pt_context* ctx) {
    PT_NEED_DEVICE(ctx);
    if (!ctx->comm) {
        if (ctx->world == 1) return PT_OK;             // the colors buffer IS the frame
        return fail(ctx, PT_EINVAL, "pt_comm_init has not been called on this tiled context");
    }
    PT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t slab = (size_t)ctx->slab_pix;
    PT_ALLOC(ctx, ctx->d_gathered.reserve(slab * (size_t)ctx->world));
    PT_ALLOC(ctx, ctx->d_frame.reserve((size_t)ctx->W * (size_t)ctx->H));
    std::string err;
    const int rc = comm_all_gather(ctx->comm, ctx->d_colors, ctx->d_gathered, slab * 4, ctx->stream, &err);
    if (rc != PT_OK) return fail(ctx, rc, err);
    PT_HIP(ctx, launch_deinterleave(ctx->d_gathered, ctx->d_frame, ctx->W, ctx->H, ctx->world, ctx->rows_per_block, (long long)slab, ctx->stream));
    ctx->frame_epoch = ctx->render_epoch;
    return PT_OK;
}

// The assembled frame: the gathered copy while nothing has been rendered since the gather; for a one-rank context the
// colors buffer otherwise (it IS the frame); for a tiled context nothing -- a frame older than colors is never served.
static const float4* current_frame(const pt_context* ctx) {
    if (ctx->d_frame && ctx->frame_epoch == ctx->render_epoch) return ctx->d_frame;
    return ctx->world == 1 ? ctx->d_colors : nullptr;
}

void* pt_device_frame(pt_context* ctx) { return !ctx ? nullptr : (void*)current_frame(ctx); }

int pt_read_frame(pt_context* ctx, float* out, int64_t npix) {
    PT_NEED_DEVICE(ctx);
    if (!out || npix != (int64_t)ctx->W * ctx->H) return fail(ctx, PT_EINVAL, "npix must equal width * height of the global frame");
    const float4* src = current_frame(ctx);
    if (!src) return fail(ctx, PT_EINVAL, ctx->d_frame ? "the gathered frame is older than colors: call pt_gather_frame again" : "pt_gather_frame has not been called");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP(ctx, hipMemcpy(out, src, sizeof(float4) * (size_t)npix, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_debug_gather_index(int32_t width, int32_t height, int32_t world, int32_t rows_per_block, int64_t slab_stride, int64_t* out) {
    if (width <= 0 || height <= 0 || world < 1 || rows_per_block < 1 || !out) return PT_EINVAL;
    gather_source_index(width, height, world, rows_per_block, (long long)slab_stride, out);
    return PT_OK;
}

int pt_local_pixel_ids(const pt_context* ctx, int32_t* out, int64_t n) {
    if (!ctx || !out || n != ctx->npix) return PT_EINVAL;
    for (int32_t lr = 0; lr < ctx->local_rows; ++lr) {
        const int32_t gr = global_row(*ctx, lr);
        for (int32_t x = 0; x < ctx->W; ++x) out[(size_t)lr * ctx->W + x] = gr * ctx->W + x;
    }
    return PT_OK;
}

int pt_read_colors(pt_context* ctx, float* out, int64_t npix) {
    PT_NEED_DEVICE(ctx);
    if (!out || npix != ctx->npix) return fail(ctx, PT_EINVAL, "npix must equal the local pixel count");
    return read_back(ctx, out, ctx->d_colors, sizeof(float4) * (size_t)npix);
}
int pt_read_rnds(pt_context* ctx, int32_t* out, int64_t npix) {
    PT_NEED_DEVICE(ctx);
    if (!out || npix != ctx->npix) return fail(ctx, PT_EINVAL, "npix must equal the local pixel count");
    return read_back(ctx, out, ctx->d_rnds, sizeof(int32_t) * (size_t)npix);
}
// the samples behind each pixel's colour: its tile's count in an adaptive frame, current_sample otherwise
int pt_read_sample_counts(pt_context* ctx, int32_t* out, int64_t npix) {
    PT_NEED_DEVICE(ctx);
    if (!out || npix != ctx->npix) return fail(ctx, PT_EINVAL, "npix must equal the local pixel count");
    if (!ctx->adaptive_frame) {
        std::fill(out, out + npix, ctx->current_sample);
        return PT_OK;
    }
    std::vector<int32_t> spp((size_t)local_tiles(ctx));
    const int rc = read_back(ctx, spp.data(), ctx->d_adapt_spp, sizeof(int32_t) * spp.size());
    if (rc != PT_OK) return rc;
    const int32_t tiles_x = (ctx->W + 7) / 8;
    for (int64_t i = 0; i < npix; ++i) {
        const int32_t y = (int32_t)(i / ctx->W), x = (int32_t)(i % ctx->W);
        out[i] = spp[(size_t)(y / 8) * tiles_x + x / 8];
    }
    return PT_OK;
}
int pt_read_tile_state(pt_context* ctx, int32_t* spp, float* err, int64_t n_tiles) {
    PT_NEED_DEVICE(ctx);
    if (n_tiles != local_tiles(ctx)) return fail(ctx, PT_EINVAL, "pt_read_tile_state: n_tiles must be the number of 8x8 tiles of the local frame");
    if (!ctx->adaptive_frame) {
        if (spp) std::fill(spp, spp + n_tiles, ctx->current_sample);
        if (err) std::fill(err, err + n_tiles, std::numeric_limits<float>::infinity());
        return PT_OK;
    }
    int rc = PT_OK;
    if (spp && (rc = read_back(ctx, spp, ctx->d_adapt_spp, sizeof(int32_t) * (size_t)n_tiles)) != PT_OK) return rc;
    if (err && (rc = read_back(ctx, err, ctx->d_adapt_err, sizeof(float) * (size_t)n_tiles)) != PT_OK) return rc;
    return PT_OK;
}

// ---- next-event estimation (kernel: pt_nee.hip; the estimator is pinned in include/pt_api.h)
uint32_t pt_nee_rand(uint32_t state, int32_t segment, int32_t dim) { return nee_rand(state, segment, dim); }
// The light table of the uploaded scene, in packed order: type-3 triangles with E.r + E.g + E.b > 0 and non-zero area, P_sel
// proportional to area x (E.r + E.g + E.b) (summed and normalised in double, then rounded; the last cdf entry is 1)
static int nee_table(pt_context* ctx) {
    if (!ctx->tris_uploaded) return fail(ctx, PT_EINVAL, "pt_upload_triangles has not been called");
    if (!ctx->mats_uploaded) return fail(ctx, PT_EINVAL, "pt_upload_materials has not been called");
    if (ctx->nee_valid) return PT_OK;
    const size_t m = ctx->orig.size();
    std::vector<double> wgt, area;
    ctx->nee_tri.clear();
    ctx->nee_cdf.clear();
    ctx->nee_pdf_area.assign(std::max<size_t>(m, 1), 0.0f);
    for (size_t k = 0; k < m; ++k) {
        const pt_triangle& t = ctx->tris[(size_t)ctx->orig[k]];
        const pt_material& mt = ctx->mats[t.mati];
        if (mt.type != 3) continue;
        const double esum = ((double)mt.emission.s[0] + (double)mt.emission.s[1]) + (double)mt.emission.s[2];
        const double e1[3] = {(double)t.r2.s[0] - t.r1.s[0], (double)t.r2.s[1] - t.r1.s[1], (double)t.r2.s[2] - t.r1.s[2]};
        const double e2[3] = {(double)t.r3.s[0] - t.r1.s[0], (double)t.r3.s[1] - t.r1.s[1], (double)t.r3.s[2] - t.r1.s[2]};
        const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
        const double a = 0.5 * std::sqrt(cx * cx + cy * cy + cz * cz);
        if (!(esum > 0.0) || !(a > 0.0) || !std::isfinite(a * esum)) continue;
        ctx->nee_tri.push_back((int32_t)k);
        wgt.push_back(a * esum);
        area.push_back(a);
    }
    double total = 0.0;
    for (double w : wgt) total += w;
    double run = 0.0;
    for (size_t j = 0; j < wgt.size(); ++j) {
        run += wgt[j];
        ctx->nee_cdf.push_back(j + 1 == wgt.size() ? 1.0f : (float)(run / total));
    }
    // P_sel as the kernel samples it, not as the weights ask for it: u0 = m 2^-24 (m < 2^24) picks light j iff
    // cdf[j-1] <= u0 < cdf[j], i.e. for ceil(cdf[j] 2^24) - ceil(cdf[j-1] 2^24) values of m.  (A light whose share rounds to no
    // value of m is never picked: its P_sel / area is 0, and the BSDF strategy keeps its hits at weight 1.)
    double below = 0.0;
    for (size_t j = 0; j < wgt.size(); ++j) {
        const double upto = std::ceil((double)ctx->nee_cdf[j] * 16777216.0);
        ctx->nee_pdf_area[(size_t)ctx->nee_tri[j]] = (float)((upto - below) / 16777216.0 / area[j]);
        below = upto;
    }
    ctx->nee_phi.swap(wgt);          // (the light hierarchy's weights, pt_lighttree.cpp)
    ctx->nee_area.swap(area);
    ctx->lt_valid = false;
    ctx->nee_valid = true;
    ctx->nee_uploaded = false;
    return PT_OK;
}
}  // extern "C"
namespace ptamd {
int light_table_ready(pt_context* ctx) { return nee_table(ctx); }     // for pt_env.cpp
}  // namespace ptamd
extern "C" {
int pt_debug_light_table(pt_context* ctx, int32_t* orig_tri, float* cdf, int64_t cap, int64_t* n) {
    if (!ctx) return PT_EINVAL;
    if (!n || cap < 0) return fail(ctx, PT_EINVAL, "pt_debug_light_table: n is NULL or cap < 0");
    int rc = nee_table(ctx);
    if (rc != PT_OK) return rc;
    *n = (int64_t)ctx->nee_tri.size();
    const size_t k = (size_t)std::min<int64_t>(cap, *n);
    for (size_t j = 0; j < k; ++j) {
        if (orig_tri) orig_tri[j] = ctx->orig[(size_t)ctx->nee_tri[j]];
        if (cdf) cdf[j] = ctx->nee_cdf[j];
    }
    return PT_OK;
}
}  // extern "C"
namespace ptamd {
// What a launch of the NEE kernels needs besides RenderParams (pt_render_nee, the NEE rounds of pt_render_adaptive_ex): the light table
// of the uploaded scene on the device, and the environment's view when a map with a distribution is set (*sky)
int nee_prepare(pt_context* ctx, int32_t strategy, NeeTable* ltp, EnvView* envp, bool* skyp) {
    int rc = PT_OK;
    if ((rc = nee_table(ctx)) != PT_OK) return rc;
    PT_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->nee_uploaded) {
        ctx->d_nee_tri.reset();
        ctx->d_nee_cdf.reset();
        ctx->d_nee_pdf_area.reset();
        const size_t nl = std::max<size_t>(ctx->nee_tri.size(), 1);
        PT_ALLOC(ctx, ctx->d_nee_tri.replace(nl));
        PT_ALLOC(ctx, ctx->d_nee_cdf.replace(nl));
        PT_ALLOC(ctx, ctx->d_nee_pdf_area.replace(ctx->nee_pdf_area.size()));
        if (!ctx->nee_tri.empty()) {
            PT_HIP(ctx, hipMemcpy(ctx->d_nee_tri, ctx->nee_tri.data(), sizeof(int32_t) * ctx->nee_tri.size(), hipMemcpyHostToDevice));
            PT_HIP(ctx, hipMemcpy(ctx->d_nee_cdf, ctx->nee_cdf.data(), sizeof(float) * ctx->nee_cdf.size(), hipMemcpyHostToDevice));
        }
        PT_HIP(ctx, hipMemcpy(ctx->d_nee_pdf_area, ctx->nee_pdf_area.data(), sizeof(float) * ctx->nee_pdf_area.size(), hipMemcpyHostToDevice));
        ctx->nee_uploaded = true;
    }
    NeeTable& lt = *ltp;
    lt.tri = ctx->d_nee_tri;
    lt.cdf = ctx->d_nee_cdf;
    lt.pdf_area = ctx->d_nee_pdf_area;
    lt.n = (int32_t)ctx->nee_tri.size();
    lt.strategy = strategy;
    // an environment without a distribution is all zero: the instances without one compute the same frame
    EnvView& env = *envp;
    const bool sky = ctx->env_set && ctx->env_dist;
    if (sky) {
        env.texels = ctx->d_env_texels;
        env.row_cdf = ctx->d_env_row_cdf;
        env.col_cdf = ctx->d_env_col_cdf;
        env.w = ctx->env_w;
        env.h = ctx->env_h;
        env.scale = ctx->env_scale;
        env.yaw = ctx->env_yaw;
        env.p_env = env_select(ctx, lt.n == 0);
    }
    *skyp = sky;
    return PT_OK;
}
int nee_launch_for(pt_context* ctx, const pt_camera* cam, bool nee_on, NeeLaunch* nl) {
    *nl = NeeLaunch{};                 // (kNeePlain, every view null or zero)
    nl->lens = lens_view(*cam, lens_on(ctx) ? ctx->lens_aperture : 0.0f, ctx->lens_focus);
    if (!nee_on) return PT_OK;
    int rc;
    if ((rc = smooth_prepare(ctx, &nl->vn)) != PT_OK) return rc;
    if ((rc = texture_prepare(ctx, &nl->tv)) != PT_OK) return rc;
    const bool coated = ctx->coated && ctx->coated_mats, glossy = ctx->glossy && (ctx->glossy_mats || coated);
    const bool frosted = ctx->frosted && ctx->frosted_mats;
    if (lights_on(ctx)) {              // (after nee_prepare: the light table is the uploaded scene's)
        const bool no_other = ctx->nee_tri.empty() && !(ctx->env_set && ctx->env_dist);
        nl->lights = LightsView{ctx->d_lights_rec, ctx->d_lights_cdf, (int32_t)ctx->lights.size(), lights_select(ctx, no_other)};
    }
    else nl->lights = LightsView{nullptr, nullptr, 0, 0.0f};      // (kNeeMedium without a set: P_ana = 0, the branch is never taken)
    if (medium_on(ctx)) nl->medium = medium_view(ctx);
    if (grid_on(ctx)) nl->grid = grid_view(ctx);
    if (interior_on(ctx) && (rc = interior_prepare(ctx, &nl->interior)) != PT_OK) return rc;
    const bool ltree = ctx->light_tree && !ctx->nee_tri.empty();      // (after nee_prepare, as above)
    if (ltree && (rc = light_tree_prepare(ctx, &nl->ltree)) != PT_OK) return rc;
    if (area_on(ctx)) nl->area = area_view(ctx, ctx->nee_tri.empty() && !(ctx->env_set && ctx->env_dist) && !lights_on(ctx));
    nl->family = area_on(ctx)                      ? kNeeAreaLights
                 : ltree                           ? kNeeLightTree
                 : interior_on(ctx)                ? kNeeInterior
                 : grid_on(ctx)                    ? kNeeGrid
                 : medium_on(ctx)                  ? kNeeMedium
                 : lights_on(ctx)                  ? kNeeLights
                 : frosted                         ? kNeeFrosted
                 : lens_on(ctx)                    ? kNeeLens
                 : coated                          ? kNeeCoated
                 : glossy                          ? kNeeGlossy
                 : nl->tv.uv                       ? kNeeTex
                 : nl->vn                          ? kNeeSmooth
                                                   : kNeePlain;
    // (every bit says what is live; a family reads the ones that are run-time answers in it: kNeeInterior serves frames with and without a medium
    // or a grid, kNeeLightTree frames with and without an interior binding)
    nl->flags = (ctx->glossy ? kNeeFlagGlossy : 0) | (ctx->coated ? kNeeFlagCoated : 0) | (lens_on(ctx) ? kNeeFlagLens : 0) | (frosted ? kNeeFlagFrosted : 0) |
                (lights_on(ctx) ? kNeeFlagLights : 0) | (medium_on(ctx) ? kNeeFlagMedium : 0) | (grid_on(ctx) ? kNeeFlagGrid : 0) |
                (interior_on(ctx) ? kNeeFlagInterior : 0) | (ltree ? kNeeFlagLightTree : 0);
    return PT_OK;
}
hipError_t launch_nee_noted(pt_context* ctx, const RenderParams& p, const NeeTable& lt, const NeeLaunch& nl) {
    NeeLaunch noted = nl;
    int block = 0;
    noted.block = &block;
    const hipError_t e = launch_nee(p, lt, noted, ctx->npix, ctx->cu_count, ctx->stream);
    if (block > 0) {                   // (a round over an empty tile list launches nothing and leaves the record as it was)
        ctx->nee_family = nl.family;
        ctx->nee_form = (nl.env ? 1 : 0) | (nl.tiled ? 2 : 0);
        ctx->nee_block = block;
    }
    return e;
}
}  // namespace ptamd
extern "C" {
int pt_render_nee(pt_context* ctx, const pt_camera* cam, int32_t iterations, int32_t nsamples, int32_t strategy) {
    if (!ctx) return PT_EINVAL;
    if (iterations < 0 || nsamples < 0) return fail(ctx, PT_EINVAL, "pt_render_nee: iterations/nsamples must be >= 0");
    if (strategy < PT_NEE_BSDF || strategy > PT_NEE_MIS) return fail(ctx, PT_EINVAL, "pt_render_nee: strategy must be PT_NEE_BSDF, PT_NEE_LIGHT or PT_NEE_MIS");
    if (strategy == PT_NEE_BSDF && lights_on(ctx)) return fail(ctx, PT_EINVAL, lights_refusal("pt_render_nee with PT_NEE_BSDF"));
    if (grid_on(ctx) && !grid_unbounded(ctx).empty()) return fail(ctx, PT_EINVAL, "pt_render_nee: " + grid_unbounded(ctx));
    PT_NEED_DEVICE(ctx);
    int rc = check_ready(ctx, cam);
    if (rc != PT_OK) return rc;
    if (ctx->adaptive_frame) return fail(ctx, PT_EINVAL, "pt_render_nee: an adaptive frame is held: pt_set_current_sample(ctx, 0) starts a new frame");
    if ((int64_t)ctx->current_sample + nsamples > INT32_MAX) return fail(ctx, PT_EINVAL, "pt_render_nee: current_sample + nsamples overflows");
    if (nsamples == 0) return PT_OK;
    NeeTable lt;
    EnvView env;
    bool sky = false;
    if ((rc = nee_prepare(ctx, strategy, &lt, &env, &sky)) != PT_OK) return rc;
    NeeLaunch nl;                      // the kernel family and what it reads: vertex normals, textures, lens
    if ((rc = nee_launch_for(ctx, cam, true, &nl)) != PT_OK) return rc;
    nl.env = sky ? &env : nullptr;
    RenderParams p;
    fill_params(ctx, cam, &p);         // the render kernels' node placement
    p.iterations = iterations;
    p.first_sample = ctx->current_sample;
    p.nsamples = nsamples;
    ctx->render_epoch++;
    note_frame(ctx, p.first_sample, cam);
    EventPair* ep;
    if ((rc = time_begin(ctx, &ep)) != PT_OK) return rc;
    PT_HIP(ctx, launch_nee_noted(ctx, p, lt, nl));
    if ((rc = time_end(ctx, ep)) != PT_OK) return rc;
    ctx->current_sample += nsamples;
    return PT_OK;
}

// ---- rough metal (option glossy; kernels: pt_glossy.hip, pt_nee.hip; pinned in include/pt_api.h)
int pt_debug_glossy(pt_context* ctx, int64_t n, const float* N_D_alpha_rnd, float* out) {
    PT_NEED_DEVICE(ctx);
    if (n < 0 || (n > 0 && (!N_D_alpha_rnd || !out))) return fail(ctx, PT_EINVAL, "pt_debug_glossy: n >= 0, both arrays non-null");
    if (n == 0) return PT_OK;
    return debug_round_trip(ctx, N_D_alpha_rnd, sizeof(float) * 9 * (size_t)n, out, sizeof(float) * 8 * (size_t)n,
                            [&](void* d_in, void* d_out) { return launch_debug_glossy((const float*)d_in, n, (float*)d_out, ctx->stream); });
}

// ---- coated diffuse (option coated; kernels: pt_glossy.hip, pt_nee.hip; pinned in include/pt_api.h)
int pt_debug_coated(pt_context* ctx, int64_t n, const float* in, float* out) {
    PT_NEED_DEVICE(ctx);
    if (n < 0 || (n > 0 && (!in || !out))) return fail(ctx, PT_EINVAL, "pt_debug_coated: n >= 0, both arrays non-null");
    if (n == 0) return PT_OK;
    return debug_round_trip(ctx, in, sizeof(float) * 12 * (size_t)n, out, sizeof(float) * 10 * (size_t)n,
                            [&](void* d_in, void* d_out) { return launch_debug_coated((const float*)d_in, n, (float*)d_out, ctx->stream); });
}

// ---- rough dielectric (option frosted; kernels: pt_glossy.hip, pt_nee.hip; pinned in include/pt_api.h)
int pt_debug_frosted(pt_context* ctx, int64_t n, const float* in, float* out) {
    PT_NEED_DEVICE(ctx);
    if (n < 0 || (n > 0 && (!in || !out))) return fail(ctx, PT_EINVAL, "pt_debug_frosted: n >= 0, both arrays non-null");
    if (n == 0) return PT_OK;
    return debug_round_trip(ctx, in, sizeof(float) * 12 * (size_t)n, out, sizeof(float) * 10 * (size_t)n,
                            [&](void* d_in, void* d_out) { return launch_debug_frosted((const float*)d_in, n, (float*)d_out, ctx->stream); });
}

int pt_read_rays(pt_context* ctx, pt_ray* out, int64_t npix) {
    PT_NEED_DEVICE(ctx);
    if (!out || npix != ctx->npix) return fail(ctx, PT_EINVAL, "npix must equal the local pixel count");
    return read_back(ctx, out, ctx->d_rays, sizeof(pt_ray) * (size_t)npix);
}

int pt_resolve_ldr(pt_context* ctx, int32_t which, float* out, int64_t npix) {
    PT_NEED_DEVICE(ctx);
    if (!out || npix != ctx->npix) return fail(ctx, PT_EINVAL, "npix must equal the local pixel count");
    if (which != 0 && which != 1) return fail(ctx, PT_EINVAL, "which must be 0 (Reinhard) or 1 (filt_im)");
    if (which == 1 && ctx->world != 1) return fail(ctx, PT_EINVAL, "filt_im needs the whole frame on one context (3x3 stencil)");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    PT_ALLOC(ctx, ctx->d_ldr.reserve((size_t)std::max<int64_t>(npix, 1)));
    if (which == 0) {
        PT_HIP(ctx, launch_resolve_reinhard(ctx->d_colors, ctx->d_ldr, npix, ctx->stream));
    } else {
        PT_HIP(ctx, hipMemsetAsync(ctx->d_ldr, 0, sizeof(float4) * (size_t)npix, ctx->stream));
        PT_HIP(ctx, launch_filt_im(ctx->d_colors, ctx->d_ldr, ctx->W, ctx->H, ctx->stream));
    }
    return read_back(ctx, out, ctx->d_ldr, sizeof(float4) * (size_t)npix);
}

int pt_bind_framebuffer(pt_context* ctx, void* d_colors, void* d_rnds) {
    PT_NEED_DEVICE(ctx);
    PT_HIP(ctx, hipSetDevice(ctx->device));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (d_colors && d_colors != ctx->d_colors) {
        PT_HIP(ctx, hipMemcpy(d_colors, ctx->d_colors, sizeof(float4) * (size_t)ctx->npix, hipMemcpyDeviceToDevice));
        ctx->colors_own.reset();
        ctx->d_colors = (float4*)d_colors;
    }
    if (d_rnds && d_rnds != ctx->d_rnds) {
        PT_HIP(ctx, hipMemcpy(d_rnds, ctx->d_rnds, sizeof(int32_t) * (size_t)ctx->npix, hipMemcpyDeviceToDevice));
        ctx->rnds_own.reset();
        ctx->d_rnds = (int32_t*)d_rnds;
    }
    return PT_OK;
}

void* pt_device_colors(pt_context* ctx) { return ctx ? (void*)ctx->d_colors : nullptr; }
void* pt_device_rnds(pt_context* ctx) { return ctx ? (void*)ctx->d_rnds : nullptr; }

int pt_set_stream(pt_context* ctx, void* s) {
    PT_NEED_DEVICE(ctx);
    PT_HIP(ctx, hipSetDevice(ctx->device));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stream = (hipStream_t)s;
    return PT_OK;
}

// The options that are one int field of the context: the accepted range (and `also`, where a value inside it is still not one), or for a
// flag any value, stored as 0 / 1; whether the scene has to be uploaded again; the refusal, which begins with the key
struct OptionRow {
    const char* key;
    int pt_context::*field;
    bool flag;
    int64_t lo, hi;
    bool (*also)(int64_t);
    bool reupload;
    const char* refusal;
};
static const OptionRow kOptions[] = {
    {"variant", &pt_context::variant, false, 0, 1, nullptr, false, "variant must be 0 (megakernel) or 1 (wavefront)"},
    {"lds_scene", &pt_context::lds_scene, false, 0, 2, [](int64_t v) { return v != 1; }, false, "lds_scene: 0 every node through L1/L2, 2 stage the tree (or its top) in LDS"},
    {"treelet", &pt_context::treelet, false, -1, 2048, nullptr, true, "treelet: 0 off, -1 as many nodes as fit, 2..2048 nodes"},      // the tree is re-indexed at upload
    {"lbvh_cluster", &pt_context::lbvh_cluster, false, 0, 1 << 20, nullptr, true, "lbvh_cluster: 0 off, 1..2^20 triangles"},
    {"build_threads", &pt_context::build_threads, false, 0, 256, nullptr, false, "build_threads: 0 automatic, 1..256"},
    {"wide_nodes", &pt_context::wide_nodes, false, 0, 2, nullptr, true, "wide_nodes: 0 never, 1 for trees that do not fit LDS, 2 always"},      // the wide nodes are built at upload
    // (the global part of the stacks is sized at upload)
    {"wide_lds_entries", &pt_context::wide_lds_entries, false, 4, kWideLdsEntries, [](int64_t v) { return (v & 1) == 0; }, true, "wide_lds_entries: even, 4..20"},
    {"moments", &pt_context::moments, false, 0, 1, nullptr, false, "moments must be 0 (off) or 1 (second moment of the luminance in colors[].w)"},
    {"smooth_normals", &pt_context::smooth_normals, false, 0, 1, nullptr, false, "smooth_normals must be 0 (geometric normals) or 1 (pt_render_nee shades with interpolated vertex normals)"},
    {"textures", &pt_context::textures, false, 0, 1, nullptr, false, "textures must be 0 (the material's kd) or 1 (pt_render_nee multiplies kd by the bound albedo texture)"},
    {"glossy", &pt_context::glossy, false, 0, 1, nullptr, false, "glossy must be 0 (material type 4 is inert) or 1 (pt_render_nee shades it as a rough metal)"},
    {"coated", &pt_context::coated, false, 0, 1, nullptr, false, "coated must be 0 (material type 5 is inert) or 1 (pt_render_nee shades it as a diffuse base under a rough dielectric coat)"},
    {"frosted", &pt_context::frosted, false, 0, 1, nullptr, false, "frosted must be 0 (material type 6 is inert) or 1 (pt_render_nee shades it as a rough dielectric)"},
    {"light_tree", &pt_context::light_tree, false, 0, 1, nullptr, false, "light_tree must be 0 (a light sample picks its triangle from the table's cdf) or 1 (pt_render_nee picks it by walking the light hierarchy)"},
    {"aov_lights", &pt_context::aov_lights, false, 0, 1, nullptr, false, "aov_lights must be 0 (the guides see triangles only) or 1 (pt_render_aovs and pt_render_aovs_ex see the sphere lights and suns of the area set)"},
    {"timing", &pt_context::timing, true, 0, 0, nullptr, false, nullptr},
    {"count_work", &pt_context::count_work, true, 0, 0, nullptr, false, nullptr},
    {"chunk_taper", &pt_context::chunk_taper, false, -1, 1 << 15, nullptr, false, "chunk_taper: -1 default, 0 off, else the shortest pass"},
    {"chunk_spp", &pt_context::chunk_spp, false, -1, 1 << 20, nullptr, false, "chunk_spp out of range"},
    {"persistent", &pt_context::persistent, true, 0, 0, nullptr, false, nullptr},
    {"sah_visit_cost", &pt_context::sah_visit_cost, false, 0, 1000, nullptr, false, "sah_visit_cost: tenths of a triangle test, 0..1000"},
    {"schedule", &pt_context::schedule, false, -1, 2, nullptr, false, "schedule: -1 automatic, 0 lockstep per sample, 1 restart + tail suspension, 2 the same with lanes moving on to the wave's next work item"},
    {"flat_list", &pt_context::flat_list, false, 0, 32, nullptr, true, "flat_list: 0..32 big triangles tested before the tree (a 32-bit candidate mask per lane)"},
    {"poll_timeout_ms", &pt_context::poll_timeout_ms, false, 1, 40000, nullptr, false, "poll_timeout_ms: 1..40000"},
    {"debug_stall_tile", &pt_context::debug_stall_tile, false, -1, 0x7fffffff, nullptr, false, "debug_stall_tile: -1 none, or a tile index"},
    {"wf_streams", &pt_context::wf_streams, false, -1, kWfMaxChains, [](int64_t v) { return v != 0; }, false, "wf_streams: -1 default, 1..8"},
    {"node_min_lanes", &pt_context::node_min_lanes, false, -1, 63, nullptr, false, "node_min_lanes: -1 default, 0..63"},
    {"leaf_min_lanes", &pt_context::leaf_min_lanes, false, -1, 63, nullptr, false, "leaf_min_lanes: -1 default, 0..63"},
    {"migrate_lanes", &pt_context::migrate_lanes, false, -1, 64, [](int64_t v) { return v != 0; }, false, "migrate_lanes: -1 default, 1..64"},
    {"suspend_lanes", &pt_context::suspend_lanes, false, -1, 63, nullptr, false, "suspend_lanes: -1 default, 0..63"},
    {"waves_per_simd", &pt_context::waves_per_simd, false, -1, 8, [](int64_t v) { return v == -1 || v >= 4; }, false, "waves_per_simd: -1 automatic (at most 7), 4..8 (kernels that read nodes from global memory)"},
    {"bvh_device", &pt_context::bvh_device, false, -1, 1, nullptr, false, "bvh_device: -1 (by scene size), 0 (host) or 1 (device)"},
    {"wide_on_device", &pt_context::wide_on_device, false, 0, 1, nullptr, false, "wide_on_device: 0 or 1"},
    {"sah_grain", &pt_context::sah_grain, false, 8, 1 << 16, nullptr, false, "sah_grain: 8..65536 triangles"},
    {"lbvh_ploc", &pt_context::lbvh_ploc, false, 0, 32, [](int64_t v) { return v == 0 || v == 8 || v == 16 || v == 32; }, false, "lbvh_ploc: 0 (radix tree), 8, 16 or 32 (PLOC search radius)"},
    {"lds_block", &pt_context::lds_block, false, -1, kLdsBlockWide, [](int64_t v) { return v == -1 || v == kLdsBlockBase || v == kLdsBlockWide; }, false, "lds_block: -1 automatic, 512 or 768"},
    {"debug_repeat", &pt_context::debug_repeat, false, 0, 1000, nullptr, false, "debug_repeat: 0..1000 extra timed launches"},
    {"cost_binning", &pt_context::cost_binning, true, 0, 0, nullptr, false, nullptr},
    {"bvh_policy", &pt_context::bvh_policy, false, 0, 5, nullptr, true, "bvh_policy must be 0..5 (4 = device LBVH, 5 = the SAH tree built on the device)"},
};

int pt_set_option(pt_context* ctx, const char* key, int64_t value) {
    if (!ctx || !key) return PT_EINVAL;
    std::string k(key);
    for (const OptionRow& o : kOptions) {
        if (k != o.key) continue;
        if (!o.flag && (value < o.lo || value > o.hi || (o.also && !o.also(value)))) return fail(ctx, PT_EINVAL, o.refusal);
        ctx->*o.field = o.flag ? (value ? 1 : 0) : (int)value;
        if (o.reupload) ctx->tris_uploaded = false;
        return PT_OK;
    }
    if (k != "reset_stats") return fail(ctx, PT_EINVAL, "unknown option: " + k);
    if (ctx->has_device) {
        PT_HIP(ctx, hipSetDevice(ctx->device));
        PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        PT_HIP(ctx, hipMemset(ctx->d_stats, 0, sizeof(unsigned long long) * kStatCols * kStatRows));
    }
    int rc = time_collect(ctx);
    if (rc != PT_OK) return rc;
    ctx->kernel_ms_acc = 0.0;
    ctx->kernel_launches = 0;
    return PT_OK;
}

int pt_get_stat(pt_context* ctx, const char* key, double* out) {
    if (!ctx || !key || !out) return PT_EINVAL;
    std::string k(key);
    if (k == "bvh_nodes") { *out = (double)ctx->nodes.size(); return PT_OK; }
    if (k == "bvh_depth") { *out = (double)ctx->bvh_depth; return PT_OK; }
    if (k == "stack_entries") { *out = (double)stack_entries_for(ctx->interior_depth); return PT_OK; }
    if (k == "bvh_build_ms") { *out = ctx->bvh_build_ms; return PT_OK; }
    if (k == "bvh_on_device") { *out = (double)ctx->bvh_on_device; return PT_OK; }
    if (k == "bvh_median_splits") { *out = (double)ctx->bvh_median_splits; return PT_OK; }
    if (k == "triangles") { *out = (double)ctx->orig.size(); return PT_OK; }
    if (k == "lds_bytes") { *out = (double)ctx->last_lds_bytes; return PT_OK; }
    if (k == "waves_per_simd") { *out = (double)ctx->last_waves_per_simd; return PT_OK; }
    if (k == "treelet_nodes") { *out = (double)ctx->treelet_nodes; return PT_OK; }
    if (k == "wide_nodes") { *out = (double)ctx->nodes4.size(); return PT_OK; }
    if (k == "wide_pending") { *out = (double)ctx->wide_pending; return PT_OK; }
    if (k == "flat_triangles") { *out = (double)ctx->n_flat; return PT_OK; }
    if (k == "obj_textures_loaded") { *out = (double)ctx->obj_textures_loaded; return PT_OK; }
    if (k == "obj_textures_skipped") { *out = (double)ctx->obj_textures_skipped; return PT_OK; }
    if (k == "obj_pieces") { *out = (double)ctx->obj_pieces; return PT_OK; }
    if (k == "flat_boxes") { *out = (double)ctx->n_fbox; return PT_OK; }
    if (k == "node_mode") {      // what the next launch will use: 0 whole tree in LDS, 1 L1/L2 only, 2 treelet
        pt_camera cam;
        std::memset(&cam, 0, sizeof cam);
        RenderParams p;
        fill_params(ctx, &cam, &p);
        *out = (double)p.node_mode;
        return PT_OK;
    }
    if (k == "light_tree_nodes" || k == "light_tree_depth") {      // (builds the tree of the uploaded scene if it is stale; host only)
        const int rc = light_tree_ready(ctx);
        if (rc != PT_OK) return rc;
        *out = k == "light_tree_nodes" ? (double)(ctx->lt_nodes.size() / 8) : (double)ctx->lt_depth;
        return PT_OK;
    }
    if (k == "nee_family") { *out = (double)ctx->nee_family; return PT_OK; }
    if (k == "aov_lights") { *out = ctx->aov_lit ? 1.0 : 0.0; return PT_OK; }
    if (k == "nee_form") { *out = (double)ctx->nee_form; return PT_OK; }
    if (k == "nee_block") { *out = (double)ctx->nee_block; return PT_OK; }
    if (k == "kernel_launches") { *out = (double)ctx->kernel_launches; return PT_OK; }
    PT_NEED_DEVICE(ctx);
    PT_HIP(ctx, hipSetDevice(ctx->device));
    if (k == "kernel_ms") {
        int rc = time_collect(ctx);
        if (rc != PT_OK) return rc;
        *out = ctx->kernel_ms_acc;
        return PT_OK;
    }
    if (k == "segments" || k == "samples" || k == "node_visits" || k == "tri_tests" || k == "wave_node_steps" || k == "wave_tri_steps" || k == "tile_lane_steps" ||
        k == "wave_shade_steps" || k == "wave_trips" || k == "wave_rounds" || k.rfind("low_", 0) == 0) {
        std::vector<unsigned long long> rows((size_t)kStatCols * kStatRows);
        unsigned long long h[kStatCols] = {};
        PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        PT_HIP(ctx, hipMemcpy(rows.data(), ctx->d_stats, sizeof(unsigned long long) * rows.size(), hipMemcpyDeviceToHost));
        for (int r = 0; r < kStatRows; ++r)
            for (int c = 0; c < kStatCols; ++c) h[c] += rows[(size_t)r * kStatCols + c];
        // low_node / low_tri / low_exact / low_shade: executions of that body for at most 8 lanes; exact_steps: all executions of the
        // exact part of the triangle test (counting instances)
        if (k.rfind("low_", 0) == 0 || k == "exact_steps") {
            const int slot = k == "low_node" ? 10 : k == "low_tri" ? 11 : k == "low_exact" ? 12 : k == "low_shade" ? 13 : k == "low_exact_all" ? 15 : -1;
            if (slot < 0) return fail(ctx, PT_EINVAL, "unknown stat " + k);
            *out = (double)h[slot];
            return PT_OK;
        }
        *out = (double)h[k == "segments" ? 0 : k == "samples" ? 1 : k == "node_visits" ? 2 : k == "tri_tests" ? 3 : k == "wave_node_steps" ? 4 : k == "wave_tri_steps" ? 5 : k == "tile_lane_steps" ? 6 : k == "wave_shade_steps" ? 7 : k == "wave_trips" ? 8 : 9];
        return PT_OK;
    }
    return fail(ctx, PT_EINVAL, "unknown stat: " + k);
}

int pt_debug_bvh_sizes(const pt_context* ctx, int64_t* nnodes, int64_t* ntris) {
    if (!ctx) return PT_EINVAL;
    if (nnodes) *nnodes = (int64_t)ctx->nodes.size();
    if (ntris) *ntris = (int64_t)ctx->orig.size();
    return PT_OK;
}

int pt_debug_wide_nodes(const pt_context* ctx, void* out, int64_t capacity, int64_t* count) {
    if (!ctx || !count || capacity < 0) return PT_EINVAL;
    *count = (int64_t)ctx->nodes4.size();
    if (out) std::memcpy(out, ctx->nodes4.data(), sizeof(Node4q) * (size_t)std::min<int64_t>(capacity, *count));
    return PT_OK;
}

int pt_debug_flat_list(const pt_context* ctx, float* packets, uint32_t* pair_mask) {
    if (!ctx || !ctx->tris_uploaded) return PT_EINVAL;
    if (packets)
        for (int k = 0; k < ctx->n_flat; ++k) flat_test_packet(ctx, k, packets + 12 * k);
    if (pair_mask) *pair_mask = ctx->fpair_mask;
    return PT_OK;
}

int pt_debug_bvh_copy(const pt_context* cctx, float* nodes, float* tris, int32_t* meta, int32_t* orig) {
    if (!cctx || !cctx->tris_uploaded) return PT_EINVAL;
    pt_context* ctx = const_cast<pt_context*>(cctx);            // (the host mirror of a device-built tree is filled on demand)
    if (ctx->host_packets_stale && (tris || meta)) {
        const size_t m = ctx->orig.size();
        ctx->packets.resize(m);
        ctx->meta.resize(m);
        PT_HIP(ctx, hipSetDevice(ctx->device));
        PT_HIP(ctx, hipMemcpy(ctx->packets.data(), ctx->d_tris, sizeof(TriPacket) * m, hipMemcpyDeviceToHost));
        PT_HIP(ctx, hipMemcpy(ctx->meta.data(), ctx->d_meta, sizeof(TriMeta) * m, hipMemcpyDeviceToHost));
        ctx->host_packets_stale = false;
    }
    if (nodes) std::memcpy(nodes, ctx->nodes.data(), sizeof(Node64) * ctx->nodes.size());
    if (tris) std::memcpy(tris, ctx->packets.data(), sizeof(TriPacket) * ctx->orig.size());
    if (meta) std::memcpy(meta, ctx->meta.data(), sizeof(TriMeta) * ctx->orig.size());
    if (orig) std::memcpy(orig, ctx->orig.data(), sizeof(int32_t) * ctx->orig.size());
    return PT_OK;
}

namespace {
struct EventOwner {
    hipEvent_t e = nullptr;
    ~EventOwner() { if (e) (void)hipEventDestroy(e); }
};
}  // namespace

int pt_debug_math(pt_context* ctx, int32_t fn, int64_t first, int64_t n, int64_t out[3], uint32_t* bad, int64_t bad_cap) {
    PT_NEED_DEVICE(ctx);
    if (fn < PT_MATH_SQRT || fn > PT_MATH_LCG || first < 0 || n < 0 || !out || bad_cap < 0 || (bad_cap > 0 && !bad))
        return fail(ctx, PT_EINVAL, "pt_debug_math: bad arguments");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    DeviceBuf d_out, d_bad;
    PT_HIP(ctx, d_out.alloc(3 * sizeof(unsigned long long)));
    PT_HIP(ctx, d_bad.alloc(2 * sizeof(uint32_t) * (size_t)std::max<int64_t>(bad_cap, 1)));
    PT_HIP(ctx, hipMemsetAsync(d_out.p, 0, 3 * sizeof(unsigned long long), ctx->stream));
    PT_HIP(ctx, launch_debug_math(fn, (unsigned long long)first, (unsigned long long)n, (unsigned long long*)d_out.p, (uint32_t*)d_bad.p, (long long)bad_cap,
                                  ctx->cu_count, ctx->stream));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    unsigned long long h[3];
    PT_HIP(ctx, hipMemcpy(h, d_out.p, sizeof h, hipMemcpyDeviceToHost));
    for (int i = 0; i < 3; ++i) out[i] = (int64_t)h[i];
    const int64_t k = std::min<int64_t>(out[2], bad_cap);
    if (k > 0) PT_HIP(ctx, hipMemcpy(bad, d_bad.p, 2 * sizeof(uint32_t) * (size_t)k, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_debug_spec(pt_context* ctx, int32_t fn, int64_t n, const uint32_t* in, uint32_t* out) {
    if (!ctx) return PT_EINVAL;
    const size_t wi = (size_t)spec_words_in(fn), wo = (size_t)spec_words_out(fn);
    if (wi == 0) return fail(ctx, PT_EINVAL, "pt_debug_spec: unknown fn");
    if (n < 0 || (n > 0 && (!in || !out))) return fail(ctx, PT_EINVAL, "pt_debug_spec: n >= 0, both arrays non-null");
    if (n == 0) return PT_OK;
    PT_NEED_DEVICE(ctx);
    return debug_round_trip(ctx, in, sizeof(uint32_t) * wi * (size_t)n, out, sizeof(uint32_t) * wo * (size_t)n,
                            [&](void* d_in, void* d_out) { return launch_debug_spec(fn, (const uint32_t*)d_in, n, (uint32_t*)d_out, ctx->stream); });
}

int pt_debug_shade(pt_context* ctx, const pt_camera* cam, int32_t iterations, int32_t instance, int64_t n, const uint32_t* in, uint32_t* out) {
    if (!ctx) return PT_EINVAL;
    if (instance < 0 || instance > (PT_SHADE_SK | PT_SHADE_REC)) return fail(ctx, PT_EINVAL, "pt_debug_shade: unknown instance");
    if (n < 0 || (n > 0 && (!in || !out))) return fail(ctx, PT_EINVAL, "pt_debug_shade: n >= 0, both arrays non-null");
    int rc = check_ready(ctx, cam);
    if (rc != PT_OK) return rc;
    const int64_t n_tris = (int64_t)ctx->orig.size();
    for (int64_t i = 0; i < n; ++i) {
        const int32_t ti = (int32_t)in[(size_t)i * kShadeWordsIn + 7];
        if (ti < 0 || ti >= n_tris) return fail(ctx, PT_EINVAL, "pt_debug_shade: an item's ti is outside the packed triangles");
    }
    if (n == 0) return PT_OK;
    PT_NEED_DEVICE(ctx);
    PT_HIP(ctx, hipSetDevice(ctx->device));
    RenderParams p;
    fill_params(ctx, cam, &p);
    p.iterations = iterations;
    if ((rc = ensure_shade_records(ctx, &p)) != PT_OK) return rc;
    if ((instance & PT_SHADE_REC) && !p.shaderec) return fail(ctx, PT_EINVAL, "pt_debug_shade: this context's launches carry no shading records");
    return debug_round_trip(ctx, in, sizeof(uint32_t) * kShadeWordsIn * (size_t)n, out, sizeof(uint32_t) * kShadeWordsOut * (size_t)n,
                            [&](void* d_in, void* d_out) { return launch_debug_shade(p, instance, (const uint32_t*)d_in, n, (uint32_t*)d_out, ctx->stream); });
}

int pt_debug_closest_hit(pt_context* ctx, const pt_ray* rays, int64_t n, float* out_t, int32_t* out_tri) {
    PT_NEED_DEVICE(ctx);
    if (!rays || !out_t || !out_tri || n < 0) return fail(ctx, PT_EINVAL, "bad arguments");
    if (!ctx->tris_uploaded) return fail(ctx, PT_EINVAL, "pt_upload_triangles has not been called");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    pt_camera cam;
    std::memset(&cam, 0, sizeof cam);
    RenderParams p;
    fill_params(ctx, &cam, &p);         // same node placement as the render kernels would use
    DeviceBuf d_rays, d_t, d_tri;
    PT_HIP(ctx, d_rays.alloc(sizeof(pt_ray) * (size_t)n));
    PT_HIP(ctx, d_t.alloc(sizeof(float) * (size_t)n));
    PT_HIP(ctx, d_tri.alloc(sizeof(int32_t) * (size_t)n));
    if (n) PT_HIP(ctx, hipMemcpy(d_rays.p, rays, sizeof(pt_ray) * (size_t)n, hipMemcpyHostToDevice));
    ctx->last_lds_bytes = traversal_lds_bytes(p, traversal_block(p.node_mode, false));
    PT_HIP(ctx, launch_debug_closest_hit(p, (const pt_ray*)d_rays.p, n, (float*)d_t.p, (int32_t*)d_tri.p, ctx->cu_count, ctx->stream));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->debug_repeat > 0) {      // traversal-only timing: the same launch, debug_repeat times
        EventOwner e0, e1;
        PT_HIP(ctx, hipEventCreate(&e0.e));
        PT_HIP(ctx, hipEventCreate(&e1.e));
        PT_HIP(ctx, hipEventRecord(e0.e, ctx->stream));
        for (int r = 0; r < ctx->debug_repeat; ++r)
            PT_HIP(ctx, launch_debug_closest_hit(p, (const pt_ray*)d_rays.p, n, (float*)d_t.p, (int32_t*)d_tri.p, ctx->cu_count, ctx->stream));
        PT_HIP(ctx, hipEventRecord(e1.e, ctx->stream));
        PT_HIP(ctx, hipEventSynchronize(e1.e));
        float ms = 0.f;
        PT_HIP(ctx, hipEventElapsedTime(&ms, e0.e, e1.e));
        ctx->kernel_ms_acc += ms;
        ctx->kernel_launches += ctx->debug_repeat;
    }
    if (n) {
        PT_HIP(ctx, hipMemcpy(out_t, d_t.p, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
        PT_HIP(ctx, hipMemcpy(out_tri, d_tri.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    }
    for (int64_t i = 0; i < n; ++i)
        if (out_tri[i] >= 0) out_tri[i] = ctx->orig[(size_t)out_tri[i]];      // packed -> add order
    return PT_OK;
}

int pt_debug_deinterleave(pt_context* ctx, const float* gathered, int64_t n_pixels, float* out_frame) {
    PT_NEED_DEVICE(ctx);
    if (!gathered || !out_frame || n_pixels != ctx->slab_pix * ctx->world) return fail(ctx, PT_EINVAL, "gathered must hold world x slab pixels");
    return debug_round_trip(ctx, gathered, sizeof(float4) * (size_t)n_pixels, out_frame, sizeof(float4) * (size_t)ctx->W * (size_t)ctx->H, [&](void* d_g, void* d_f) {
        return launch_deinterleave((const float4*)d_g, (float4*)d_f, ctx->W, ctx->H, ctx->world, ctx->rows_per_block, (long long)ctx->slab_pix, ctx->stream);
    });
}

int pt_debug_scene_sizes(const pt_context* ctx, int64_t* ntris, int64_t* nmats, int64_t* nobjs) {
    if (!ctx) return PT_EINVAL;
    if (ntris) *ntris = (int64_t)ctx->tris.size();
    if (nmats) *nmats = (int64_t)ctx->mats.size();
    if (nobjs) *nobjs = (int64_t)ctx->obj_begin.size();
    return PT_OK;
}

int pt_debug_scene_copy(const pt_context* ctx, pt_triangle* tris, pt_material* mats, int32_t* obj_begin) {
    if (!ctx) return PT_EINVAL;
    if (tris && !ctx->tris.empty()) std::memcpy(tris, ctx->tris.data(), sizeof(pt_triangle) * ctx->tris.size());
    if (mats && !ctx->mats.empty()) std::memcpy(mats, ctx->mats.data(), sizeof(pt_material) * ctx->mats.size());
    if (obj_begin && !ctx->obj_begin.empty()) std::memcpy(obj_begin, ctx->obj_begin.data(), sizeof(int32_t) * ctx->obj_begin.size());
    return PT_OK;
}

int pt_debug_tile_cost(pt_context* ctx, uint32_t* out, int64_t n) {
    PT_NEED_DEVICE(ctx);
    const int64_t n_tiles = (int64_t)((ctx->W + 7) / 8) * ((ctx->local_rows + 7) / 8);
    if (!out || n != n_tiles) return fail(ctx, PT_EINVAL, "pt_debug_tile_cost: n must be the number of 8x8 tiles of the local frame");
    if (!ctx->d_tile_cost) return fail(ctx, PT_EINVAL, "pt_debug_tile_cost: no counting launch yet (option count_work, then pt_render)");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP(ctx, hipMemcpy(out, ctx->d_tile_cost, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_debug_encounter_rank(const pt_context* ctx, int32_t* out, int64_t n) {
    if (!ctx || !out || n != (int64_t)ctx->enc_rank.size()) return PT_EINVAL;
    std::memcpy(out, ctx->enc_rank.data(), sizeof(int32_t) * (size_t)n);
    return PT_OK;
}

}  // extern "C"
