// pt_host.cpp -- host side of libptamd.so: the C ABI of include/pt_api.h (context, authoring, read-back, options, statistics).
//
// What lives here (all of it host work the reference also does on the host):
//   * value-type constructors            main.cpp:101-111, 144-166, 311-347
//   * context life cycle, Scene authoring (add_Material / add_Triangle), seeds, materials
//   * read-back, frame assembly entry points, options, statistics, debug getters
// Scene -> tree is pt_builder.cpp (pt_end_obj, pt_upload_triangles), tree -> launches pt_launch.cpp (pt_render ...); what the
// three share is pt_context.hpp.  There is no CPU render path in this library: every pt_render / pt_trace_rays /
// pt_generate_rays call launches HIP kernels or fails.
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
    ctx->aov_valid = false;
    ctx->despeckle_valid = false;    // (pt_despeckle's result is a frame of the old scene)
    ctx->display_has_prev = false;   // (and pt_display's remembered exposure its brightness)
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

static int read_back(pt_context* ctx, void* dst, const void* src, size_t bytes) {
    const int rc = sync_and_check(ctx);
    if (rc != PT_OK) return rc;
    if (bytes) PT_HIP(ctx, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
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
// ---- guide buffers + a-trous denoiser (kernels: pt_denoise.hip; the filter is pinned in include/pt_api.h)
// the lit instances of k_aovs: option aov_lights, and an area set with a non-black light (what selects kNeeAreaLights)
static bool aov_lit_now(const pt_context* ctx) { return ctx->aov_lights && area_on(ctx); }
int pt_render_aovs(pt_context* ctx, const pt_camera* cam, int32_t subpixels, int32_t specular_depth) {
    if (!ctx) return PT_EINVAL;
    if (subpixels < 1 || subpixels > 8) return fail(ctx, PT_EINVAL, "pt_render_aovs: subpixels must be 1..8");
    if (specular_depth < 0 || specular_depth > 16) return fail(ctx, PT_EINVAL, "pt_render_aovs: specular_depth must be 0..16");
    PT_NEED_DEVICE(ctx);
    int rc = check_ready(ctx, cam);
    if (rc != PT_OK) return rc;
    PT_HIP(ctx, hipSetDevice(ctx->device));
    PT_ALLOC(ctx, ctx->d_aov.reserve(2 * (size_t)std::max<int64_t>(ctx->npix, 1)));
    RenderParams p;
    fill_params(ctx, cam, &p);         // the render kernels' node placement
    const bool lit = aov_lit_now(ctx);
    const AreaLightsView lights = area_view(ctx, true);
    PT_HIP(ctx, launch_aovs(p, subpixels, specular_depth, ctx->npix, ctx->d_aov, ctx->d_aov + ctx->npix, lit ? &lights : nullptr, ctx->cu_count, ctx->stream));
    // the first guides after pt_upload_triangles / pt_upload_materials (which made the old ones stale): the temporal history describes
    // the old scene, and every accumulate needs guides, so this is where it is dropped
    if (!ctx->aov_valid) ctx->temporal_history = false;
    ctx->aov_valid = true;
    ctx->aov_shaded = false;
    ctx->aov_lit = lit;
    ctx->aov_cam = *cam;
    ++ctx->aov_serial;
    return PT_OK;
}
void pt_aov_defaults(pt_aov_params* p) {
    if (!p) return;
    p->subpixels = 1;
    p->specular_depth = 4;
    p->shading = PT_AOV_GEOMETRIC;
}
int pt_render_aovs_ex(pt_context* ctx, const pt_camera* cam, const pt_aov_params* ap) {
    if (!ctx) return PT_EINVAL;
    if (!ap) return fail(ctx, PT_EINVAL, "pt_render_aovs_ex: params is NULL");
    if (ap->subpixels < 1 || ap->subpixels > 8) return fail(ctx, PT_EINVAL, "pt_render_aovs_ex: subpixels must be 1..8");
    if (ap->specular_depth < 0 || ap->specular_depth > 16) return fail(ctx, PT_EINVAL, "pt_render_aovs_ex: specular_depth must be 0..16");
    if (ap->shading != PT_AOV_GEOMETRIC && ap->shading != PT_AOV_SHADED)
        return fail(ctx, PT_EINVAL, "pt_render_aovs_ex: shading must be PT_AOV_GEOMETRIC or PT_AOV_SHADED");
    if (ap->shading == PT_AOV_GEOMETRIC) return pt_render_aovs(ctx, cam, ap->subpixels, ap->specular_depth);
    PT_NEED_DEVICE(ctx);
    int rc = check_ready(ctx, cam);
    if (rc != PT_OK) return rc;
    PT_HIP(ctx, hipSetDevice(ctx->device));
    const float4* vn = nullptr;        // option smooth_normals: the packed vertex normals
    if ((rc = smooth_prepare(ctx, &vn)) != PT_OK) return rc;
    TexView tv;                        // option textures: uvs, texels, descriptors, bindings
    if ((rc = texture_prepare(ctx, &tv)) != PT_OK) return rc;
    PT_ALLOC(ctx, ctx->d_aov.reserve(2 * (size_t)std::max<int64_t>(ctx->npix, 1)));
    RenderParams p;
    fill_params(ctx, cam, &p);         // the render kernels' node placement
    const bool lit = aov_lit_now(ctx);
    const AreaLightsView lights = area_view(ctx, true);
    PT_HIP(ctx, launch_aovs_shaded(p, ap->subpixels, ap->specular_depth, ctx->npix, ctx->d_aov, ctx->d_aov + ctx->npix, vn, tv, ctx->glossy, ctx->coated, ctx->frosted,
                                   lit ? &lights : nullptr, ctx->cu_count, ctx->stream));
    if (!ctx->aov_valid) ctx->temporal_history = false;      // (as pt_render_aovs: the first guides after stale ones)
    ctx->aov_valid = true;
    ctx->aov_shaded = true;
    ctx->aov_lit = lit;
    ctx->aov_cam = *cam;
    ++ctx->aov_serial;
    return PT_OK;
}
int pt_read_aovs(pt_context* ctx, float* albedo_rgbm, float* normal_depth, int64_t npix) {
    PT_NEED_DEVICE(ctx);
    if (npix != ctx->npix) return fail(ctx, PT_EINVAL, "npix must equal the local pixel count");
    if (!ctx->d_aov) return fail(ctx, PT_EINVAL, "pt_read_aovs: pt_render_aovs has not run");
    int rc = PT_OK;
    if (albedo_rgbm && (rc = read_back(ctx, albedo_rgbm, ctx->d_aov, sizeof(float4) * (size_t)npix)) != PT_OK) return rc;
    if (normal_depth && (rc = read_back(ctx, normal_depth, ctx->d_aov + npix, sizeof(float4) * (size_t)npix)) != PT_OK) return rc;
    return PT_OK;
}
void pt_denoise_defaults(pt_denoise_params* p) {
    if (!p) return;
    p->iterations = 3;
    p->sigma_color = 0.125f;
    p->sigma_normal = 8.0f;
    p->sigma_depth = 0.05f;
    p->demodulate = 1;
}
int pt_denoise(pt_context* ctx, const pt_denoise_params* dp) {
    if (!ctx) return PT_EINVAL;
    if (!dp) return fail(ctx, PT_EINVAL, "pt_denoise: params is NULL");
    if (dp->iterations < 1 || dp->iterations > 10) return fail(ctx, PT_EINVAL, "pt_denoise: iterations must be 1..10");
    if (!(dp->sigma_color >= 0.0f) || !(dp->sigma_normal >= 0.0f) || !(dp->sigma_depth >= 0.0f))
        return fail(ctx, PT_EINVAL, "pt_denoise: sigmas must be >= 0 (and not NaN)");
    if (ctx->world != 1) return fail(ctx, PT_EINVAL, "pt_denoise: contexts of one rank (world == 1) only");
    if (!ctx->aov_valid)
        return fail(ctx, PT_EINVAL, "pt_denoise: no guides (pt_render_aovs has not run since the scene was last uploaded)");
    PT_NEED_DEVICE(ctx);
    PT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->npix;
    PT_ALLOC(ctx, ctx->d_dn.reserve(2 * std::max<size_t>(npix, 1)));
    for (int i = 0; i < dp->iterations; ++i) {
        AtrousStep s;
        s.step = 1 << i;
        s.demodulate = dp->demodulate ? 1 : 0;
        s.color_on = std::isfinite(dp->sigma_color) ? 1 : 0;
        s.normal_on = std::isfinite(dp->sigma_normal) && dp->sigma_normal > 0.0f ? 1 : 0;
        s.depth_on = std::isfinite(dp->sigma_depth) ? 1 : 0;
        s.color_scale = (float)(1 << (2 * i));
        s.sigma_color2 = dp->sigma_color * dp->sigma_color;
        s.sigma_normal = dp->sigma_normal;
        s.sigma_depth = dp->sigma_depth;
        const float4* in = i == 0 ? ctx->d_colors : ctx->d_dn + ((i - 1) & 1) * npix;
        float4* out = ctx->d_dn + (i & 1) * npix;
        PT_HIP(ctx, launch_atrous(in, out, ctx->d_aov, ctx->d_aov + npix, ctx->W, ctx->local_rows, s, i == 0, i == dp->iterations - 1, ctx->stream));
    }
    ctx->d_denoised = ctx->d_dn + ((dp->iterations - 1) & 1) * npix;
    return PT_OK;
}
int pt_read_denoised(pt_context* ctx, float* out, int64_t npix) {
    PT_NEED_DEVICE(ctx);
    if (!out || npix != ctx->npix) return fail(ctx, PT_EINVAL, "npix must equal the local pixel count");
    if (!ctx->d_denoised) return fail(ctx, PT_EINVAL, "pt_read_denoised: pt_denoise has not run");
    return read_back(ctx, out, ctx->d_denoised, sizeof(float4) * (size_t)npix);
}
void* pt_device_denoised(pt_context* ctx) { return ctx ? (void*)ctx->d_denoised : nullptr; }

// ---- variance of each pixel's mean luminance (kernel k_variance, pt_denoise.hip; pinned in include/pt_api.h)
static int compute_variance(pt_context* ctx, const char* who) {
    if (!ctx->moments_valid) return fail(ctx, PT_EINVAL, std::string(who) + ": the frame was not rendered with option moments = 1 from its first sample");
    if (ctx->current_sample <= 0) return fail(ctx, PT_EINVAL, std::string(who) + ": the frame has no samples");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    PT_ALLOC(ctx, ctx->d_variance.reserve((size_t)std::max<int64_t>(ctx->npix, 1)));
    PT_HIP(ctx, launch_variance(ctx->d_colors, ctx->adaptive_frame ? ctx->d_adapt_spp : nullptr, ctx->current_sample, ctx->W, ctx->npix,
                                ctx->d_variance, ctx->stream));
    return PT_OK;
}
int pt_read_variance(pt_context* ctx, float* out, int64_t npix) {
    PT_NEED_DEVICE(ctx);
    if (!out || npix != ctx->npix) return fail(ctx, PT_EINVAL, "npix must equal the local pixel count");
    const int rc = compute_variance(ctx, "pt_read_variance");
    if (rc != PT_OK) return rc;
    return read_back(ctx, out, ctx->d_variance, sizeof(float) * (size_t)npix);
}
void* pt_device_variance(pt_context* ctx) {
    if (!ctx || !ctx->has_device) {
        if (ctx) (void)fail(ctx, PT_ENODEVICE, "context was created without a HIP device (host-only); no CPU render path exists");
        return nullptr;
    }
    return compute_variance(ctx, "pt_device_variance") == PT_OK ? (void*)ctx->d_variance : nullptr;
}

// ---- variance-guided a-trous filter (kernel k_atrous_var, pt_denoise.hip; pinned in include/pt_api.h)
void pt_denoise_variance_defaults(pt_denoise_variance_params* p) {
    if (!p) return;
    p->iterations = 2;
    p->sigma_luminance = 4.0f;
    p->sigma_normal = 8.0f;
    p->sigma_depth = 0.05f;
    p->demodulate = 0;
}
// the arguments of the variance-guided filter: "" or what is wrong (pt_denoise_variance, pt_denoise_temporal)
static std::string variance_params_error(const pt_denoise_variance_params* dp) {
    if (!dp) return "params is NULL";
    if (dp->iterations < 1 || dp->iterations > 10) return "iterations must be 1..10";
    if (!(dp->sigma_luminance >= 0.0f) || !(dp->sigma_normal >= 0.0f) || !(dp->sigma_depth >= 0.0f)) return "sigmas must be >= 0 (and not NaN)";
    return "";
}
// the iterations of k_atrous_var over colour in0 (.xyz) and variance var with the current guides, into the two d_dn buffers
static int atrous_var_iterations(pt_context* ctx, const pt_denoise_variance_params* dp, const float4* in0, const float* var) {
    const size_t npix = (size_t)ctx->npix;
    PT_ALLOC(ctx, ctx->d_dn.reserve(2 * std::max<size_t>(npix, 1)));
    for (int i = 0; i < dp->iterations; ++i) {
        AtrousVarStep s;
        s.step = 1 << i;
        s.demodulate = dp->demodulate ? 1 : 0;
        s.lum_on = std::isfinite(dp->sigma_luminance) ? 1 : 0;
        s.normal_on = std::isfinite(dp->sigma_normal) && dp->sigma_normal > 0.0f ? 1 : 0;
        s.depth_on = std::isfinite(dp->sigma_depth) ? 1 : 0;
        s.sigma_luminance = dp->sigma_luminance;
        s.sigma_normal = dp->sigma_normal;
        s.sigma_depth = dp->sigma_depth;
        const float4* in = i == 0 ? in0 : ctx->d_dn + ((i - 1) & 1) * npix;
        float4* out = ctx->d_dn + (i & 1) * npix;
        PT_HIP(ctx, launch_atrous_var(in, var, out, ctx->d_aov, ctx->d_aov + npix, ctx->W, ctx->local_rows, s, i == 0,
                                      i == dp->iterations - 1, ctx->stream));
    }
    ctx->d_denoised = ctx->d_dn + ((dp->iterations - 1) & 1) * npix;
    return PT_OK;
}
int pt_denoise_variance(pt_context* ctx, const pt_denoise_variance_params* dp) {
    if (!ctx) return PT_EINVAL;
    const std::string why = variance_params_error(dp);
    if (!why.empty()) return fail(ctx, PT_EINVAL, "pt_denoise_variance: " + why);
    if (ctx->world != 1) return fail(ctx, PT_EINVAL, "pt_denoise_variance: contexts of one rank (world == 1) only");
    if (!ctx->aov_valid)
        return fail(ctx, PT_EINVAL, "pt_denoise_variance: no guides (pt_render_aovs has not run since the scene was last uploaded)");
    PT_NEED_DEVICE(ctx);
    const int rc = compute_variance(ctx, "pt_denoise_variance");       // (checks the moments)
    if (rc != PT_OK) return rc;
    return atrous_var_iterations(ctx, dp, ctx->d_colors, ctx->d_variance);
}

// ---- temporal accumulation with reprojection (kernel k_temporal, pt_temporal.hip; pinned in include/pt_api.h)
void pt_temporal_defaults(pt_temporal_params* p) {
    if (!p) return;
    p->max_history = 64;
    p->normal_cos = 0.9f;
    p->depth_tolerance = 0.02f;
}
// set s of the two history sets: {r, g, b, m2}, {nx, ny, nz, depth}, {n, material} per local pixel
static float4* temporal_colour(const pt_context* ctx, int s) { return ctx->d_temporal + (size_t)s * (size_t)std::max<int64_t>(ctx->npix, 1); }
static float4* temporal_guides(const pt_context* ctx, int s) { return ctx->d_temporal + (size_t)(2 + s) * (size_t)std::max<int64_t>(ctx->npix, 1); }
static float2* temporal_nm(const pt_context* ctx, int s) {
    const size_t np = (size_t)std::max<int64_t>(ctx->npix, 1);
    return reinterpret_cast<float2*>(ctx->d_temporal + 4 * np) + (size_t)s * np;
}
int pt_temporal_accumulate(pt_context* ctx, const pt_temporal_params* tp) {
    if (!ctx) return PT_EINVAL;
    if (!tp) return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: params is NULL");
    if (tp->max_history < 0) return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: max_history must be >= 0");
    if (!(tp->normal_cos >= -1.0f && tp->normal_cos <= 1.0f)) return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: normal_cos must be in [-1, 1]");
    if (!(tp->depth_tolerance >= 0.0f)) return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: depth_tolerance must be >= 0 (and not NaN)");
    if (ctx->world != 1) return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: contexts of one rank (world == 1) only");
    PT_NEED_DEVICE(ctx);
    if (!ctx->aov_valid)
        return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: no guides (pt_render_aovs has not run since the scene was last uploaded)");
    if (!ctx->moments_valid)
        return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: the frame was not rendered with option moments = 1 from its first sample");
    if (ctx->current_sample <= 0) return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: the frame has no samples");
    if (!ctx->frame_cam_same) return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: the launches of the frame used different cameras");
    if (std::memcmp(&ctx->aov_cam, &ctx->frame_cam, sizeof(pt_camera)) != 0)
        return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: the guides were rendered with a different camera from the frame");
    if (ctx->temporal_frame == ctx->frame_serial) return fail(ctx, PT_EINVAL, "pt_temporal_accumulate: this frame was already accumulated");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t np = (size_t)std::max<int64_t>(ctx->npix, 1);
    static_assert(4 * sizeof(float4) + 2 * sizeof(float2) == 5 * sizeof(float4), "the two history sets: five float4 per local pixel");
    PT_ALLOC(ctx, ctx->d_temporal.reserve(5 * np));
    PT_ALLOC(ctx, ctx->d_temporal_var.reserve(np));
    const int out = ctx->temporal_out == 0 ? 1 : 0, prev = 1 - out;
    TemporalArgs a;
    a.cur = ctx->frame_cam;
    a.prev = ctx->temporal_cam;
    a.colors = ctx->d_colors;
    a.tile_spp = ctx->adaptive_frame ? ctx->d_adapt_spp : nullptr;
    a.n_all = ctx->current_sample;
    a.albedo = ctx->d_aov;
    a.nd = ctx->d_aov + ctx->npix;
    a.prev_c = temporal_colour(ctx, prev);
    a.prev_g = temporal_guides(ctx, prev);
    a.prev_nm = temporal_nm(ctx, prev);
    a.out_c = temporal_colour(ctx, out);
    a.out_g = temporal_guides(ctx, out);
    a.out_nm = temporal_nm(ctx, out);
    a.out_v = ctx->d_temporal_var;
    a.W = ctx->W;
    a.H = ctx->local_rows;
    a.has_prev = ctx->temporal_history ? 1 : 0;
    a.max_history = (float)tp->max_history;
    a.normal_cos = tp->normal_cos;
    a.depth_tolerance = tp->depth_tolerance;
    PT_HIP(ctx, launch_temporal(a, ctx->stream));
    ctx->temporal_out = out;
    ctx->temporal_history = true;
    ctx->temporal_cam = ctx->frame_cam;
    ctx->temporal_frame = ctx->frame_serial;
    ctx->temporal_aov = ctx->aov_serial;
    return PT_OK;
}
int pt_read_temporal(pt_context* ctx, float* rgbv, float* n, int64_t npix) {
    PT_NEED_DEVICE(ctx);
    if (npix != ctx->npix) return fail(ctx, PT_EINVAL, "npix must equal the local pixel count");
    if (ctx->temporal_out < 0) return fail(ctx, PT_EINVAL, "pt_read_temporal: pt_temporal_accumulate has not run");
    int rc = PT_OK;
    if (rgbv) {
        std::vector<float> v((size_t)npix);
        if ((rc = read_back(ctx, rgbv, temporal_colour(ctx, ctx->temporal_out), sizeof(float4) * (size_t)npix)) != PT_OK) return rc;
        if ((rc = read_back(ctx, v.data(), ctx->d_temporal_var, sizeof(float) * (size_t)npix)) != PT_OK) return rc;
        for (int64_t i = 0; i < npix; ++i) rgbv[4 * i + 3] = v[(size_t)i];
    }
    if (n) {
        std::vector<float2> nm((size_t)npix);
        if ((rc = read_back(ctx, nm.data(), temporal_nm(ctx, ctx->temporal_out), sizeof(float2) * (size_t)npix)) != PT_OK) return rc;
        for (int64_t i = 0; i < npix; ++i) n[i] = nm[(size_t)i].x;
    }
    return PT_OK;
}
void* pt_device_temporal(pt_context* ctx) { return ctx && ctx->temporal_out >= 0 ? (void*)temporal_colour(ctx, ctx->temporal_out) : nullptr; }
int pt_denoise_temporal(pt_context* ctx, const pt_denoise_variance_params* dp) {
    if (!ctx) return PT_EINVAL;
    const std::string why = variance_params_error(dp);
    if (!why.empty()) return fail(ctx, PT_EINVAL, "pt_denoise_temporal: " + why);
    if (ctx->world != 1) return fail(ctx, PT_EINVAL, "pt_denoise_temporal: contexts of one rank (world == 1) only");
    PT_NEED_DEVICE(ctx);
    if (!ctx->aov_valid || ctx->temporal_out < 0 || ctx->temporal_aov != ctx->aov_serial)
        return fail(ctx, PT_EINVAL, "pt_denoise_temporal: pt_temporal_accumulate has not run on the current guides");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    return atrous_var_iterations(ctx, dp, temporal_colour(ctx, ctx->temporal_out), ctx->d_temporal_var);
}

// ---- variance-gated firefly filter (kernel k_despeckle, pt_despeckle.hip; pinned in include/pt_api.h)
void pt_despeckle_defaults(pt_despeckle_params* p) {
    if (!p) return;
    p->source = PT_DESPECKLE_FRAME;
    p->radius = 2;
    p->rank = 2;
    p->threshold = 4.0f;
    p->floor = 0.0f;
    p->min_rel_sigma = 0.5f;
    p->spread = 1;
}
// the arguments of the firefly filter: "" or what is wrong (pt_despeckle, pt_debug_despeckle)
static std::string despeckle_params_error(const pt_despeckle_params* dp) {
    if (!dp) return "params is NULL";
    if (dp->radius < 1 || dp->radius > 3) return "radius must be 1..3";
    if (dp->rank < 1 || dp->rank > 3) return "rank must be 1..3";
    if (!(dp->threshold >= 1.0f)) return "threshold must be >= 1 (and not NaN)";
    if (!(dp->floor >= 0.0f)) return "floor must be >= 0 (and not NaN)";
    if (!(dp->min_rel_sigma >= 0.0f)) return "min_rel_sigma must be >= 0 (and not NaN)";
    if (dp->spread != 0 && dp->spread != 1) return "spread must be 0 or 1";
    if (dp->source != PT_DESPECKLE_FRAME && dp->source != PT_DESPECKLE_TEMPORAL) return "source must be PT_DESPECKLE_FRAME or PT_DESPECKLE_TEMPORAL";
    return "";
}
// the three parts of d_despeckle: {r, g, b, v}, v, flags per local pixel
static float* despeckle_var(const pt_context* ctx) { return reinterpret_cast<float*>(ctx->d_despeckle + (size_t)std::max<int64_t>(ctx->npix, 1)); }
static int32_t* despeckle_flags(const pt_context* ctx) { return reinterpret_cast<int32_t*>(despeckle_var(ctx) + (size_t)std::max<int64_t>(ctx->npix, 1)); }
static void despeckle_args(const pt_despeckle_params* dp, DespeckleArgs* a) {
    a->rank = dp->rank;
    a->threshold = dp->threshold;
    a->floor_ = dp->floor;
    a->min_rel_sigma = dp->min_rel_sigma;
}
int pt_despeckle(pt_context* ctx, const pt_despeckle_params* dp) {
    if (!ctx) return PT_EINVAL;
    const std::string why = despeckle_params_error(dp);
    if (!why.empty()) return fail(ctx, PT_EINVAL, "pt_despeckle: " + why);
    if (ctx->world != 1) return fail(ctx, PT_EINVAL, "pt_despeckle: contexts of one rank (world == 1) only");
    PT_NEED_DEVICE(ctx);
    DespeckleArgs a;
    if (dp->source == PT_DESPECKLE_TEMPORAL) {
        if (ctx->temporal_out < 0) return fail(ctx, PT_EINVAL, "pt_despeckle: pt_temporal_accumulate has not run");
        PT_HIP(ctx, hipSetDevice(ctx->device));
        a.c = temporal_colour(ctx, ctx->temporal_out);
        a.v = ctx->d_temporal_var;
    } else {
        const int rc = compute_variance(ctx, "pt_despeckle");          // (checks the moments)
        if (rc != PT_OK) return rc;
        a.c = ctx->d_colors;
        a.v = ctx->d_variance;
    }
    const size_t np = (size_t)std::max<int64_t>(ctx->npix, 1);
    static_assert(sizeof(float4) + sizeof(float) + sizeof(int32_t) == 24, "colour + variance, the variance, the flag: 24 B per local pixel");
    PT_ALLOC(ctx, ctx->d_despeckle.reserve((np * 24 + sizeof(float4) - 1) / sizeof(float4)));
    a.out = ctx->d_despeckle;
    a.out_v = despeckle_var(ctx);
    a.flags = despeckle_flags(ctx);
    a.W = ctx->W;
    a.H = ctx->local_rows;
    despeckle_args(dp, &a);
    ctx->despeckle_valid = false;
    PT_HIP(ctx, launch_despeckle(a, dp->radius, dp->spread, ctx->stream));
    ctx->despeckle_valid = true;
    ctx->despeckle_source = dp->source;
    ctx->despeckle_epoch = ctx->render_epoch;
    ctx->despeckle_frame = ctx->frame_serial;
    ctx->despeckle_temporal = ctx->temporal_frame;
    return PT_OK;
}
int pt_read_despeckled(pt_context* ctx, float* rgbv, int32_t* flags, int64_t npix) {
    PT_NEED_DEVICE(ctx);
    if (npix != ctx->npix) return fail(ctx, PT_EINVAL, "npix must equal the local pixel count");
    if (!ctx->d_despeckle) return fail(ctx, PT_EINVAL, "pt_read_despeckled: pt_despeckle has not run");
    int rc = PT_OK;
    if (rgbv && (rc = read_back(ctx, rgbv, ctx->d_despeckle, sizeof(float4) * (size_t)npix)) != PT_OK) return rc;
    if (flags && (rc = read_back(ctx, flags, despeckle_flags(ctx), sizeof(int32_t) * (size_t)npix)) != PT_OK) return rc;
    return PT_OK;
}
void* pt_device_despeckled(pt_context* ctx) { return ctx ? (void*)ctx->d_despeckle.get() : nullptr; }
int pt_denoise_despeckled(pt_context* ctx, const pt_denoise_variance_params* dp) {
    if (!ctx) return PT_EINVAL;
    const std::string why = variance_params_error(dp);
    if (!why.empty()) return fail(ctx, PT_EINVAL, "pt_denoise_despeckled: " + why);
    if (ctx->world != 1) return fail(ctx, PT_EINVAL, "pt_denoise_despeckled: contexts of one rank (world == 1) only");
    PT_NEED_DEVICE(ctx);
    if (!ctx->aov_valid)
        return fail(ctx, PT_EINVAL, "pt_denoise_despeckled: no guides (pt_render_aovs has not run since the scene was last uploaded)");
    if (!ctx->d_despeckle || !ctx->despeckle_valid) return fail(ctx, PT_EINVAL, "pt_denoise_despeckled: pt_despeckle has not run on the scene as uploaded");
    if (ctx->despeckle_epoch != ctx->render_epoch || ctx->despeckle_frame != ctx->frame_serial)
        return fail(ctx, PT_EINVAL, "pt_denoise_despeckled: the despeckled result is stale (a launch has written colors since pt_despeckle)");
    if (ctx->despeckle_source == PT_DESPECKLE_TEMPORAL && ctx->despeckle_temporal != ctx->temporal_frame)
        return fail(ctx, PT_EINVAL, "pt_denoise_despeckled: the despeckled result is stale (a newer pt_temporal_accumulate ran)");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    return atrous_var_iterations(ctx, dp, ctx->d_despeckle, despeckle_var(ctx));
}
int pt_debug_despeckle(pt_context* ctx, const float* rgbv_in, int32_t w, int32_t h, const pt_despeckle_params* dp, float* rgbv_out, int32_t* flags) {
    if (!ctx) return PT_EINVAL;
    pt_despeckle_params p = {};
    if (dp) {
        p = *dp;
        p.source = PT_DESPECKLE_FRAME;       // (ignored)
    }
    const std::string why = despeckle_params_error(dp ? &p : nullptr);
    if (!why.empty()) return fail(ctx, PT_EINVAL, "pt_debug_despeckle: " + why);
    if (w < 1 || w > 4096 || h < 1 || h > 4096) return fail(ctx, PT_EINVAL, "pt_debug_despeckle: w and h must be 1..4096");
    if (!rgbv_in || !rgbv_out || !flags) return fail(ctx, PT_EINVAL, "pt_debug_despeckle: NULL argument");
    PT_NEED_DEVICE(ctx);
    const size_t n = (size_t)w * (size_t)h;
    std::vector<float4> out(n + (n + 3) / 4);        // {r, g, b, v} per pixel, then the flags
    const int rc = debug_round_trip(ctx, rgbv_in, sizeof(float4) * n, out.data(), sizeof(float4) * out.size(), [&](void* d_in, void* d_out) {
        DespeckleArgs a;
        a.c = static_cast<const float4*>(d_in);
        a.v = nullptr;
        a.out = static_cast<float4*>(d_out);
        a.out_v = nullptr;
        a.flags = reinterpret_cast<int32_t*>(a.out + n);
        a.W = w;
        a.H = h;
        despeckle_args(&p, &a);
        return launch_despeckle(a, p.radius, p.spread, ctx->stream);
    });
    if (rc != PT_OK) return rc;
    std::memcpy(rgbv_out, out.data(), sizeof(float4) * n);
    std::memcpy(flags, out.data() + n, sizeof(int32_t) * n);
    return PT_OK;
}

// ---- display stage (kernels k_display_*, pt_display.hip; pinned in include/pt_api.h)
void pt_display_defaults(pt_display_params* p) {
    if (!p) return;
    p->source = PT_DISPLAY_FRAME;
    p->metering = PT_METER_AUTO;
    p->ev = 0.0f;
    p->key = 0.18f;
    p->low_permille = 100;
    p->high_permille = 950;
    p->min_ev = -16.0f;
    p->max_ev = 16.0f;
    p->adapt = 1.0f;
    p->bloom_levels = 4;
    p->bloom_threshold = 1.0f;
    p->bloom_intensity = 0.0f;
    p->curve = PT_CURVE_ACES;
    p->white = std::numeric_limits<float>::infinity();
    p->encoding = PT_ENCODE_SRGB;
}
// the arguments of the display stage in the pinned order: "" or what is wrong (pt_display, pt_debug_display)
static std::string display_params_error(const pt_display_params* dp) {
    if (!dp) return "params is NULL";
    if (dp->source < PT_DISPLAY_FRAME || dp->source > PT_DISPLAY_DESPECKLED) return "source must be PT_DISPLAY_FRAME .. PT_DISPLAY_DESPECKLED";
    if (dp->metering != PT_METER_MANUAL && dp->metering != PT_METER_AUTO) return "metering must be PT_METER_MANUAL or PT_METER_AUTO";
    if (dp->curve < PT_CURVE_LINEAR || dp->curve > PT_CURVE_ACES) return "curve must be PT_CURVE_LINEAR, PT_CURVE_REINHARD or PT_CURVE_ACES";
    if (dp->encoding != PT_ENCODE_SRGB && dp->encoding != PT_ENCODE_LINEAR) return "encoding must be PT_ENCODE_SRGB or PT_ENCODE_LINEAR";
    for (float f : {dp->ev, dp->key, dp->min_ev, dp->max_ev, dp->adapt, dp->bloom_threshold, dp->bloom_intensity, dp->white})
        if (std::isnan(f)) return "a parameter is NaN";
    if (!(dp->key > 0.0f)) return "key must be > 0";
    if (dp->low_permille < 0 || dp->low_permille >= dp->high_permille || dp->high_permille > 1000) return "permille must be 0 <= low < high <= 1000";
    if (dp->min_ev > dp->max_ev) return "min_ev must be <= max_ev";
    if (!(dp->adapt > 0.0f && dp->adapt <= 1.0f)) return "adapt must be in (0, 1]";
    if (dp->bloom_levels < 1 || dp->bloom_levels > kDisplayMaxLevels) return "bloom_levels must be 1..6";
    if (dp->bloom_threshold < 0.0f) return "bloom_threshold must be >= 0";
    if (dp->bloom_intensity < 0.0f) return "bloom_intensity must be >= 0";
    if (!(dp->white > 0.0f)) return "white must be > 0";
    return "";
}
static void display_args(const pt_display_params* dp, DisplayArgs* a) {
    a->metering = dp->metering;
    a->ev = dp->ev;
    a->key = dp->key;
    a->low_permille = dp->low_permille;
    a->high_permille = dp->high_permille;
    a->min_ev = dp->min_ev;
    a->max_ev = dp->max_ev;
    a->adapt = dp->adapt;
    a->levels = dp->bloom_intensity > 0.0f ? dp->bloom_levels : 0;
    a->threshold = dp->bloom_threshold;
    a->intensity = dp->bloom_intensity;
    a->curve = dp->curve;
    a->white = dp->white;
    a->encoding = dp->encoding;
}
// the bytes of d_display: right behind the float4 result
static uint8_t* display_bytes(const pt_context* ctx) { return reinterpret_cast<uint8_t*>(ctx->d_display + (size_t)std::max<int64_t>(ctx->npix, 1)); }
static void display_info_from(const DisplayStat& st, int32_t levels, struct pt_display_info* out) {
    out->exposure = st.exposure;
    out->mean_log2 = st.mean_log2;
    out->n_metered = st.n_metered;
    out->n_dark = st.n_dark;
    out->n_nonfinite = st.n_nonfinite;
    out->levels = levels;
}
int pt_display(pt_context* ctx, const pt_display_params* dp) {
    if (!ctx) return PT_EINVAL;
    const std::string why = display_params_error(dp);
    if (!why.empty()) return fail(ctx, PT_EINVAL, "pt_display: " + why);
    if (ctx->world != 1) return fail(ctx, PT_EINVAL, "pt_display: contexts of one rank (world == 1) only");
    PT_NEED_DEVICE(ctx);
    DisplayArgs a;
    switch (dp->source) {
    case PT_DISPLAY_DENOISED:
        if (!ctx->d_denoised) return fail(ctx, PT_EINVAL, "pt_display: source DENOISED, but pt_denoise has not run");
        a.c = ctx->d_denoised;
        break;
    case PT_DISPLAY_TEMPORAL:
        if (ctx->temporal_out < 0) return fail(ctx, PT_EINVAL, "pt_display: source TEMPORAL, but pt_temporal_accumulate has not run");
        a.c = temporal_colour(ctx, ctx->temporal_out);
        break;
    case PT_DISPLAY_DESPECKLED:
        if (!ctx->d_despeckle) return fail(ctx, PT_EINVAL, "pt_display: source DESPECKLED, but pt_despeckle has not run");
        a.c = ctx->d_despeckle;
        break;
    default: a.c = ctx->d_colors; break;
    }
    PT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t np = (size_t)std::max<int64_t>(ctx->npix, 1);
    display_args(dp, &a);
    PT_ALLOC(ctx, ctx->d_display.reserve(np + (3 * np + sizeof(float4) - 1) / sizeof(float4)));
    PT_ALLOC(ctx, ctx->d_display_stat.reserve(1));
    if (a.levels > 0) PT_ALLOC(ctx, ctx->d_display_pyr.reserve(display_pyramid_elems(ctx->W, ctx->local_rows, a.levels)));
    a.W = ctx->W;
    a.H = ctx->local_rows;
    a.stat = ctx->d_display_stat;
    a.out = ctx->d_display;
    a.rgb8 = display_bytes(ctx);
    a.pyr = ctx->d_display_pyr;
    a.prev_mode = ctx->display_has_prev ? 1 : 0;
    a.prev_value = 0.0f;
    ctx->display_ran = false;
    ctx->display_has_prev = false;
    PT_HIP(ctx, launch_display(a, ctx->stream));
    ctx->display_ran = true;
    ctx->display_has_prev = true;
    ctx->display_levels = a.levels;
    return PT_OK;
}
int pt_read_display(pt_context* ctx, float* rgba, uint8_t* rgb8, int64_t npix) {
    PT_NEED_DEVICE(ctx);
    if (npix != ctx->npix) return fail(ctx, PT_EINVAL, "npix must equal the local pixel count");
    if (!ctx->display_ran) return fail(ctx, PT_EINVAL, "pt_read_display: pt_display has not run");
    int rc = PT_OK;
    if (rgba && (rc = read_back(ctx, rgba, ctx->d_display, sizeof(float4) * (size_t)npix)) != PT_OK) return rc;
    if (rgb8 && (rc = read_back(ctx, rgb8, display_bytes(ctx), 3 * (size_t)npix)) != PT_OK) return rc;
    return PT_OK;
}
void* pt_device_display(pt_context* ctx) { return ctx && ctx->display_ran ? (void*)ctx->d_display.get() : nullptr; }
int pt_display_info(pt_context* ctx, struct pt_display_info* out) {
    PT_NEED_DEVICE(ctx);
    if (!out) return fail(ctx, PT_EINVAL, "pt_display_info: NULL argument");
    if (!ctx->display_ran) return fail(ctx, PT_EINVAL, "pt_display_info: pt_display has not run");
    DisplayStat st;
    const int rc = read_back(ctx, &st, ctx->d_display_stat, sizeof(st));
    if (rc != PT_OK) return rc;
    display_info_from(st, ctx->display_levels, out);
    return PT_OK;
}
int pt_debug_display_histogram(pt_context* ctx, uint32_t out[256]) {
    PT_NEED_DEVICE(ctx);
    if (!out) return fail(ctx, PT_EINVAL, "pt_debug_display_histogram: NULL argument");
    if (!ctx->display_ran) return fail(ctx, PT_EINVAL, "pt_debug_display_histogram: pt_display has not run");
    return read_back(ctx, out, ctx->d_display_stat, sizeof(uint32_t) * 256);
}
int pt_display_reset(pt_context* ctx) {
    if (!ctx) return PT_EINVAL;
    ctx->display_has_prev = false;
    return PT_OK;
}
int pt_write_display_ppm(pt_context* ctx, const char* path) {
    if (!ctx || !path) return PT_EINVAL;
    PT_NEED_DEVICE(ctx);
    if (!ctx->display_ran) return fail(ctx, PT_EINVAL, "pt_write_display_ppm: pt_display has not run");
    std::vector<uint8_t> bytes(3 * (size_t)ctx->npix);
    const int rc = read_back(ctx, bytes.data(), display_bytes(ctx), bytes.size());
    if (rc != PT_OK) return rc;
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(ctx, PT_EIO, std::string("cannot write ") + path);
    std::fprintf(f, "P6\n%d %d\n255\n", ctx->W, ctx->local_rows);      // (the bytes are top row first already)
    bool ok = std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    ok = (std::fclose(f) == 0) && ok;
    return ok ? PT_OK : fail(ctx, PT_EIO, std::string("cannot write ") + path);
}
int pt_debug_display(pt_context* ctx, const float* rgba_in, int32_t w, int32_t h, const pt_display_params* dp, float prev_exposure, float* rgba_out,
                     uint8_t* rgb8_out, uint32_t* hist, struct pt_display_info* info) {
    if (!ctx) return PT_EINVAL;
    pt_display_params p = {};
    if (dp) {
        p = *dp;
        p.source = PT_DISPLAY_FRAME;         // (ignored)
    }
    const std::string why = display_params_error(dp ? &p : nullptr);
    if (!why.empty()) return fail(ctx, PT_EINVAL, "pt_debug_display: " + why);
    if (w < 1 || w > 4096 || h < 1 || h > 4096) return fail(ctx, PT_EINVAL, "pt_debug_display: w and h must be 1..4096");
    if (!rgba_in || std::isnan(prev_exposure)) return fail(ctx, PT_EINVAL, "pt_debug_display: rgba_in is NULL or prev_exposure is NaN");
    PT_NEED_DEVICE(ctx);
    DisplayArgs a;
    display_args(&p, &a);
    // the output allocation, in float4: the result, its bytes, the DisplayStat, the pyramid
    const size_t n = (size_t)w * (size_t)h, nb = (3 * n + sizeof(float4) - 1) / sizeof(float4), ns = sizeof(DisplayStat) / sizeof(float4);
    static_assert(sizeof(DisplayStat) % sizeof(float4) == 0, "the DisplayStat sits between float4 arrays");
    const size_t back = n + nb + ns;          // what comes back to the host
    std::vector<float4> out(back);
    const int rc = debug_round_trip(ctx, rgba_in, sizeof(float4) * n, out.data(), sizeof(float4) * back, [&](void* d_in, void* d_out) {
        DeviceBuf pyr;                       // (freed when the lambda returns, so the lambda waits for the kernels below)
        if (a.levels > 0) {
            const hipError_t e = pyr.alloc(sizeof(float4) * display_pyramid_elems(w, h, a.levels));
            if (e != hipSuccess) return e;
        }
        a.c = static_cast<const float4*>(d_in);
        a.W = w;
        a.H = h;
        a.out = static_cast<float4*>(d_out);
        a.rgb8 = reinterpret_cast<uint8_t*>(a.out + n);
        a.stat = reinterpret_cast<DisplayStat*>(a.out + n + nb);
        a.pyr = static_cast<float4*>(pyr.p);
        a.prev_mode = prev_exposure > 0.0f ? 2 : 0;
        a.prev_value = prev_exposure;
        hipError_t e = launch_display(a, ctx->stream);
        if (e == hipSuccess && a.levels > 0) e = hipStreamSynchronize(ctx->stream);      // the pyramid must outlive the kernels
        return e;
    });
    if (rc != PT_OK) return rc;
    const DisplayStat* st = reinterpret_cast<const DisplayStat*>(out.data() + n + nb);
    if (rgba_out) std::memcpy(rgba_out, out.data(), sizeof(float4) * n);
    if (rgb8_out) std::memcpy(rgb8_out, out.data() + n, 3 * n);
    if (hist) std::memcpy(hist, st->hist, sizeof(uint32_t) * 256);
    if (info) display_info_from(*st, a.levels, info);
    return PT_OK;
}
int pt_debug_reproject(const pt_camera* cur, const pt_camera* prev, int32_t x, int32_t y, float depth, float out[3]) {
    if (!cur || !prev || !out) return fail(nullptr, PT_EINVAL, "pt_debug_reproject: NULL argument");
    if (!(cur->XM >= 1.0f && cur->XM <= 65535.0f && cur->YM >= 1.0f && cur->YM <= 65535.0f) || x < 0 || y < 0 || x >= (int32_t)cur->XM || y >= (int32_t)cur->YM)
        return fail(nullptr, PT_EINVAL, "pt_debug_reproject: (x, y) must lie in cur's frame");
    if (!reproject(*cur, *prev, y * (int32_t)cur->XM + x, depth, out))
        return fail(nullptr, PT_EINVAL, "pt_debug_reproject: the point is not in front of prev (a <= 0)");
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

// Shaded guides (pt_render_aovs_ex, PT_AOV_SHADED) are a snapshot of the vertex normals, uvs, textures and bindings: an authoring call
// for any of them makes them stale, as an upload makes any guides stale.  Geometric guides read none of that and stay valid.
static void shaded_guides_stale(pt_context* ctx) {
    if (ctx->aov_shaded) ctx->aov_valid = false;
}

// ---- smooth shading from vertex normals (kernels: pt_smooth.hip, pt_nee.hip; pinned in include/pt_api.h)
static bool vn_has(const float* n) {
    for (int c = 0; c < 3; ++c) {
        const float* v = n + 3 * c;
        if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2])) return false;
        if (v[0] == 0.0f && v[1] == 0.0f && v[2] == 0.0f) return false;
    }
    return true;
}

int pt_set_vertex_normals(pt_context* ctx, int64_t first, int64_t count, const float* normals) {
    if (!ctx) return PT_EINVAL;
    if (first < 0 || count < 0 || (count > 0 && !normals) || first + count > (int64_t)ctx->tris.size())
        return fail(ctx, PT_EINVAL, "pt_set_vertex_normals: [first_triangle, first_triangle + count) must lie inside the triangles added so far");
    if (count == 0) return PT_OK;
    if (ctx->vnormals.size() < (size_t)(first + count) * 9) ctx->vnormals.resize((size_t)(first + count) * 9, 0.0f);
    std::memcpy(ctx->vnormals.data() + (size_t)first * 9, normals, sizeof(float) * 9 * (size_t)count);
    ctx->vnormals_dirty = true;
    shaded_guides_stale(ctx);
    return PT_OK;
}

int pt_clear_vertex_normals(pt_context* ctx) {
    if (!ctx) return PT_EINVAL;
    ctx->vnormals.clear();
    ctx->vnormals_dirty = true;
    shaded_guides_stale(ctx);
    return PT_OK;
}

int pt_debug_vertex_normals(const pt_context* ctx, float* normals, int32_t* has) {
    if (!ctx) return PT_EINVAL;
    const size_t n = ctx->tris.size(), have = std::min(n, ctx->vnormals.size() / 9);
    for (size_t i = 0; i < n; ++i) {
        const bool h = i < have && vn_has(ctx->vnormals.data() + 9 * i);
        if (has) has[i] = h ? 1 : 0;
        if (normals)
            for (int c = 0; c < 9; ++c) normals[9 * i + c] = i < have ? ctx->vnormals[9 * i + c] : 0.0f;
    }
    return PT_OK;
}

int pt_compute_vertex_normals(pt_context* ctx, int32_t object, float crease_degrees) {
    if (!ctx) return PT_EINVAL;
    const int32_t nobj = (int32_t)ctx->obj_begin.size();
    if (!(crease_degrees >= 0.0f && crease_degrees <= 180.0f)) return fail(ctx, PT_EINVAL, "pt_compute_vertex_normals: crease_degrees must lie in [0, 180]");
    if (object < -1 || object >= nobj) return fail(ctx, PT_EINVAL, "pt_compute_vertex_normals: object must be -1 (all) or the index of a closed object");
    const double cos_crease = std::cos((double)crease_degrees * 3.14159265358979323846 / 180.0) - 1e-12;
    struct Corner { uint32_t key[3]; int32_t tri, c; };
    auto key_of = [](float f) { uint32_t u; if (f == 0.0f) f = 0.0f * 0.0f; std::memcpy(&u, &f, 4); return u; };      // +0 == -0
    for (int32_t o = object < 0 ? 0 : object; o < (object < 0 ? nobj : object + 1); ++o) {
        const size_t b = (size_t)ctx->obj_begin[(size_t)o], e = o + 1 < nobj ? (size_t)ctx->obj_begin[(size_t)o + 1] : (size_t)ctx->tri_shift;
        if (e <= b) continue;
        const size_t m = e - b;
        std::vector<double> fn(m * 3), ang(m * 3);
        std::vector<char> good(m);
        std::vector<Corner> corners(m * 3);
        for (size_t i = 0; i < m; ++i) {
            const pt_triangle& t = ctx->tris[b + i];
            const double N[3] = {t.N.s[0], t.N.s[1], t.N.s[2]};
            const double l = std::sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
            good[i] = std::isfinite(l) && l > 0.0;
            for (int a = 0; a < 3; ++a) fn[3 * i + a] = good[i] ? N[a] / l : 0.0;
            const float* r[3] = {t.r1.s, t.r2.s, t.r3.s};
            for (int c = 0; c < 3; ++c) {
                const float *p0 = r[c], *p1 = r[(c + 1) % 3], *p2 = r[(c + 2) % 3];
                double u[3], v[3], uu = 0.0, vv = 0.0, uv = 0.0;
                for (int a = 0; a < 3; ++a) {
                    u[a] = (double)p1[a] - p0[a];
                    v[a] = (double)p2[a] - p0[a];
                    uu += u[a] * u[a]; vv += v[a] * v[a]; uv += u[a] * v[a];
                }
                const double den = std::sqrt(uu * vv);
                ang[3 * i + c] = den > 0.0 ? std::acos(std::min(1.0, std::max(-1.0, uv / den))) : 0.0;
                corners[3 * i + c] = Corner{{key_of(p0[0]), key_of(p0[1]), key_of(p0[2])}, (int32_t)i, c};
            }
        }
        // corners at the same position, each group in add order (triangle, then corner)
        std::sort(corners.begin(), corners.end(), [](const Corner& x, const Corner& y) {
            if (x.key[0] != y.key[0]) return x.key[0] < y.key[0];
            if (x.key[1] != y.key[1]) return x.key[1] < y.key[1];
            if (x.key[2] != y.key[2]) return x.key[2] < y.key[2];
            return x.tri != y.tri ? x.tri < y.tri : x.c < y.c;
        });
        if (ctx->vnormals.size() < e * 9) ctx->vnormals.resize(e * 9, 0.0f);
        for (size_t g0 = 0; g0 < corners.size();) {
            size_t g1 = g0 + 1;
            while (g1 < corners.size() && std::memcmp(corners[g1].key, corners[g0].key, sizeof corners[g0].key) == 0) ++g1;
            for (size_t k = g0; k < g1; ++k) {
                const Corner& me = corners[k];
                float* out = ctx->vnormals.data() + (b + (size_t)me.tri) * 9 + 3 * (size_t)me.c;
                out[0] = out[1] = out[2] = 0.0f;
                if (!good[(size_t)me.tri]) continue;
                const double* mine = &fn[3 * (size_t)me.tri];
                double acc[3] = {0.0, 0.0, 0.0};
                for (size_t j = g0; j < g1; ++j) {
                    const Corner& ot = corners[j];
                    if (!good[(size_t)ot.tri]) continue;
                    const double* theirs = &fn[3 * (size_t)ot.tri];
                    const double d = mine[0] * theirs[0] + mine[1] * theirs[1] + mine[2] * theirs[2];
                    if (ot.tri != me.tri && !(d >= cos_crease)) continue;
                    const double w = ang[3 * (size_t)ot.tri + (size_t)ot.c];
                    for (int a = 0; a < 3; ++a) acc[a] += w * theirs[a];
                }
                double l = std::sqrt(acc[0] * acc[0] + acc[1] * acc[1] + acc[2] * acc[2]);
                if (!(l > 0.0)) { acc[0] = mine[0]; acc[1] = mine[1]; acc[2] = mine[2]; l = 1.0; }      // (a degenerate corner: the face normal)
                for (int a = 0; a < 3; ++a) out[a] = (float)(acc[a] / l);
            }
            g0 = g1;
        }
        // a triangle with a corner that got nothing has none
        for (size_t i = 0; i < m; ++i)
            if (!good[i]) std::fill_n(ctx->vnormals.data() + (b + i) * 9, 9, 0.0f);
    }
    ctx->vnormals_dirty = true;
    shaded_guides_stale(ctx);
    return PT_OK;
}
}  // extern "C"
namespace ptamd {
int smooth_prepare(pt_context* ctx, const float4** vn, bool force) {
    *vn = nullptr;
    if (!ctx->smooth_normals && !force) return PT_OK;
    PT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = ctx->orig.size();
    if (ctx->vnormals_dirty || !ctx->d_vnormals) {
        PT_ALLOC(ctx, ctx->d_vnormals.reserve(3 * std::max<size_t>(n, 1)));
        // (an empty scene keeps one all-zero record next to its one all-zero packet, which can never be hit)
        if (n == 0) PT_HIP(ctx, hipMemsetAsync(ctx->d_vnormals, 0, sizeof(float4) * 3, ctx->stream));
        const size_t n_src = std::min(ctx->tris.size(), ctx->vnormals.size() / 9);
        DeviceBuf d_src, d_orig;
        hipError_t e = d_src.alloc(sizeof(float) * 9 * n_src);
        if (e == hipSuccess) e = d_orig.alloc(sizeof(int32_t) * n);
        if (e == hipSuccess && n_src) e = hipMemcpyAsync(d_src.p, ctx->vnormals.data(), sizeof(float) * 9 * n_src, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && n) e = hipMemcpyAsync(d_orig.p, ctx->orig.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = launch_pack_vertex_normals((const float*)d_src.p, (int64_t)n_src, (const int32_t*)d_orig.p, (int32_t)n, ctx->d_vnormals, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // the staging copies end with this block, the host vectors may change
        if (e != hipSuccess) return fail(ctx, PT_EHIP, std::string("vertex normals: ") + hipGetErrorString(e));
        ctx->vnormals_dirty = false;
    }
    *vn = ctx->d_vnormals;
    return PT_OK;
}
}  // namespace ptamd
extern "C" {
int pt_debug_shading_normal(pt_context* ctx, const pt_ray* rays, int64_t n, int32_t* out_tri, float* out_ns) {
    PT_NEED_DEVICE(ctx);
    if (!rays || !out_tri || !out_ns || n < 0) return fail(ctx, PT_EINVAL, "bad arguments");
    if (!ctx->tris_uploaded) return fail(ctx, PT_EINVAL, "pt_upload_triangles has not been called");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    const float4* vn = nullptr;
    const int rc = smooth_prepare(ctx, &vn, true);      // (the packed normals are built whatever the option says)
    if (rc != PT_OK) return rc;
    pt_camera cam;
    std::memset(&cam, 0, sizeof cam);
    RenderParams p;
    fill_params(ctx, &cam, &p);
    DeviceBuf d_rays, d_tri, d_ns;
    PT_HIP(ctx, d_rays.alloc(sizeof(pt_ray) * (size_t)n));
    PT_HIP(ctx, d_tri.alloc(sizeof(int32_t) * (size_t)n));
    PT_HIP(ctx, d_ns.alloc(sizeof(float4) * (size_t)n));
    if (n) PT_HIP(ctx, hipMemcpy(d_rays.p, rays, sizeof(pt_ray) * (size_t)n, hipMemcpyHostToDevice));
    PT_HIP(ctx, launch_debug_shading_normal(p, vn, (const pt_ray*)d_rays.p, n, (int32_t*)d_tri.p, (float4*)d_ns.p, ctx->cu_count, ctx->stream));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n) {
        PT_HIP(ctx, hipMemcpy(out_tri, d_tri.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
        PT_HIP(ctx, hipMemcpy(out_ns, d_ns.p, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost));
    }
    for (int64_t i = 0; i < n; ++i)
        if (out_tri[i] >= 0) out_tri[i] = ctx->orig[(size_t)out_tri[i]];      // packed -> add order
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

// ---- thin lens (pt_set_lens; kernels: pt_lens.hip, pt_nee.hip; pinned in include/pt_api.h)
void pt_lens_defaults(pt_lens_params* p) {
    if (!p) return;
    p->aperture = 0.0f;
    p->focus_distance = 1.0f;
    p->_pad[0] = p->_pad[1] = 0.0f;
}

static std::string lens_check(const pt_lens_params* p) {
    if (!p) return "params is NULL";
    if (!(p->aperture >= 0.0f && std::isfinite(p->aperture))) return "aperture must be >= 0 and finite";
    if (!(p->focus_distance > 0.0f && std::isfinite(p->focus_distance))) return "focus_distance must be > 0 and finite";
    return "";
}

int pt_set_lens(pt_context* ctx, const pt_lens_params* p) {
    if (!ctx) return PT_EINVAL;
    const std::string why = lens_check(p);
    if (!why.empty()) return fail(ctx, PT_EINVAL, "pt_set_lens: " + why);
    ctx->lens_set = true;
    ctx->lens_aperture = p->aperture;
    ctx->lens_focus = p->focus_distance;
    return PT_OK;
}

int pt_clear_lens(pt_context* ctx) {
    if (!ctx) return PT_EINVAL;
    ctx->lens_set = false;
    ctx->lens_aperture = 0.0f;
    ctx->lens_focus = 1.0f;
    return PT_OK;
}

int pt_focus_at(pt_context* ctx, const pt_camera* cam, int32_t x, int32_t y, float* distance) {
    PT_NEED_DEVICE(ctx);
    if (!distance) return fail(ctx, PT_EINVAL, "pt_focus_at: distance is NULL");
    int rc = check_ready(ctx, cam);
    if (rc != PT_OK) return rc;
    if (x < 0 || x >= ctx->W || y < 0 || y >= ctx->H) return fail(ctx, PT_EINVAL, "pt_focus_at: (x, y) must be a pixel of the frame");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    RenderParams p;
    fill_params(ctx, cam, &p);
    DeviceBuf d_out;
    PT_HIP(ctx, d_out.alloc(sizeof(float)));
    PT_HIP(ctx, launch_focus_at(p, lens_view(*cam, 0.0f, 1.0f), y * ctx->W + x, (float*)d_out.p, ctx->cu_count, ctx->stream));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PT_HIP(ctx, hipMemcpy(distance, d_out.p, sizeof(float), hipMemcpyDeviceToHost));
    return PT_OK;
}

int pt_debug_lens(pt_context* ctx, const pt_camera* cam, const pt_lens_params* lens, int64_t n, const int32_t* gid_state, float* out) {
    PT_NEED_DEVICE(ctx);
    if (!cam || n < 0 || (n > 0 && (!gid_state || !out))) return fail(ctx, PT_EINVAL, "pt_debug_lens: camera non-null, n >= 0, both arrays non-null");
    const std::string why = lens_check(lens);
    if (!why.empty()) return fail(ctx, PT_EINVAL, "pt_debug_lens: " + why);
    if (!((int32_t)cam->XM > 0 && (int32_t)cam->YM > 0)) return fail(ctx, PT_EINVAL, "pt_debug_lens: camera XM/YM must be positive");
    if (n == 0) return PT_OK;
    return debug_round_trip(ctx, gid_state, sizeof(int32_t) * 2 * (size_t)n, out, sizeof(float) * 6 * (size_t)n, [&](void* d_in, void* d_out) {
        return launch_debug_lens(*cam, lens_view(*cam, lens->aperture, lens->focus_distance), (const int32_t*)d_in, n, (float*)d_out, ctx->stream);
    });
}

// ---- albedo textures with UV coordinates (kernels: pt_texture.hip, pt_nee.hip; pinned in include/pt_api.h)
// a float in [0, 65504] as an IEEE half, round to nearest even
static uint16_t float_to_half(float f) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint32_t e = (x >> 23) & 0xffu;
    if (e >= 113) {                                      // a normal half
        const uint32_t m = x & 0x7fffffu, rem = m & 0x1fffu;
        uint32_t h = ((e - 112) << 10) | (m >> 13);
        if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;      // (a carry moves into the exponent as it should)
        return (uint16_t)h;
    }
    if (e < 102) return 0;                               // below 2^-25: zero
    const uint32_t m = (x & 0x7fffffu) | 0x800000u;      // a subnormal half: m 2^(e - 150) in units of 2^-24
    const uint32_t shift = 126 - e, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    uint32_t h = m >> shift;
    if (rem > half || (rem == half && (h & 1u))) ++h;
    return (uint16_t)h;
}
static float half_to_float(uint16_t h) {                // no sign, no inf / NaN: what float_to_half produces
    const uint32_t e = h >> 10, m = h & 0x3ffu;
    return e ? std::ldexp((float)(m | 0x400u), (int)e - 25) : std::ldexp((float)m, -24);
}

void pt_texture_defaults(pt_texture_params* p) {
    if (!p) return;
    p->filter = 1;
    p->srgb = 0;
}

int pt_add_texture(pt_context* ctx, const float* rgb, int32_t w, int32_t h, const pt_texture_params* tp) {
    if (!ctx) return PT_EINVAL;
    pt_texture_params p;
    pt_texture_defaults(&p);
    if (tp) p = *tp;
    if (!rgb || w < 1 || h < 1 || w > PT_TEX_MAX_SIZE || h > PT_TEX_MAX_SIZE)
        return fail(ctx, PT_EINVAL, "pt_add_texture: width and height must lie in [1, 8192]");
    if (ctx->tex_desc.size() >= (size_t)PT_TEX_MAX_COUNT) return fail(ctx, PT_EINVAL, "pt_add_texture: more than 1024 textures");
    if ((p.filter != 0 && p.filter != 1) || (p.srgb != 0 && p.srgb != 1)) return fail(ctx, PT_EINVAL, "pt_add_texture: filter and srgb must be 0 or 1");
    const size_t n = (size_t)w * (size_t)h, first = ctx->tex_texels.size();
    if (first + n > 0x7fffffffull) return fail(ctx, PT_EINVAL, "pt_add_texture: more than 2^31 - 1 texels over all textures");
    std::vector<uint64_t> tex(n);
    for (size_t i = 0; i < n; ++i) {
        uint64_t q = 0;
        for (int c = 0; c < 3; ++c) {
            float v = rgb[3 * i + c];
            if (!(std::isfinite(v) && v >= 0.0f && v <= 65504.0f)) return fail(ctx, PT_EINVAL, "pt_add_texture: a texel is not finite, negative or above 65504");
            if (p.srgb) {
                const double d = (double)v;
                v = (float)(d <= 0.04045 ? d / 12.92 : std::pow((d + 0.055) / 1.055, 2.4));
                if (!(v <= 65504.0f)) return fail(ctx, PT_EINVAL, "pt_add_texture: a texel is above 65504 after the sRGB transfer function");
            }
            q |= (uint64_t)float_to_half(v) << (16 * c);
        }
        tex[i] = q;
    }
    ctx->tex_texels.insert(ctx->tex_texels.end(), tex.begin(), tex.end());
    ctx->tex_desc.push_back(TexDesc{(uint32_t)first, w, h, p.filter});
    ctx->tex_dirty = true;
    shaded_guides_stale(ctx);
    return (int)ctx->tex_desc.size() - 1;
}

int pt_clear_textures(pt_context* ctx) {
    if (!ctx) return PT_EINVAL;
    ctx->tex_texels.clear();
    ctx->tex_desc.clear();
    ctx->mat_tex.clear();
    ctx->tex_dirty = true;
    shaded_guides_stale(ctx);
    return PT_OK;
}

int pt_set_material_texture(pt_context* ctx, int32_t material, int32_t texture) {
    if (!ctx) return PT_EINVAL;
    if (material < 0 || (size_t)material >= ctx->mats.size()) return fail(ctx, PT_EINVAL, "pt_set_material_texture: material must be the index of a material added so far");
    if (texture < -1 || texture >= (int32_t)ctx->tex_desc.size()) return fail(ctx, PT_EINVAL, "pt_set_material_texture: texture must be -1 (none) or the index of a texture added so far");
    if (ctx->mat_tex.size() <= (size_t)material) ctx->mat_tex.resize((size_t)material + 1, -1);
    ctx->mat_tex[(size_t)material] = texture;
    ctx->tex_dirty = true;
    shaded_guides_stale(ctx);
    return PT_OK;
}

int pt_debug_texture(const pt_context* ctx, int32_t texture, float* rgb, int64_t cap, int32_t* w, int32_t* h, int32_t* filter) {
    if (!ctx || texture < 0 || (size_t)texture >= ctx->tex_desc.size() || cap < 0) return PT_EINVAL;
    const TexDesc& d = ctx->tex_desc[(size_t)texture];
    if (w) *w = d.w;
    if (h) *h = d.h;
    if (filter) *filter = d.filter;
    if (!rgb) return PT_OK;
    const size_t n = (size_t)d.w * (size_t)d.h;
    if ((uint64_t)cap < n) return PT_EINVAL;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t q = ctx->tex_texels[d.first + i];
        for (int c = 0; c < 3; ++c) rgb[3 * i + c] = half_to_float((uint16_t)(q >> (16 * c)));
    }
    return PT_OK;
}

static bool uv_has(const float* uv) {
    for (int c = 0; c < 6; ++c)
        if (!(std::fabs(uv[c]) <= 65536.0f)) return false;      // (false for NaN and inf)
    return true;
}

int pt_set_vertex_uvs(pt_context* ctx, int64_t first, int64_t count, const float* uvs) {
    if (!ctx) return PT_EINVAL;
    if (first < 0 || count < 0 || (count > 0 && !uvs) || first + count > (int64_t)ctx->tris.size())
        return fail(ctx, PT_EINVAL, "pt_set_vertex_uvs: [first_triangle, first_triangle + count) must lie inside the triangles added so far");
    if (count == 0) return PT_OK;
    if (ctx->vuvs.size() < (size_t)(first + count) * 6) ctx->vuvs.resize((size_t)(first + count) * 6, std::numeric_limits<float>::quiet_NaN());
    std::memcpy(ctx->vuvs.data() + (size_t)first * 6, uvs, sizeof(float) * 6 * (size_t)count);
    ctx->vuvs_dirty = true;
    shaded_guides_stale(ctx);
    return PT_OK;
}

int pt_clear_vertex_uvs(pt_context* ctx) {
    if (!ctx) return PT_EINVAL;
    ctx->vuvs.clear();
    ctx->vuvs_dirty = true;
    shaded_guides_stale(ctx);
    return PT_OK;
}

int pt_debug_vertex_uvs(const pt_context* ctx, float* uvs, int32_t* has) {
    if (!ctx) return PT_EINVAL;
    const size_t n = ctx->tris.size(), have = std::min(n, ctx->vuvs.size() / 6);
    for (size_t i = 0; i < n; ++i) {
        const bool h = i < have && uv_has(ctx->vuvs.data() + 6 * i);
        if (has) has[i] = h ? 1 : 0;
        if (uvs)
            for (int c = 0; c < 6; ++c) uvs[6 * i + c] = h ? ctx->vuvs[6 * i + c] : 0.0f;
    }
    return PT_OK;
}
}  // extern "C"
namespace ptamd {
int texture_prepare(pt_context* ctx, TexView* tv, bool force) {
    *tv = TexView{nullptr, nullptr, nullptr, nullptr};
    if (!ctx->textures && !force) return PT_OK;
    PT_HIP(ctx, hipSetDevice(ctx->device));
    if (ctx->tex_dirty || !ctx->d_mat_tex) {
        // (every array keeps one readable record; a binding is -1 wherever the material on the device is not of type 0 or 5; only the
        // coated instances and the shaded guides under option coated look a type-5 binding up)
        const size_t nmat = std::max<size_t>((size_t)ctx->mats_on_device, 1), ntex = std::max<size_t>(ctx->tex_desc.size(), 1),
                     ntexel = std::max<size_t>(ctx->tex_texels.size(), 1);
        std::vector<int32_t> bind(nmat, -1);
        for (size_t i = 0; i < std::min<size_t>({(size_t)ctx->mats_on_device, ctx->mat_tex.size(), ctx->mats.size()}); ++i)
            if ((ctx->mats[i].type == 0 || ctx->mats[i].type == 5) && ctx->mat_tex[i] >= 0 && ctx->mat_tex[i] < (int32_t)ctx->tex_desc.size()) bind[i] = ctx->mat_tex[i];
        std::vector<TexDesc> desc(ctx->tex_desc);
        desc.resize(ntex, TexDesc{0, 1, 1, 0});
        ctx->d_mat_tex.reset();
        ctx->d_tex_desc.reset();
        ctx->d_tex_texels.reset();
        static_assert(sizeof(uint2) == sizeof(uint64_t), "a texel is 8 bytes");
        PT_ALLOC(ctx, ctx->d_tex_texels.replace(ntexel));
        PT_ALLOC(ctx, ctx->d_tex_desc.replace(ntex));
        PT_ALLOC(ctx, ctx->d_mat_tex.replace(nmat));
        if (ctx->tex_texels.empty()) PT_HIP(ctx, hipMemsetAsync(ctx->d_tex_texels, 0, sizeof(uint64_t), ctx->stream));
        else PT_HIP(ctx, hipMemcpyAsync(ctx->d_tex_texels, ctx->tex_texels.data(), sizeof(uint64_t) * ctx->tex_texels.size(), hipMemcpyHostToDevice, ctx->stream));
        PT_HIP(ctx, hipMemcpyAsync(ctx->d_tex_desc, desc.data(), sizeof(TexDesc) * ntex, hipMemcpyHostToDevice, ctx->stream));
        PT_HIP(ctx, hipMemcpyAsync(ctx->d_mat_tex, bind.data(), sizeof(int32_t) * nmat, hipMemcpyHostToDevice, ctx->stream));
        PT_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the staging vectors end here, the host vectors may change
        ctx->tex_dirty = false;
    }
    const size_t n = ctx->orig.size();
    if (ctx->vuvs_dirty || !ctx->d_vuvs) {
        PT_ALLOC(ctx, ctx->d_vuvs.reserve(2 * std::max<size_t>(n, 1)));
        // (an empty scene keeps one all-zero record next to its one all-zero packet, which can never be hit)
        if (n == 0) PT_HIP(ctx, hipMemsetAsync(ctx->d_vuvs, 0, sizeof(float4) * 2, ctx->stream));
        const size_t n_src = std::min(ctx->tris.size(), ctx->vuvs.size() / 6);
        DeviceBuf d_src, d_orig;
        hipError_t e = d_src.alloc(sizeof(float) * 6 * n_src);
        if (e == hipSuccess) e = d_orig.alloc(sizeof(int32_t) * n);
        if (e == hipSuccess && n_src) e = hipMemcpyAsync(d_src.p, ctx->vuvs.data(), sizeof(float) * 6 * n_src, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && n) e = hipMemcpyAsync(d_orig.p, ctx->orig.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = launch_pack_vertex_uvs((const float*)d_src.p, (int64_t)n_src, (const int32_t*)d_orig.p, (int32_t)n, ctx->d_vuvs, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // the staging copies end with this block, the host vectors may change
        if (e != hipSuccess) return fail(ctx, PT_EHIP, std::string("vertex uvs: ") + hipGetErrorString(e));
        ctx->vuvs_dirty = false;
    }
    *tv = TexView{ctx->d_vuvs, ctx->d_tex_texels, ctx->d_tex_desc, ctx->d_mat_tex};
    return PT_OK;
}
}  // namespace ptamd
extern "C" {
int pt_debug_albedo(pt_context* ctx, const pt_ray* rays, int64_t n, int32_t* out_tri, float* out_rgbt) {
    PT_NEED_DEVICE(ctx);
    if (!rays || !out_tri || !out_rgbt || n < 0) return fail(ctx, PT_EINVAL, "bad arguments");
    if (!ctx->tris_uploaded || !ctx->mats_uploaded) return fail(ctx, PT_EINVAL, "pt_upload_triangles / pt_upload_materials have not been called");
    PT_HIP(ctx, hipSetDevice(ctx->device));
    const float4* vn = nullptr;
    int rc = smooth_prepare(ctx, &vn);                   // (the normals only when the option asks for them: they do not change the albedo)
    if (rc != PT_OK) return rc;
    TexView tv;
    if ((rc = texture_prepare(ctx, &tv, true)) != PT_OK) return rc;      // (the textures whatever the option says)
    pt_camera cam;
    std::memset(&cam, 0, sizeof cam);
    RenderParams p;
    fill_params(ctx, &cam, &p);
    DeviceBuf d_rays, d_tri, d_out;
    PT_HIP(ctx, d_rays.alloc(sizeof(pt_ray) * (size_t)n));
    PT_HIP(ctx, d_tri.alloc(sizeof(int32_t) * (size_t)n));
    PT_HIP(ctx, d_out.alloc(sizeof(float4) * (size_t)n));
    if (n) PT_HIP(ctx, hipMemcpy(d_rays.p, rays, sizeof(pt_ray) * (size_t)n, hipMemcpyHostToDevice));
    PT_HIP(ctx, launch_debug_albedo(p, vn, tv, (const pt_ray*)d_rays.p, n, (int32_t*)d_tri.p, (float4*)d_out.p, ctx->cu_count, ctx->stream));
    PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n) {
        PT_HIP(ctx, hipMemcpy(out_tri, d_tri.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
        PT_HIP(ctx, hipMemcpy(out_rgbt, d_out.p, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost));
    }
    for (int64_t i = 0; i < n; ++i)
        if (out_tri[i] >= 0) out_tri[i] = ctx->orig[(size_t)out_tri[i]];      // packed -> add order
    return PT_OK;
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

int pt_set_option(pt_context* ctx, const char* key, int64_t value) {
    if (!ctx || !key) return PT_EINVAL;
    std::string k(key);
    if (k == "variant") {
        if (value != 0 && value != 1) return fail(ctx, PT_EINVAL, "variant must be 0 (megakernel) or 1 (wavefront)");
        ctx->variant = (int)value;
    } else if (k == "lds_scene") {
        if (value != 0 && value != 2) return fail(ctx, PT_EINVAL, "lds_scene: 0 every node through L1/L2, 2 stage the tree (or its top) in LDS");
        ctx->lds_scene = (int)value;
    } else if (k == "treelet") {
        if (value < -1 || value > 2048) return fail(ctx, PT_EINVAL, "treelet: 0 off, -1 as many nodes as fit, 2..2048 nodes");
        ctx->treelet = (int)value;
        ctx->tris_uploaded = false;                  // the tree is re-indexed at upload
    } else if (k == "lbvh_cluster") {
        if (value < 0 || value > (1 << 20)) return fail(ctx, PT_EINVAL, "lbvh_cluster: 0 off, 1..2^20 triangles");
        ctx->lbvh_cluster = (int)value;
        ctx->tris_uploaded = false;
    } else if (k == "build_threads") {
        if (value < 0 || value > 256) return fail(ctx, PT_EINVAL, "build_threads: 0 automatic, 1..256");
        ctx->build_threads = (int)value;
    } else if (k == "wide_nodes") {
        if (value < 0 || value > 2) return fail(ctx, PT_EINVAL, "wide_nodes: 0 never, 1 for trees that do not fit LDS, 2 always");
        ctx->wide_nodes = (int)value;
        ctx->tris_uploaded = false;                  // the wide nodes are built at upload
    } else if (k == "wide_lds_entries") {
        if (value < 4 || value > kWideLdsEntries || (value & 1)) return fail(ctx, PT_EINVAL, "wide_lds_entries: even, 4..20");
        ctx->wide_lds_entries = (int)value;
        ctx->tris_uploaded = false;                  // the global part of the stacks is sized at upload
    } else if (k == "moments") {
        if (value != 0 && value != 1) return fail(ctx, PT_EINVAL, "moments must be 0 (off) or 1 (second moment of the luminance in colors[].w)");
        ctx->moments = (int)value;
    } else if (k == "smooth_normals") {
        if (value != 0 && value != 1) return fail(ctx, PT_EINVAL, "smooth_normals must be 0 (geometric normals) or 1 (pt_render_nee shades with interpolated vertex normals)");
        ctx->smooth_normals = (int)value;
    } else if (k == "textures") {
        if (value != 0 && value != 1) return fail(ctx, PT_EINVAL, "textures must be 0 (the material's kd) or 1 (pt_render_nee multiplies kd by the bound albedo texture)");
        ctx->textures = (int)value;
    } else if (k == "glossy") {
        if (value != 0 && value != 1) return fail(ctx, PT_EINVAL, "glossy must be 0 (material type 4 is inert) or 1 (pt_render_nee shades it as a rough metal)");
        ctx->glossy = (int)value;
    } else if (k == "coated") {
        if (value != 0 && value != 1) return fail(ctx, PT_EINVAL, "coated must be 0 (material type 5 is inert) or 1 (pt_render_nee shades it as a diffuse base under a rough dielectric coat)");
        ctx->coated = (int)value;
    } else if (k == "frosted") {
        if (value != 0 && value != 1) return fail(ctx, PT_EINVAL, "frosted must be 0 (material type 6 is inert) or 1 (pt_render_nee shades it as a rough dielectric)");
        ctx->frosted = (int)value;
    } else if (k == "light_tree") {
        if (value != 0 && value != 1) return fail(ctx, PT_EINVAL, "light_tree must be 0 (a light sample picks its triangle from the table's cdf) or 1 (pt_render_nee picks it by walking the light hierarchy)");
        ctx->light_tree = (int)value;
    } else if (k == "aov_lights") {
        if (value != 0 && value != 1) return fail(ctx, PT_EINVAL, "aov_lights must be 0 (the guides see triangles only) or 1 (pt_render_aovs and pt_render_aovs_ex see the sphere lights and suns of the area set)");
        ctx->aov_lights = (int)value;
    } else if (k == "timing") {
        ctx->timing = value ? 1 : 0;
    } else if (k == "count_work") {
        ctx->count_work = value ? 1 : 0;
    } else if (k == "chunk_taper") {
        if (value < -1 || value > 1 << 15) return fail(ctx, PT_EINVAL, "chunk_taper: -1 default, 0 off, else the shortest pass");
        ctx->chunk_taper = (int)value;
    } else if (k == "chunk_spp") {
        if (value < -1 || value > 1 << 20) return fail(ctx, PT_EINVAL, "chunk_spp out of range");
        ctx->chunk_spp = (int)value;
    } else if (k == "persistent") {
        ctx->persistent = value ? 1 : 0;
    } else if (k == "sah_visit_cost") {
        if (value < 0 || value > 1000) return fail(ctx, PT_EINVAL, "sah_visit_cost: tenths of a triangle test, 0..1000");
        ctx->sah_visit_cost = (int)value;
    } else if (k == "schedule") {
        if (value < -1 || value > 2) return fail(ctx, PT_EINVAL, "schedule: -1 automatic, 0 lockstep per sample, 1 restart + tail suspension, 2 the same with lanes moving on to the wave's next work item");
        ctx->schedule = (int)value;
    } else if (k == "flat_list") {
        if (value < 0 || value > 32) return fail(ctx, PT_EINVAL, "flat_list: 0..32 big triangles tested before the tree (a 32-bit candidate mask per lane)");
        ctx->flat_list = (int)value;
        ctx->tris_uploaded = false;
    } else if (k == "poll_timeout_ms") {
        if (value < 1 || value > 40000) return fail(ctx, PT_EINVAL, "poll_timeout_ms: 1..40000");
        ctx->poll_timeout_ms = (int)value;
    } else if (k == "debug_stall_tile") {
        if (value < -1 || value > 0x7fffffff) return fail(ctx, PT_EINVAL, "debug_stall_tile: -1 none, or a tile index");
        ctx->debug_stall_tile = (int)value;
    } else if (k == "wf_streams") {
        if (value < -1 || value == 0 || value > kWfMaxChains) return fail(ctx, PT_EINVAL, "wf_streams: -1 default, 1..8");
        ctx->wf_streams = (int)value;
    } else if (k == "node_min_lanes" || k == "leaf_min_lanes") {
        if (value < -1 || value > 63) return fail(ctx, PT_EINVAL, k + ": -1 default, 0..63");
        (k == "node_min_lanes" ? ctx->node_min_lanes : ctx->leaf_min_lanes) = (int)value;
    } else if (k == "migrate_lanes") {
        if (value != -1 && (value < 1 || value > 64)) return fail(ctx, PT_EINVAL, "migrate_lanes: -1 default, 1..64");
        ctx->migrate_lanes = (int)value;
    } else if (k == "suspend_lanes") {
        if (value < -1 || value > 63) return fail(ctx, PT_EINVAL, "suspend_lanes: -1 default, 0..63");
        ctx->suspend_lanes = (int)value;
    } else if (k == "waves_per_simd") {
        if (value != -1 && (value < 4 || value > 8)) return fail(ctx, PT_EINVAL, "waves_per_simd: -1 automatic (at most 7), 4..8 (kernels that read nodes from global memory)");
        ctx->waves_per_simd = (int)value;
    } else if (k == "bvh_device") {
        if (value < -1 || value > 1) return fail(ctx, PT_EINVAL, "bvh_device: -1 (by scene size), 0 (host) or 1 (device)");
        ctx->bvh_device = (int)value;
    } else if (k == "wide_on_device") {
        if (value != 0 && value != 1) return fail(ctx, PT_EINVAL, "wide_on_device: 0 or 1");
        ctx->wide_on_device = (int)value;
    } else if (k == "sah_grain") {
        if (value < 8 || value > (1 << 16)) return fail(ctx, PT_EINVAL, "sah_grain: 8..65536 triangles");
        ctx->sah_grain = (int)value;
    } else if (k == "lbvh_ploc") {
        if (value != 0 && value != 8 && value != 16 && value != 32) return fail(ctx, PT_EINVAL, "lbvh_ploc: 0 (radix tree), 8, 16 or 32 (PLOC search radius)");
        ctx->lbvh_ploc = (int)value;
    } else if (k == "lds_block") {
        if (value != -1 && value != kLdsBlockBase && value != kLdsBlockWide) return fail(ctx, PT_EINVAL, "lds_block: -1 automatic, 512 or 768");
        ctx->lds_block = (int)value;
    } else if (k == "debug_repeat") {
        if (value < 0 || value > 1000) return fail(ctx, PT_EINVAL, "debug_repeat: 0..1000 extra timed launches");
        ctx->debug_repeat = (int)value;
    } else if (k == "cost_binning") {
        ctx->cost_binning = value ? 1 : 0;
    } else if (k == "bvh_policy") {
        if (value < 0 || value > 5) return fail(ctx, PT_EINVAL, "bvh_policy must be 0..5 (4 = device LBVH, 5 = the SAH tree built on the device)");
        ctx->bvh_policy = (int)value;
        ctx->tris_uploaded = false;
    } else if (k == "reset_stats") {
        if (ctx->has_device) {
            PT_HIP(ctx, hipSetDevice(ctx->device));
            PT_HIP(ctx, hipStreamSynchronize(ctx->stream));
            PT_HIP(ctx, hipMemset(ctx->d_stats, 0, sizeof(unsigned long long) * kStatCols * kStatRows));
        }
        int rc = time_collect(ctx);
        if (rc != PT_OK) return rc;
        ctx->kernel_ms_acc = 0.0;
        ctx->kernel_launches = 0;
    } else {
        return fail(ctx, PT_EINVAL, "unknown option: " + k);
    }
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
