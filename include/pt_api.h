/*
 * pt_api.h -- C ABI of the MI355X-native path-tracing hot path (libptamd.so).
 *
 * Drop-in boundary: the reference's host class `Scene` (main.cpp:363-742) and the value
 * types it is fed (main.cpp:92-193, 306-348).  Every entry point below names the
 * reference interface it replaces ("main.cpp:NN" = /root/reference/main.cpp,
 * "prog.cl:NN" = /root/reference/prog.cl).  Call order is the reference's:
 *
 *   pt_create                       (Scene::init_Scene)
 *   pt_add_material*                (Scene::add_Material)
 *   (pt_add_triangle* pt_end_obj)*  (Scene::add_Triangle / Scene::end_Obj)   | pt_add_obj*
 *   pt_upload_triangles             (Scene::upload_Triangles)
 *   pt_upload_materials             (Scene::upload_Materials)
 *   pt_render* | (pt_generate_rays pt_trace_rays)*        (Scene::render / generate_rays / trace_rays)
 *   pt_read_colors / pt_read_rnds / pt_read_rays / pt_resolve_ldr
 *   pt_destroy
 *
 * Conventions: plain pointers and sizes, no C++ or torch types.  Every function returns
 * PT_OK (0) or a negative PT_E* code and never calls exit(); the message is available from
 * pt_last_error().  Upload/add functions copy (the caller keeps ownership of its arrays);
 * read functions fill caller-provided host buffers.  One host thread per context; one
 * context per GPU.  Nothing here runs on the CPU as a fallback: without a usable HIP
 * device pt_create fails with PT_ENODEVICE.
 */
#ifndef PT_API_H
#define PT_API_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PT_OK 0
#define PT_EINVAL (-1)     /* bad argument / call order */
#define PT_ENODEVICE (-2)  /* no HIP device, or the device is not gfx950-compatible */
#define PT_EHIP (-3)       /* a HIP runtime call failed (text in pt_last_error) */
#define PT_ESCENE (-4)     /* scene cannot be built (e.g. the reference's build would not terminate) */
#define PT_EIO (-5)        /* a file could not be read, parsed or written */
#define PT_ECOMM (-6)      /* RCCL is unavailable or a collective failed (text in pt_last_error) */

/* ---- value types, byte-compatible with the reference's device structs ------------ */
typedef struct { float s[4]; } pt_float3;                 /* cl_float3: 16 B, .s[3] is padding */
typedef struct {                                           /* Material: prog.cl:1-5, main.cpp:92-112 (80 B) */
    pt_float3 kd, ks, emission, F0;
    float n, shininess;
    int32_t type;                                          /* 0 diffuse, 1 mirror, 2 dielectric, 3 emitter */
    int32_t _pad;
} pt_material;
typedef struct { pt_float3 P, D; } pt_ray;                 /* Ray: prog.cl:7-9 (32 B) */
typedef struct {                                           /* Triangle: prog.cl:18-21, main.cpp:139-182 (80 B) */
    pt_float3 r1, r2, r3, N;
    uint16_t mati;
    uint8_t _pad[14];
} pt_triangle;
typedef struct {                                           /* Camera: prog.cl:32-35, main.cpp:306-348 (80 B) */
    pt_float3 eye, lookat, up, right;
    float XM, YM;
    float _pad[2];
} pt_camera;

typedef struct pt_context pt_context;

/* ---- value-type constructors (host arithmetic of the reference's constructors) --- */
/* Material(kd,ks,emission,N,K,shininess,type): main.cpp:101-111 */
void pt_material_init(pt_material* m, const float kd[3], const float ks[3], const float emission[3],
                      const float N[3], const float K[3], float shininess, int32_t type);
/* Triangle(r1,r2,r3,mati): main.cpp:144-166 (precomputes the unit geometric normal) */
void pt_triangle_init(pt_triangle* t, const float r1[3], const float r2[3], const float r3[3], uint16_t mati);
/* n x Triangle(...): verts holds 9 floats per triangle (r1, r2, r3), mati one index each */
void pt_triangles_init(pt_triangle* out, const float* verts, const uint16_t* mati, int64_t n);
/* Camera(): main.cpp:311-347, with the globals it reads (global_fov/yaw/pitch/shift,
 * screen_width/height: main.cpp:20-21,30-39) passed as arguments */
void pt_camera_init(pt_camera* c, float fov, float yaw, float pitch, const float shift[3],
                    int32_t width, int32_t height);
/* The side effect of the reference's Camera() (main.cpp:334-336): shift += ahead * forward + right * rightward + up * upward
 * along the rotated unit axes, in place -- what moves the camera when the key handlers (main.cpp:1189-1209) set the three
 * globals.  Call it before pt_camera_init, once per Camera() the reference would have constructed. */
void pt_camera_move(float shift[3], float yaw, float pitch, float forward, float rightward, float upward);

/* ---- context: Scene::init_Scene, main.cpp:456-528 --------------------------------- */
/* Selects HIP device `device`, allocates rays (32 B/px), rnds (4 B/px), colors (16 B/px)
 * and seeds rnds from std::minstd_rand0 in pixel order (main.cpp:508-527). */
int pt_create(int device, int32_t width, int32_t height, pt_context** out);
/* Multi-GPU variant: this context owns the rows r with (r / rows_per_block) % world == rank
 * of the global width x height frame.  Seeds and pixel ids stay those of the
 * GLOBAL frame, so the union of all ranks' pixels equals a 1-GPU render bit for bit. */
int pt_create_tiled(int device, int32_t width, int32_t height, int32_t rank, int32_t world,
                    int32_t rows_per_block, pt_context** out);
void pt_destroy(pt_context* ctx);
/* Message of the last failure on ctx (ctx == NULL: last failure of pt_create*). */
const char* pt_last_error(const pt_context* ctx);
/* Scene::list_info, main.cpp:389-455: one line describing the device into buf. */
int pt_device_info(const pt_context* ctx, char* buf, int32_t buflen);

/* ---- scene authoring: main.cpp:529-617 --------------------------------------------- */
int pt_add_material(pt_context* ctx, const pt_material* m);          /* Scene::add_Material: returns the index (>= 0) */
int pt_add_triangle(pt_context* ctx, const pt_triangle* t);          /* Scene::add_Triangle */
int pt_add_triangles(pt_context* ctx, const pt_triangle* t, int64_t n); /* n x add_Triangle */
int pt_end_obj(pt_context* ctx);                                     /* Scene::end_Obj: closes one object */
/* Scene::add_Obj(file,pos,scale,pitch,yaw), main.cpp:552-617: OBJ+MTL import with the
 * reference's conventions (x negated, rotate_x(pitch), rotate_y(yaw), scale, translate;
 * first three vertices of each face; MTL keys Kd Ks Ke Ns + custom Kn Kk Tp; one object
 * per shape). */
int pt_add_obj(pt_context* ctx, const char* file, const float pos[3], const float scale[3],
               float pitch, float yaw);
int pt_upload_triangles(pt_context* ctx);                            /* Scene::upload_Triangles, main.cpp:618-630 */
int pt_upload_materials(pt_context* ctx);                            /* Scene::upload_Materials, main.cpp:631-634 */

/* ---- RNG state: main.cpp:522-527 ---------------------------------------------------- */
int pt_seed_default(pt_context* ctx);                                /* re-seed from minstd_rand0 */
/* seeds[] holds one int per pixel of the GLOBAL frame (n = width*height) */
int pt_upload_seeds(pt_context* ctx, const int32_t* seeds, int64_t n);

/* ---- the hot path: main.cpp:635-687 -> prog.cl:384-389, 292-381 --------------------- */
int pt_generate_rays(pt_context* ctx, const pt_camera* cam);         /* Scene::generate_rays -> gen_ray */
int pt_trace_rays(pt_context* ctx, const pt_camera* cam, int32_t iterations, int32_t current_sample); /* Scene::trace_rays -> trace_ray */
/* nsamples x Scene::render(): for current_sample = s0 .. s0+nsamples-1 (s0 = the context's
 * sample counter, main.cpp:28) do generate_rays + trace_rays; the counter advances by
 * nsamples.  Fused on the device: one launch, path state in registers. */
int pt_render(pt_context* ctx, const pt_camera* cam, int32_t iterations, int32_t nsamples);
/* Adaptive frame: renders min_spp samples to every tile, then keeps doubling the sample count of the 8x8 tiles whose
 * noise estimate is still >= threshold, up to max_spp.  Starts a frame: current_sample must be 0.
 * Rounds: boundaries b0 = min_spp/2, b1 = min_spp, b(k+1) = min(2 b(k), max_spp) (pt_adaptive_rounds); round k renders
 * samples [b(k-1), b(k)) of the tiles still active.  After every b(k) with k >= 1 and b(k) < max_spp each pixel's mean M is
 * compared with its mean A at b(k-1) = b(k)/2 in float32, in this order: e = ((|M.r-A.r| + |M.g-A.g|) + |M.b-A.b|) /
 * (1e-4 + sqrt((M.r + M.g) + M.b)); a tile's estimate is the max over its pixels (+inf if any e is not finite) and the tile
 * retires iff it is < threshold, keeping its colours and LCG states.  A retired tile has the samples of the boundary it
 * retired at, the others max_spp; the call returns early when no tile is active, and current_sample is the largest count.
 * min_spp even and >= 2, max_spp >= min_spp, threshold >= 0 (0 retires nothing, +inf every tile with a finite estimate);
 * contexts of one rank (world 1) and variant 0 only, else PT_EINVAL.  Synchronises the stream once per round (the number of
 * active tiles comes back to the host).  Until pt_set_current_sample(ctx, 0) starts a new frame, pt_render, pt_trace_rays
 * and another pt_render_adaptive return PT_EINVAL. */
int pt_render_adaptive(pt_context* ctx, const pt_camera* cam, int32_t iterations,
                       int32_t min_spp, int32_t max_spp, float threshold);
/* The same frame with a choice of error measure and render path (new; pt_render_adaptive is {PT_ADAPT_HALF, PT_ADAPT_PATH_RENDER} and
 * is unchanged).  Rounds, boundaries, decisions after every b(k) with k >= 1 and b(k) < max_spp, one synchronisation per round, the
 * held frame, world 1, pt_read_sample_counts / pt_read_tile_state / pt_debug_adaptive_list, the "samples" statistic and the argument
 * checks are pt_render_adaptive's; params NULL, an unknown metric or path, or (path NEE) an unknown strategy give PT_EINVAL, all before
 * PT_ENODEVICE.
 * metric PT_ADAPT_HALF: the estimate above, max over the tile.
 * metric PT_ADAPT_VARIANCE: option "moments" must be 1 (else PT_EINVAL); no snapshot is kept.  At boundary b, float32, in this order:
 *   per pixel inside the frame  mu = l(colors.xyz), v = fmaxf(fmaf(-mu, mu, colors.w), 0) / (float)(b - 1)   (pt_read_variance at n = b)
 *   tonemapped != 0:            d = 1.0f + mu, v = v / ((d*d)*(d*d))      (the derivative of Reinhard's L / (1 + L), pt_resolve_ldr(0))
 *   lane (y&7)*8 + (x&7) of the tile's 64 holds v (0 outside the frame); for off = 32, 16, 8, 4, 2, 1: s[lane] = s[lane] + s[lane ^ off]
 *   e = sqrtf(s / (float)pixels inside), +inf if not finite; the tile retires iff e < threshold.
 *   The threshold is the tile's predicted root-mean-square error of the mean luminance (display-referred with tonemapped).
 * path PT_ADAPT_PATH_RENDER: rounds are pt_render's megakernel over the active tiles; PT_EINVAL while an environment is set and for
 *   variant != 0; strategy is ignored.
 * path PT_ADAPT_PATH_NEE: rounds render with pt_render_nee's estimator at `strategy` (PT_NEE_*), the environment included when one is
 *   set; a pixel that stopped after k samples holds what pt_render_nee(k) from sample 0 leaves in colors (.w too), rnds and rays.  Any
 *   variant; the 31-bit work-item check of the megakernel path does not apply. */
enum { PT_ADAPT_HALF = 0, PT_ADAPT_VARIANCE = 1 };          /* metric */
enum { PT_ADAPT_PATH_RENDER = 0, PT_ADAPT_PATH_NEE = 1 };   /* path   */
typedef struct { int32_t min_spp, max_spp; float threshold;
                 int32_t metric, path, strategy, tonemapped; } pt_adaptive_params;
/* min_spp 16, max_spp 1024, threshold 0.03, metric VARIANCE, path RENDER, strategy PT_NEE_MIS, tonemapped 1.  The threshold comes from
 * the {VARIANCE, RENDER, tonemapped 1} sweep of tools/adaptive_sweep.py at 1920x1080, 8 bounces (profiles/adaptive/README.md): the
 * largest value of the sweep whose display-referred RMSE stays near the one of max_spp -- Cornell box 0.0260 against 0.0215 with 0.73 of
 * the samples, MESH-100k (16..256) 0.0445 against 0.0433 with 0.86.  It saves neither samples nor wall time against uniform sampling at
 * equal error there; the one measured saving (25-30 % of the samples at equal RMSE, wall time about level) is tonemapped 0 with a
 * threshold on the linear scale, 0.05 to 0.15 in that sweep (same file). */
void pt_adaptive_defaults(pt_adaptive_params* p);
int pt_render_adaptive_ex(pt_context* ctx, const pt_camera* cam, int32_t iterations, const pt_adaptive_params* params);
/* per local pixel: the number of samples its colour is the mean of (0 for none yet) */
int pt_read_sample_counts(pt_context* ctx, int32_t* out, int64_t npix);
/* per 8x8 tile of the local frame (raster order): samples rendered, and the last noise estimate computed for it (+inf: none);
 * either pointer may be NULL */
int pt_read_tile_state(pt_context* ctx, int32_t* spp, float* err, int64_t n_tiles);
/* host only, no device: the sample-count boundaries pt_render_adaptive uses (min_spp/2, min_spp, 2*min_spp, ..., max_spp);
 * *count = their number, the first min(cap, *count) are written to out */
int pt_adaptive_rounds(int32_t min_spp, int32_t max_spp, int32_t* out, int32_t cap, int32_t* count);
int pt_set_current_sample(pt_context* ctx, int32_t current_sample);  /* main.cpp:1046 etc.: key events reset it to 0 */
int pt_get_current_sample(const pt_context* ctx, int32_t* out);
int pt_sync(pt_context* ctx);                                        /* queue.finish(), main.cpp:675 */

/* ---- readback (the reference never reads back; its only output is a GL texture) ----- */
int pt_local_pixel_count(const pt_context* ctx, int64_t* out);
int pt_local_pixel_ids(const pt_context* ctx, int32_t* out_ids, int64_t n);  /* global pixel id of each local pixel */
int pt_slab_pixel_count(const pt_context* ctx, int64_t* out);       /* max over ranks of the local pixel count */
int pt_read_colors(pt_context* ctx, float* out_rgba, int64_t npix);  /* buffer_colors: float3 @ 16 B stride */
int pt_read_rnds(pt_context* ctx, int32_t* out, int64_t npix);       /* buffer_rnds */
int pt_read_rays(pt_context* ctx, pt_ray* out, int64_t npix);        /* buffer_rays */
/* reinhard_tone_map + sRGB of colors (prog.cl:247-269, the value write_imagef stores at
 * prog.cl:380); which = 0 Reinhard, 1 = filt_im (3x3 median + filmic, prog.cl:391-427). */
int pt_resolve_ldr(pt_context* ctx, int32_t which, float* out_rgba, int64_t npix);

/* ---- next-event estimation with multiple importance sampling (new: opt-in; pt_render is unchanged) -------------------
 * The estimator of pt_render (prog.cl:292-389), per sample: a lobe vertex (type 0 diffuse, type 3 emitter) draws w with
 * pdf p_b(w) = max(0, N.w) / pi (two LCG values); type 0 then does fL *= kd max(0, N.w), fB *= ks pow(max(0, N.h), shininess)
 * with h = normalize(normalize(eye - x) + w) (the CAMERA eye), type 3 leaves the factors; an emitter hit at y adds
 * E (fL + fB) fS fR |cos_y|; types 1 / 2 change fS / fR only; iterations segments; iterations == 1 is the flat preview.
 * pt_render_nee keeps that LCG stream draw for draw -- rnds and rays after a frame are pt_render's in every strategy -- and
 * adds, at a lobe vertex x of segment k with k + 1 < iterations, a light sample:
 *   u0, u1, u2 = pt_nee_rand(S, k, 0 / 1 / 2) >> 8 times 2^-24, S = the pixel's LCG state at the start of the sample;
 *   light j = the first index with cdf[j] > u0 (pt_debug_light_table), su = sqrt(u1),
 *   y = r1 + (r2 - r1) (u2 su) + (r3 - r1) (su (1 - u2)) on that triangle;
 *   o = x + 0.001 N (the origin the BSDF ray uses), d = y - o, r = |d|, w = d / r;
 *   y is visible iff the closest hit of (o, w) with the search cut at 1.0001 r is that triangle;
 *   p_b = max(0, N.w) / pi, p_l = (P_sel / area)(tri) r^2 / |cos_y|, both > 0 or no contribution;
 *   contribution = E_y (fL' + fB') fS fR |cos_y| times W_l, fL' / fB' = the factors x's own update with w would give;
 * and every emitter hit on segment k + 1 after a lobe vertex x on segment k (BSDF-sampled, p_b from x's normal and the
 * ray, p_l with r = the hit distance from x's offset origin and P_sel / area of the hit triangle, 0 for a non-light) has
 * its addition times W_b.  A hit seen from the camera or through mirror / glass vertices only keeps W_b = 1.
 *   PT_NEE_BSDF   W_b = 1, no light sample: exactly pt_render's estimator (same bits)
 *   PT_NEE_LIGHT  W_b = 0 if p_l > 0 else 1,          W_l = p_b / p_l
 *   PT_NEE_MIS    W_b = p_b^2 / (p_b^2 + p_l^2),      W_l = p_b p_l / (p_b^2 + p_l^2)   (power heuristic; W_l includes p_b / p_l)
 * All three have pt_render's expectation.  Light table (built on the host at the first pt_render_nee after an upload): the
 * packed triangles of type-3 material with E.r + E.g + E.b > 0 and non-zero area (in packed order), cdf in float (last entry 1)
 * proportional to the running sum of area (E.r + E.g + E.b); P_sel in p_l and in the weights is the probability the 24-bit u0
 * actually picks the light with: (ceil(cdf[j] 2^24) - ceil(cdf[j-1] 2^24)) / 2^24 (0: never picked, p_l = 0 for its hits).
 * No lights: every strategy is PT_NEE_BSDF.
 * Same rules as pt_render: argument checks (iterations >= 0, nsamples >= 0, strategy 0..2, else PT_EINVAL), advances
 * current_sample by nsamples, running mean into colors (or the bound framebuffer), refused while an adaptive frame is held,
 * any rank of a tiled frame, any variant (one launch of k_nee, pt_nee.hip). */
#define PT_NEE_BSDF 0
#define PT_NEE_LIGHT 1
#define PT_NEE_MIS 2
int pt_render_nee(pt_context* ctx, const pt_camera* cam, int32_t iterations, int32_t nsamples, int32_t strategy);
/* lowbias32(x) = x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15, x *= 0x846ca68b, x ^= x >> 16;
 * pt_nee_rand(state, segment, dim) = lowbias32(lowbias32(state) + 0x9e3779b9 * (3 segment + dim + 1)) (uint32 arithmetic) */
uint32_t pt_nee_rand(uint32_t state, int32_t segment, int32_t dim);
/* the light table (host only, any context with triangles and materials uploaded): *n = lights; the first min(cap, *n) of
 * orig_tri (add-order triangle index) and cdf are written (either may be NULL) */
int pt_debug_light_table(pt_context* ctx, int32_t* orig_tri, float* cdf, int64_t cap, int64_t* n);

/* ---- environment lighting for pt_render_nee (new: the reference's sky terms, prog.cl:367-376, are commented out) -----------
 * A lat-long map lights the scene from infinity.  Only pt_render_nee draws it; without one (or with an all-zero one) pt_render_nee
 * computes exactly what it computed before.
 * Map and lookup: w x h texels of float RGB, row 0 touches the +y pole (y is up).  For a unit direction d, in float32:
 *   theta = acosf(clamp(d.y, -1, 1)), phi = atan2f(d.z, d.x) - yaw (yaw = yaw_degrees pi / 180, rounded to float);
 *   row = min(h - 1, floor(theta / pi * h)); col = min(w - 1, floor(frac(phi / (2 pi)) * w)), frac(x) = x - floor(x);
 *   nearest texel (the map is piecewise constant); E(d) = scale * texel.  A 1 x 1 map is a constant sky.
 * A miss on segment k along D ends the path as before and adds
 *   k = 0: E(D) (prog.cl:369: no factor of two for a sky seen directly; iterations == 1, the flat preview, shows E(D));
 *   k > 0: W_b E(D) (fL + fB) fS fR (prog.cl:371-373), W_b = 1 unless the previous vertex was a lobe vertex (below).
 * Distribution: piecewise constant over texels with weight lum(texel) Omega(row), lum = the luminance of option "moments",
 *   Omega(row) = (2 pi / w)(cos theta_row - cos theta_row+1), theta_row = pi row / h.  The host builds the row marginal cdf [h] and
 *   the per-row column cdfs [h][w] in double and stores them as float (last entries 1; a row of weight 0 gets a uniform column cdf and
 *   is never picked).  u1 picks the first row with row_cdf > u1, t1 = (u1 - below) / (row_cdf[row] - below) is the position inside
 *   it: cos theta = cos theta_row - t1 (cos theta_row - cos theta_row+1); u2 picks the column the same way, phi = 2 pi (col + t2) / w
 *   + yaw; w = (sin theta cos phi, cos theta, sin theta sin phi): uniform in solid angle inside the texel.
 *   p_env(d) = P(texel) / Omega(row), P(texel) = the product of the two stored float cdfs' own steps (computed in double, stored as
 *   float next to the texel).  A map whose weights are all 0 has no distribution.
 * At a lobe vertex x of segment k with k + 1 < iterations, strategies LIGHT and MIS:
 *   u_sel = pt_nee_rand(~S, k, 0) >> 8 times 2^-24 (the complemented key: dimension 3 of S would be the next segment's dimension 0);
 *   u_sel < P_env: the sky, direction from u1, u2 as above (u0 is not used); else the light table with u0, u1, u2 as before.
 *   P_env = ceil(select 2^24) / 2^24; 1 when the light table is empty; 0 when the map has no distribution.
 *   Triangle pdfs become (1 - P_env) (P_sel / area) r^2 / |cos_y| (in the weights of emitter hits too); p_l(sky) = P_env p_env(w).
 *   Sky sample: o = x + 0.001 N; rejected unless N.w > 0 and p_l > 0; visible iff no triangle is hit from o along w at any distance;
 *   adds E (fL' + fB') fS fR W_l, E the sampled texel's value (no second lookup), p_b = max(0, N.w) / pi, W_l from the strategy table.
 *   A miss after a lobe vertex: W_b from the strategy table with p_l = P_env p_env(D), p_b from that vertex's normal.
 * PT_NEE_BSDF: W_b = 1, no light samples.  All three strategies have the same expectation; rnds and rays are pt_render's.
 * While an environment is set (an all-zero one too) pt_render, pt_generate_rays, pt_trace_rays and pt_render_adaptive return
 * PT_EINVAL naming pt_render_nee; after pt_clear_environment they render what they rendered before.  pt_upload_triangles /
 * pt_upload_materials keep the map.  Every rank of a tiled frame sets its own copy. */
typedef struct { float scale, yaw_degrees, select; } pt_environment_params;
#define PT_ENV_MAX_WIDTH 4096
#define PT_ENV_MAX_HEIGHT 2048
void pt_environment_defaults(pt_environment_params* p);              /* scale 1, yaw_degrees 0, select 0.5 */
/* rgb: w x h x 3 floats, row 0 at the +y pole; p = NULL: the defaults.  Copies the map, builds the tables on the host (works on a
 * host-only context) and uploads them on a device context.  PT_EINVAL: a NaN, infinite or negative texel, w or h < 1 or above
 * PT_ENV_MAX_*, select outside [0, 1], a non-finite or negative scale, a non-finite yaw_degrees */
int pt_set_environment(pt_context* ctx, const float* rgb, int32_t w, int32_t h, const pt_environment_params* p);
int pt_clear_environment(pt_context* ctx);
/* host only: the texel of unit direction dir[3] (the mapping above, the code the kernel runs) */
int pt_env_lookup(int32_t w, int32_t h, float yaw_degrees, const float dir[3], int32_t* row, int32_t* col);
/* the tables the kernel samples (host data): *w, *h the map's size; row_cdf: min(cap, h) entries; col_cdf and pdf (p_env per texel):
 * min(cap, w h) entries, row-major; *P_env the effective value (the light table is built if the scene is uploaded, else taken as empty).
 * Any pointer may be NULL.  PT_EINVAL when no environment is set */
int pt_debug_environment(pt_context* ctx, int32_t* w, int32_t* h, float* row_cdf, float* col_cdf, float* pdf, int64_t cap, float* P_env);

/* ---- point, spot and directional lights for pt_render_nee (new: opt-in with pt_set_lights; the reference lights with emitters only) ----
 * A set of analytic ("delta") lights lights the scene through light samples only.  Only pt_render_nee and the NEE path of
 * pt_render_adaptive_ex draw them.  Without a set -- never set, cleared, count 0, or every light black -- every path launches the kernels
 * it launched before and computes what it computed before, bit for bit.  Everything below is stated in the reference's integrand, as the
 * estimator of pt_render_nee is: p_b and the primed factors are what a light sample of that block computes for each vertex type (0, with
 * a texture; 3; 4; 5; 6 on the reflection lobe only).
 * Set: a light's selection weight is `weight`, or intensity.r + intensity.g + intensity.b when weight is 0; a light whose weight is
 *   still 0 (black) stays in the set but is never picked.  The host normalises direction in double and stores floats; the cdf over the
 *   set is float, proportional to the running sum of the weights (summed and normalised in double; 1 from the last pickable light on);
 *   P_light(j) = (ceil(cdf[j] 2^24) - ceil(cdf[j-1] 2^24)) / 2^24, the share of the 2^24 values of u0 that pick light j (the counting
 *   rule of the light table).  A set has a pickable light iff some P_light > 0.
 * Selection, at a lobe vertex x of segment k with k + 1 < iterations, strategies LIGHT and MIS, while the set has a pickable light:
 *   u_ana = pt_nee_rand(~S, k, 2) >> 8 times 2^-24 (dimensions 0 and 1 of the complemented key are the sky's and the coat / frost lobe's
 *   selectors); u_ana < P_ana: the analytic set; else the sky / light-table sample as before, its p_l times 1 - P_ana (in the weights
 *   W_b of emitter hits and sky misses after a lobe vertex too).
 *   P_ana = ceil(select 2^24) / 2^24; 1 when the light table is empty and no environment with a distribution is set; 0 when no light
 *   is pickable.
 *   Inside the set u0 = pt_nee_rand(S, k, 0) (the triangle draw, which this branch does not use) picks the first light with cdf > u0.
 * Sample: o = x + 0.001 Ng' (the origin every light sample uses).
 *   POINT: d = P - o, r^2 = d.d, rejected unless r^2 > 0 and finite; r = sqrtf(r^2), w = d / r; visible iff no triangle is hit from o
 *     along w nearer than exactly r.
 *   DIRECTIONAL: w = -direction (unit); visible iff no triangle is hit from o along w at any distance.
 *   Rejected unless N.w > 0 (under "smooth_normals": unless it is also above the geometric surface).
 *   Cone: c = dot(-w, axis); 1 if c >= cos_inner; else 0 if c <= cos_outer; else s^2 (3 - 2 s), s = (c - cos_outer) / (cos_inner -
 *     cos_outer), tested in that order.  cos_outer = -1 is "no cone": direction and cos_inner are then not read (the factor is 1), and a
 *     directional light has none.
 *   Adds intensity cone (fL' + fB') fS' fR' p_b(w) / (P_ana P_light d), d = r^2 (POINT) or 1 (DIRECTIONAL): the weight of a delta-light
 *     sample is p_b / p_l in PT_NEE_LIGHT and in PT_NEE_MIS, because no other strategy can find the light.
 *   POINT intensity is radiant intensity I (what an emitter's E x area x |cos_y| is at a distance), DIRECTIONAL intensity the irradiance
 *   E_perp on a surface facing the light.  In the reference's integrand a diffuse floor facing the light shows kd E_perp / pi, and
 *   kd I cos^2 / (pi r^2) under a point light (the second cosine is p_b's).
 * No LCG draw is added: rnds and rays after a frame are pt_render's.  The lights are not visible to the camera or through specular
 * chains; the guides, the denoisers, the variance read-out and temporal accumulation are not affected.
 * While a set with a pickable light is held, pt_render, pt_generate_rays, pt_trace_rays, pt_render_adaptive, pt_render_nee with
 * PT_NEE_BSDF (which is pt_render bit for bit and would drop the lights) and pt_render_adaptive_ex with PT_ADAPT_PATH_RENDER or with
 * strategy PT_NEE_BSDF return PT_EINVAL naming pt_clear_lights, checked before the device.
 * The set lives in the context: pt_upload_triangles / pt_upload_materials keep it (P_ana is worked out at each launch from the light
 * table of the scene as uploaded), every rank of a tiled frame sets its own copy, a host-only context validates and stores. */
#define PT_LIGHT_POINT 0        /* also the spot light: a point light with a cone */
#define PT_LIGHT_DIRECTIONAL 1
#define PT_LIGHTS_MAX 4096
typedef struct {
    int32_t type;
    float position[3];          /* POINT: where it is (scene coordinates, as triangles are added) */
    float direction[3];         /* POINT: the cone's axis, the way the light points (read only when cos_outer > -1);
                                   DIRECTIONAL: the way the light travels.  Need not be unit, must be non-zero where read */
    float intensity[3];         /* POINT: radiant intensity I (what an emitter's E x area x |cos| is at a distance);
                                   DIRECTIONAL: irradiance E_perp on a surface facing the light */
    float cos_inner, cos_outer; /* POINT: full strength inside cos_inner, nothing outside cos_outer; -1, -1 = no cone */
    float weight;               /* selection weight; 0 = automatic: intensity r + g + b */
} pt_light;
typedef struct { float select; } pt_lights_params;      /* pt_lights_defaults: select = 0.5 */
void pt_lights_defaults(pt_lights_params* p);
/* Replaces the whole set (count == 0 is pt_clear_lights); p = NULL: the defaults.  A device context uploads the records; PT_EHIP if
 * that fails, and the context then holds no set.  PT_EINVAL, with the set left as it was: lights NULL
 * with count > 0, count < 0 or above PT_LIGHTS_MAX, select outside [0, 1], an unknown type, a non-finite field, a negative intensity,
 * a negative weight, cos_inner / cos_outer not ordered -1 <= cos_outer <= cos_inner <= 1, a zero direction where it is read */
int pt_set_lights(pt_context* ctx, const pt_light* lights, int32_t count, const pt_lights_params* p);
int pt_clear_lights(pt_context* ctx);
/* what the kernel samples (host data): *n = lights in the set; for the first min(cap, *n) lights, records = 16 floats each as uploaded
 * ({position.xyz, type as int32 bits}, {axis.xyz, cos_inner}, {intensity.rgb, cos_outer}, {P_light, 0, 0, 0}; axis unit, or 0 where it is
 * not read; cos -1, -1 for a directional light), cdf and P_light one float each; *P_ana the effective value for the scene as uploaded
 * (the light table is built if the scene is uploaded, else taken as empty).  Any pointer but n may be NULL */
int pt_debug_lights(pt_context* ctx, float* records, float* cdf, float* P_light, int64_t cap, int64_t* n, float* P_ana);

/* ---- sphere lights and suns with an angular size for pt_render_nee (new: opt-in with pt_set_area_lights) ----
 * A set of area lights: spheres of uniform radiance L that emit outwards, and suns, discs of angular radius a at infinity.  Unlike the
 * analytic lights above they have an extent: their shadows are soft, the camera, mirrors and glass see them, and the BSDF strategy finds
 * them, so they are balanced against it under MIS like triangle lights.  Only pt_render_nee (every strategy, PT_NEE_BSDF included) and the
 * NEE path of pt_render_adaptive_ex draw them.  Without a set -- never set, cleared, count 0, or every light black -- every path launches
 * the kernels it launched before and computes what it computed before, bit for bit.  Stated in the reference's integrand, as the estimator
 * of pt_render_nee is: a lobe vertex adds radiance x (fL' + fB') fS' fR' and does not divide by p_b.
 * Table: spheres are sorted before suns (stable).  A light's selection weight is `weight`, or when that is 0 (r + g + b) 4 pi^2 R^2 for a
 *   sphere (its power) and (r + g + b) 2 pi (1 - cos a) for a sun (its irradiance), in double.  The cdf is float, proportional to the
 *   running weight (1 from the last pickable light on); P_light(j) = (ceil(cdf[j] 2^24) - ceil(cdf[j-1] 2^24)) / 2^24, the counting rule
 *   of the light table.  A black light stays in the set and is never picked.  The host stores, per sun, the unit axis -direction
 *   (normalised in double), cos a and q = 2 sin^2(a / 2), each computed in double and rounded to float.
 * Selection, at a lobe vertex and at a scatter vertex of the medium, on segment k with k + 1 < iterations, strategies LIGHT and MIS:
 *   u_area = pt_nee_rand(S ^ PT_AREA_KEY, k, 0) >> 8 times 2^-24.  u_area < P_area: the area set is sampled.  Otherwise everything happens
 *   that happened before, with every p_l times 1 - P_area: in the analytic, sky, light-table and light-tree samples, and in W_b of emitter
 *   hits and sky misses.  P_area = ceil(select 2^24) / 2^24; 1 when nothing else is pickable (an empty light table, no environment with a
 *   distribution, no pickable analytic light); 0 when no area light is pickable.  Inside the set u0 = pt_nee_rand(S, k, 0) picks the first
 *   light with cdf > u0, and u1, u2 (dimensions 1, 2 of S) place the sample.  Nothing is drawn from the LCG.
 * Sphere sample from o (the offset origin every light sample uses; a scatter vertex itself): c = C - o, d^2 = c.c; rejected unless d^2
 *   is finite and d^2 > R^2 (a sphere is transparent from inside).  s^2 = R^2 / d^2, cos_m = sqrt(max(0, 1 - s^2)), q = s^2 / (1 + cos_m)
 *   (= 1 - cos_m without cancellation).  cos t = 1 - u1 q, sin t = sqrt(max(0, 1 - cos^2 t)), phi = 2 pi u2;
 *   w = A cos t + Z sin t sin phi + X sin t cos phi in the frame (Z, X) of A = normalize(c) that the cosine-lobe sampler builds
 *   (prog.cl:205-212; w is not renormalised).  p_omega = 1 / (2 pi q), p_l = P_area P_light p_omega.  The cut is
 *   t_s = b - sqrt(max(0, b^2 - (d^2 - R^2))), b = c.w.  Rejected unless N.w > 0 (and above the geometric surface under smooth_normals); a
 *   scatter vertex of the medium tests no cosine.
 * Sun sample: the same cone around the stored axis with the stored q; no cut.
 * Visibility: an area sphere is opaque on the NEE path.  A sample of sphere j counts iff no triangle is hit nearer than t_s and no other
 *   sphere of the set whose outside holds o is met before t_s (sphere i is met at t_i = b_i - sqrt(b_i^2 - (d_i^2 - R_i^2)) when that
 *   discriminant is >= 0 and t_i > 0).  Every other shadow ray of the path -- triangle-light, sky, analytic-light and sun samples -- is
 *   blocked by a sphere met before its own limit as well.  Suns occlude nothing.
 * Contribution: L (fL' + fB') fS' fR' T W_l, T the transmittance the shadow ray takes in a medium; W_l = p_b / p_l in LIGHT,
 *   p_b p_l / (p_b^2 + p_l^2) in MIS (the power heuristic of the triangle lights).
 * BSDF side: after the closest-hit search of a segment from P along D returned t_tri (+inf on a miss), the nearest sphere with P outside it
 *   and 0 < t_i < t_tri ends the segment in the triangle's place, before the free flight of a medium or an interior looks at the segment's
 *   length.  A segment that reaches the sphere ends the path: on segment 0 it adds L; else L (fL + fB) fS fR W_b (no |cos_y|; the form of a
 *   sky miss), W_b = 1 unless the previous vertex was a lobe vertex in LIGHT or MIS: then 0 in LIGHT when p_l > 0 and p_b^2 / (p_b^2 +
 *   p_l^2) in MIS, p_l the sphere's density seen from P.  On a miss every sun with dot(D, axis) >= cos a adds its L likewise, each with
 *   its own W_b; then the sky adds as before.
 *   A segment inside a dielectric (between a refraction in and the boundary it would leave through) is cut by a sphere light in the same
 *   way: the interior bound to that boundary's material absorbs and scatters over the cut length.  Spheres are not clipped against
 *   objects; one that overlaps a bound object shines inside it.
 * A path that ends on a sphere makes no further LCG draw: rnds and rays after a frame are pt_render's for paths that meet no sphere.
 * PT_NEE_BSDF takes no light sample and has W_b = 1; it is allowed with an area set (and still refused while a delta set is held).
 * While a set with a pickable light is held, pt_render, pt_generate_rays, pt_trace_rays, pt_render_adaptive and pt_render_adaptive_ex with
 * PT_ADAPT_PATH_RENDER return PT_EINVAL naming pt_clear_area_lights, checked before the device.
 * Guides: with option "aov_lights" = 1 pt_render_aovs and pt_render_aovs_ex see the set -- a sphere light ends a chain of the guide pass
 * exactly where it ends a segment here (the same device function, area_sphere_hit), a miss takes the suns whose disc holds the direction
 * (area_sun_mask) -- so the denoisers and temporal accumulation, which read the guides, treat a visible lamp as a surface of its own (the
 * lit guides are pinned with the guide buffers below).  pt_set_area_lights and pt_clear_area_lights make lit guides stale.  With the option
 * off (the default) the guides keep the view without the lights.  The despeckle stage (pt_despeckle) reads no guides and is what it was.
 * The set lives in the context like the analytic set: uploads keep it, every rank of a tiled frame sets its own copy, a host-only context
 * validates and stores. */
#define PT_AREA_LIGHT_SPHERE 0
#define PT_AREA_LIGHT_SUN 1
#define PT_AREA_LIGHTS_MAX 64   /* small on purpose: every path segment tests every sphere */
#define PT_AREA_KEY 0x9e3779b9u /* u_area's key is S ^ PT_AREA_KEY (taken: S, ~S, S ^ 0x5bd1e995) */
typedef struct {
    int32_t type;
    float position[3];          /* SPHERE: the centre */
    float direction[3];         /* SUN: the way the light travels.  Need not be unit, must be non-zero */
    float radiance[3];          /* the uniform emitted radiance L */
    float size;                 /* SPHERE: the radius, > 0; SUN: the angular radius a in radians, 0 < a <= pi / 2 */
    float weight;               /* selection weight; 0 = automatic (see above) */
} pt_area_light;                /* 48 bytes */
typedef struct { float select; } pt_area_lights_params;      /* pt_area_lights_defaults: select = 0.5 */
void pt_area_lights_defaults(pt_area_lights_params* p);
/* Replaces the whole set (count == 0 is pt_clear_area_lights); p = NULL: the defaults.  A device context uploads the records; PT_EHIP if
 * that fails, and the context then holds no set (as pt_set_lights).  PT_EINVAL, with the set left as it was, in this
 * order: lights NULL with count > 0 (after count < 0 or above PT_AREA_LIGHTS_MAX), select outside [0, 1], then per light an unknown
 * type, a non-finite field, a negative radiance, a negative weight, a size outside its range, a zero direction of a sun */
int pt_set_area_lights(pt_context* ctx, const pt_area_light* lights, int32_t count, const pt_area_lights_params* p);
int pt_clear_area_lights(pt_context* ctx);
/* what the kernel samples (host data): *n = lights in the set; for the first min(cap, *n) lights in table order, records = 12 floats each
 * as uploaded (sphere {C.xyz, R} {L.rgb, P_light} {0, 0, 0, 0}; sun {axis.xyz, cos a} {L.rgb, P_light} {q, 0, 0, 0}), order = the light's
 * index in the array that was set, cdf and P_light; *n_sphere the number of spheres; *P_area the effective value for the scene as
 * uploaded.  Any pointer but n may be NULL */
int pt_debug_area_lights(pt_context* ctx, float* records, int32_t* order, float* cdf, float* P_light, int64_t cap, int64_t* n, int32_t* n_sphere,
                         float* P_area);
typedef struct {
    float w[3];         /* the sampled direction */
    float p_omega;      /* its density over solid angle */
    float t_s;          /* the cut (+inf for a sun) */
    int32_t accept;     /* 0: rejected (the origin is not outside the sphere); w, p_omega, t_s are then 0, 0, +inf */
} pt_area_light_sample; /* 24 bytes */
typedef struct {
    int32_t sphere;     /* the nearest sphere (table order) in front of t_max, or -1 */
    float t;            /* its distance (t_max when none) */
    uint32_t suns[2];   /* bit s of the 64: sun number s (table order minus the number of spheres) holds the direction in its disc */
} pt_area_light_hit;    /* 16 bytes */
/* the device's sample and hit functions on given numbers (k_debug_area_light, which calls what the area-light instances of k_nee call;
 * a device context with a set held).  Samples: origins (3 floats each), lights (table order), u (u1, u2 each, in [0, 1)).  Hits: rays, 7
 * floats each {origin, unit direction, t_max}.  Either count may be 0 */
int pt_debug_area_light_eval(pt_context* ctx, const float* origins, const int32_t* lights, const float* u, int64_t n_samples, pt_area_light_sample* samples,
                             const float* rays, int64_t n_hits, pt_area_light_hit* hits);

/* ---- a homogeneous participating medium (fog) for pt_render_nee (new: opt-in with pt_set_medium; the reference renders vacuum) ----
 * One medium per context, set like the lens and the environment; it is not part of the scene, so uploads keep it.  Only pt_render_nee
 * (every strategy) and the NEE path of pt_render_adaptive_ex render it.  Without one -- never set, cleared, or sigma_t = 0 -- every path
 * launches the kernels it launched before and computes what it computed before, bit for bit.
 * The medium fills its axis-aligned box [lo, hi] wherever the path is not inside a dielectric (the `inside` flag of the specular and frosted
 * vertices is false).  (Inside one, the interior bound to its material applies instead: pt_set_material_interior below.)  It draws from a third hash stream, pt_nee_rand(S ^ 0x5bd1e995, k, dim) (S the LCG state at the start of the sample,
 * k the segment; the light samples own S and ~S), never from the LCG: rnds after a frame are pt_render's for every path that never scatters.
 * All arithmetic below is float32 with no contraction; log1pf, expf, sinf, cosf are the device library's (OCML: within 2 ulp, 1 ulp, 2 ulp,
 * 2 ulp), divides and square roots IEEE.
 * Clip(P, D, t): the part [a, b] of [0, t] inside the box, by slabs: a = 0, b = t; per axis x, y, z with i = 1 / D.axis: if |i| is finite,
 *   t0 = (lo - P) i, t1 = (hi - P) i, a = max(a, min(t0, t1)), b = min(b, max(t0, t1)) (max(a, v): v > a ? v : a; min(b, v): v < b ? v : b);
 *   else (the ray is parallel to the slab) b = -inf unless lo <= P <= hi.  L = max(b - a, 0) (0 for every NaN).
 * Free flight on segment k, after the closest hit (t its distance, +inf on a miss), while not inside a dielectric: [a, b] = Clip(P, D, t);
 *   if L > 0: u = (pt_nee_rand(S ^ 0x5bd1e995, k, 0) >> 8) 2^-24, d = -log1pf(-u) / sigma_t (-log(1 - u) with its relative precision kept for a small u); the segment scatters iff d < L, at distance
 *   s = a + d, x = fma(D, s, P) per component.  Otherwise the surface hit (or the miss) proceeds as without a medium, with no factor:
 *   surviving has probability exp(-sigma_t L), which is the transmittance, so the two cancel.
 * Scatter vertex (it consumes segment k as a surface vertex does):
 *   1 factor_S *= albedo; an all-zero product ends the path.
 *   2 with strategy LIGHT or MIS and k + 1 < iterations, one light sample as at a lobe vertex: the same three-way selection (analytic set,
 *     sky, light table), the same hash values of S and ~S at segment k; origin x itself (no offset), no cosine test at the vertex,
 *     p_b = HG(g, dot(D, w)); the factors are those after step 1; p_l, the emitter's cosine, the delta rule and the weight q / (q^2 + 1)
 *     (q = p_b / p_l; q alone for LIGHT and for a delta light) as at a surface vertex; times the transmittance T below.
 *   3 new direction: u1, u2 from dimensions 1 and 2 of the medium's stream; c = 1 - 2 u1 when |g| < 1e-3, else
 *     r = (1 - g g) / ((1 - g) + (2 g) u1), c = ((1 + g g) - r r) / (2 g); s = sqrtf(max(1 - c c, 0)), phi = 6.2831855f u2;
 *     w = X (s cosf(phi)) + Z (s sinf(phi)) + D c in the tangent frame (Z, X) of D that the diffuse vertex builds around its normal,
 *     normalised as every new direction is; the next segment starts at x.  The vertex is a lobe vertex for what follows: an emitter hit or
 *     a sky miss on segment k + 1 is weighted with p_b = HG(g, c).
 *     HG(g, c) = (1 - g g) / (12.566371f (q sqrtf(q))), q = (1 + g g) - (2 g) c.
 *   4 no emission; `inside` is unchanged.  With iterations = 1 a frame is the flat preview of the surface, and a sample that scatters is black.
 * Transmittance: every light sample whose vertex is not inside a dielectric -- at surface lobe vertices and at scatter vertices -- is
 *   multiplied by T = expf(-(sigma_t l)), l = the L of Clip(o, w, limit) for the shadow ray's origin o, direction w and cut `limit`
 *   (T = 1 exactly when l = 0).  limit is +inf for the sky and for directional lights: an unbounded medium gives those T = 0, so give the
 *   fog a box to let a sun in.  The weights of emitter hits and sky misses stay functions of the directional densities p_b and p_l only:
 *   both strategies carry the same transmittance along a direction -- the BSDF strategy as the probability of surviving the free flight,
 *   the light strategy as the factor T -- so it cancels in the balance and the weights still sum to one per direction.
 * With PT_NEE_BSDF the medium scatters and no light sample is taken.  A scatter vertex draws nothing from the LCG, so a path that scatters
 * ends with other rnds than pt_render's.  The guides (pt_render_aovs*), the denoisers and temporal accumulation keep the fog-free view, as
 * they keep the pinhole view under a lens.
 * While a medium with sigma_t > 0 is held, pt_render, pt_generate_rays, pt_trace_rays, pt_render_adaptive and pt_render_adaptive_ex with
 * PT_ADAPT_PATH_RENDER return PT_EINVAL naming pt_clear_medium, checked before the device.  Every rank of a tiled frame sets its own copy;
 * a host-only context validates and stores. */
typedef struct pt_medium {
    float sigma_t;      /* extinction per unit length, finite, >= 0; 0: no medium */
    float albedo[3];    /* single-scattering albedo, each in [0, 1] */
    float g;            /* Henyey-Greenstein asymmetry, |g| <= 0.99 */
    float lo[3], hi[3]; /* axis-aligned bounds; -inf / +inf: unbounded on that side; lo < hi on every axis */
} pt_medium;            /* 44 bytes */
void pt_medium_defaults(pt_medium* m);      /* {0, {1, 1, 1}, 0, {-inf, -inf, -inf}, {+inf, +inf, +inf}} */
/* PT_EINVAL, naming pt_set_medium and the field, with the held medium left as it was: a NaN anywhere, sigma_t negative or infinite, an
 * albedo outside [0, 1], |g| > 0.99, lo >= hi on an axis; ctx or m NULL */
int pt_set_medium(pt_context* ctx, const pt_medium* m);
int pt_clear_medium(pt_context* ctx);
/* the held record into *m (the defaults when none is held); returns 1 if one is held, 0 if not, PT_EINVAL for a NULL argument */
int pt_get_medium(const pt_context* ctx, pt_medium* m);
/* the device functions of the held medium (sigma_t > 0) on given numbers, n items: in, 12 floats each {P.xyz, D.xyz (unit), t, u, u1, u2,
 * limit, spare}; out, 10 floats each {a, b of Clip(P, D, t), 1 if d < L else 0, d = -log1pf(-u) / sigma_t, the new direction from
 * (u1, u2) around D (unit), its p_b, T of Clip(P, D, limit), 0}.  PT_EINVAL when no medium with sigma_t > 0 is held */
int pt_debug_medium(pt_context* ctx, const float* in, int64_t n, float* out);

/* ---- a voxel density grid for the medium (new: opt-in with pt_set_medium_density; smoke, clouds, mist that thins with height) ----
 * nx x ny x nz equal cells of the medium's box [lo, hi]; voxel (i, j, k), i along x, holds density[(k ny + j) nx + i], and the extinction
 * at a point of it is sigma_t x density[voxel]; the albedo and g stay pt_medium's.  The grid is kept as float32 in the context like the
 * medium -- uploads keep it, every rank of a tiled frame sets its own copy, a host-only context validates and stores -- and is live only
 * while a medium with sigma_t > 0 is held too.  Live, pt_render_nee and the NEE path of pt_render_adaptive_ex launch the grid instances
 * of k_nee (stat "nee_family" 9), and return PT_EINVAL naming the bound when lo or hi is infinite on an axis, checked before the device.
 * pt_clear_medium_density restores the homogeneous medium bit for bit.  The guides, the denoisers and temporal accumulation keep the
 * medium-free view, and the other render paths refuse as they do for any medium with sigma_t > 0.
 * The estimator is that of pt_set_medium above with the free flight and the transmittance replaced by a walk; the streams and their
 * dimensions, steps 1-4 of the scatter vertex, the `inside` rule and the weights are unchanged.  All float32, no contraction:
 * cell = (hi - lo) / (float)n and icell = (float)n / (hi - lo) per axis (IEEE divides, computed once when the launch is prepared).
 * Walk(P, D, t, tau): [a, b] = Clip(P, D, t); nothing to do unless L = max(b - a, 0) > 0.  t_cur = a, acc = 0.  Per axis, with i = 1 / D.axis
 *   (Clip's): the index is floorf((fma(D.axis, a, P.axis) - lo) icell), raised to 0 where it is not above 0 (a NaN too) and lowered to
 *   n - 1 where it is not below; if |i| is finite: step = +1 for i > 0 else -1, kb = index + (1 for i > 0 else 0), the plane is hi when
 *   kb = n else lo + (float)kb cell, tnext = (plane - P.axis) i, tdelta = cell |i|; else the axis never steps: tnext = +inf.
 *   Then at most nx + ny + nz + 3 times (a counted loop: termination does not depend on rounding):
 *     rho = density[(k ny + j) nx + i], sigma = sigma_t rho, t_exit = min(min(min(tnext_x, tnext_y), tnext_z), b) (min(p, q): q < p ? q : p),
 *     seg = max(t_exit - t_cur, 0);
 *     if sigma > 0: d = (tau - acc) / sigma, and the walk scatters in this voxel iff d < seg, at s = t_cur + d (the device skips the divide
 *       where tau - acc >= 2 (sigma seg), which decides the same);
 *     else, or without a scatter: acc = acc + sigma seg; the walk ends if t_exit >= b; else the axis of the smallest tnext steps, x before y
 *     before z on ties (x if tnext_x <= tnext_y and tnext_x <= tnext_z, else y if tnext_y <= tnext_z, else z): index += step, tnext +=
 *     tdelta, and the walk ends if the index left [0, n - 1]; t_cur = t_exit.
 * Free flight on segment k: u as for pt_medium (dimension 0 of S ^ 0x5bd1e995), tau = -log1pf(-u), Walk(P, D, t, tau); the segment scatters
 *   iff the walk does, at x = fma(D, s, P); a surviving segment takes no factor.
 * Transmittance of a light sample: T = expf(-acc) of Walk(o, w, limit, +inf) (no voxel reaches tau); T = 1 exactly when acc = 0.
 * A 1 x 1 x 1 grid of density 1.0f computes d = tau / sigma_t, d < b - a, s = a + d and T = expf(-(sigma_t (b - a))): the homogeneous
 * medium's frame bit for bit (tnext is Clip's own far slab on every axis, so t_exit = b). */
#define PT_GRID_MAX_DIM 256
/* PT_EINVAL, naming pt_set_medium_density, with the held grid left as it was: ctx or density NULL, a dimension outside [1, PT_GRID_MAX_DIM],
 * a density that is negative or not finite */
int pt_set_medium_density(pt_context* ctx, const float* density, int32_t nx, int32_t ny, int32_t nz);
int pt_clear_medium_density(pt_context* ctx);
/* the held grid: dims = {nx, ny, nz} ({0, 0, 0} when none is held) and up to cap densities into out (out may be NULL when cap is 0);
 * returns 1 if a grid is held, 0 if not, PT_EINVAL for a NULL ctx or dims or a negative cap */
int pt_debug_medium_density(pt_context* ctx, float* out, int64_t cap, int32_t dims[3]);
/* the device walk of the live grid on given numbers, n items: in, 12 floats each {P.xyz, D.xyz (unit), t, u, limit, 3 spare}; out, 8 floats
 * each {a, b of Clip(P, D, t), 1 if Walk(P, D, t, -log1pf(-u)) scatters else 0, its s (-1 without a scatter), acc of Walk(P, D, t, +inf)
 * (the optical depth over [0, t]), T over [0, limit], the voxels the free-flight walk visited, the linear index of the voxel it scattered
 * in (-1 without)}.  PT_EINVAL when no grid is live or a bound of the box is infinite */
int pt_debug_grid(pt_context* ctx, const float* in, int64_t n, float* out);

/* ---- interiors of dielectrics (new: opt-in with pt_set_material_interior; coloured glass, murky liquids, wax, jade, milk) ----
 * An interior is a medium bound to a material of type 2 (glass) or 6 (frosted glass, option "frosted") and active exactly while the path is
 * inside it (the `inside` flag of the specular and frosted vertices is true): chromatic Beer-Lambert absorption sigma_a and grey scattering
 * sigma_s with a Henyey-Greenstein g.  Only pt_render_nee (every strategy, PT_NEE_BSDF too: no light sample is involved) and the NEE path of
 * pt_render_adaptive_ex render it.  A binding lives like a texture binding (pt_set_material_texture): the material is any index added so far,
 * it is kept across uploads and on a host-only context, every rank of a tiled frame sets its own copy, and a binding on a material whose type
 * on the device is neither 2 nor 6 is ignored where the table for the device is made, as a texture on a non-diffuse material is.  The table reads
 * the type alone, not option "frosted": with the option off a type-6 surface is inert and no path enters through it, but a path that is inside
 * type-2 glass and whose segment ends on a bound type-6 triangle takes that binding's interior on the segment all the same.  A binding is
 * live as soon as it exists, even an all-zero one: while any is live the NEE launches take the interior instances of k_nee (stat "nee_family"
 * 10), which serve frames with and without a medium and its density grid, and pt_render, pt_generate_rays, pt_trace_rays, pt_render_adaptive
 * and pt_render_adaptive_ex with PT_ADAPT_PATH_RENDER return PT_EINVAL naming pt_clear_material_interiors, checked before the device.
 * Without a binding every path launches the kernels it launched before and computes the same bits.  The guides, the denoisers and temporal
 * accumulation keep the interior-free view.
 * The estimator, float32 with no contraction (log1pf, expf: the device library's; the divide IEEE), on segment k while `inside` is true:
 *   ti is the closest hit, at distance t.  The interior is the one bound to the material of triangle ti -- the surface the path will leave
 *   through, so the path carries no extra state.  A miss (a leaky mesh) or a material without a binding: no interior on this segment.
 *   Free flight, only if sigma_s > 0: u = (pt_nee_rand(S ^ 0x5bd1e995, k, 0) >> 8) 2^-24 -- dimension 0 of the medium's stream, which the
 *     exterior medium never draws while inside --, d = -log1pf(-u) / sigma_s; the segment scatters iff d < t; l = d when it scatters, else t.
 *   Absorption: per channel c, factor_S[c] *= expf(-(sigma_a[c] l)); a channel with sigma_a[c] == 0 multiplies by exactly 1.  An all-zero
 *     product ends the path.  Surviving the free flight takes no other factor: its probability is the scattering transmittance.
 *   Scatter vertex (it consumes segment k): no light sample in any strategy (a shadow ray from inside ends on the object's own boundary);
 *     the new direction is the medium's step 3 with the interior's g and u1, u2 from dimensions 1 and 2 of the same stream; the next segment
 *     starts at fma(D, d, P) per component.  It is no lobe vertex for what follows: an emitter hit or a sky miss on segment k + 1 has weight
 *     1 in every strategy, as after a frosted refraction.  `inside` is unchanged and nothing is drawn from the LCG.
 *   Surface hit: after the absorption factor the vertex proceeds exactly as without an interior.
 * So with absorption only rnds and rays after a frame are the unbound frame's; with scattering they differ only for paths that scatter.
 * The medium of pt_set_medium and its grid keep applying wherever `inside` is false; both kinds may be set at once.
 * Light inside a scattering object arrives only by paths that refract out and find a light: good under a sky or large emitters, noisy
 * under a tiny lamp (light sampling through a refracting boundary is not done). */
typedef struct pt_interior {
    float sigma_a[3];   /* absorption per unit length, per channel, finite, >= 0 */
    float sigma_s;      /* scattering per unit length (grey), finite, >= 0 */
    float g;            /* Henyey-Greenstein asymmetry, |g| <= 0.99 */
} pt_interior;          /* 20 bytes */
void pt_interior_defaults(pt_interior* in);      /* all zero */
/* PT_EINVAL, naming pt_set_material_interior and the field, with the held binding left as it was: ctx or interior NULL, material not the index
 * of a material added so far, a NaN, a negative or infinite coefficient, |g| > 0.99 */
int pt_set_material_interior(pt_context* ctx, int32_t material, const pt_interior* interior);
int pt_clear_material_interiors(pt_context* ctx);
/* the binding of `material` into *interior (all zero when it holds none); returns 1 if one is held, 0 if not, PT_EINVAL for a NULL argument
 * or a material that was never added */
int pt_get_material_interior(const pt_context* ctx, int32_t material, pt_interior* interior);
/* the device functions of an interior on given numbers, n items: in, 12 floats each {sigma_a.rgb, sigma_s, g, t, u, u1, u2, D.xyz (unit)};
 * out, 10 floats each {d = -log1pf(-u) / sigma_s (-1 when sigma_s is 0: nothing is drawn), 1 if d < t else 0, l, the absorption factor per
 * channel, the new direction from (u1, u2) around D (unit), 0}.  No binding is needed */
int pt_debug_interior(pt_context* ctx, const float* in, int64_t n, float* out);

/* ---- a light hierarchy for pt_render_nee (new: opt-in with option "light_tree"; many emitters) -----------
 * Option "light_tree" = 1 (default 0: every frame is what it was, bit for bit): the triangle-light branch of the light sample picks its
 * triangle by walking a binary tree over the light table, with a probability P that depends on the vertex, and the weight of an emitter hit
 * uses the same P.  Everything else of the estimator stays: the point on the triangle, the shadow ray, the contribution, the sky branch and
 * P_env, the analytic branch and P_ana, the hash streams and the LCG (rnds and rays after a frame are the option-off frame's).  The option is
 * inert where no triangle-light sample is taken: pt_render, the wavefront path, PT_NEE_BSDF, a scene without emitting triangles.  With the
 * option on and a non-empty light table the NEE launches take the light-tree instances of k_nee (stat "nee_family" 11), which serve frames
 * with and without an interior binding, a medium and its grid.
 * The tree (built on the host next to the light table, deterministic, invalidated with the table; stats "light_tree_nodes",
 * "light_tree_depth"): one light per leaf; a light's weight phi is the table's, area (E.r + E.g + E.b), in double.  A node holds the box of its
 * lights' vertices as a sphere -- centre c = the box's centre rounded to float32, radius r = the largest distance in double from that c to a
 * corner of the box, rounded up to float32 and then one ulp more, so the sphere contains the box -- and phi = phi(left) + phi(right), summed in
 * double and rounded to float32 once per node.  A node of more than one light splits at the spatial median of its lights' centroids
 * ((r1 + r2 + r3) / 3 in double) along the longest axis of the centroids' box (z before y before x on a tie; left: centroid < median, in the
 * order the lights had); when that leaves a side empty, or when the node's depth d and count n have d + 1 + ceil(log2(n - 1)) > 64, it
 * splits into the first ceil(n / 2) and the rest of its lights ordered by the centroid's coordinate on that axis (stable).  So no leaf is
 * deeper than 64.  Nodes lie depth first, the left child at node + 1, and the lights in leaf order (tree order): a node covers the tree-order
 * lights [first, first + count).
 * The walk from origin o with cull normal G and a number u in [0, 1), float32 with no contraction (dot products as fma(z, z', fma(y, y', x x'))):
 *   importance of a child: 0 if fma-dot(G, c - o) < -r (its sphere lies entirely below the horizon), else phi / max(|c - o|^2, r^2);
 *   if iL + iR is not a positive finite number (both culled; a light at o), iL, iR = the two phi; pL = iL / (iL + iR) (0.5 if that is no
 *   number in [0, 1]); u < pL: left, u = u / pL, P *= pL; else right, u = (u - pL) / (1 - pL), P *= 1 - pL; u >= 1 becomes 1 - 2^-24.
 *   At a leaf the light is picked with probability P (1 for a table of one light).  No orientation cones (the emitters are two-sided) and no
 *   cosine bound (sqrt(1 - cos^2) is ill-conditioned where it would matter; the cull removes what a room's own walls cannot see).
 * At a lobe vertex: o is the shadow ray's origin, G the geometric normal on the ray's side (the zero vector at a scatter vertex of the medium,
 * where nothing is culled), u = u0, dimension 0 of the light sample's stream; no extra number is drawn.
 *   p_l = P inv_area r^2 / |cos_y|, times 1 - P_env and 1 - P_ana as before, inv_area = (float)(1 / area), the value P_sel / area has for a
 *   table of one light.
 * An emitter hit after a lobe vertex: the weight walk descends from the root towards the hit triangle's leaf by the nodes' ranges, with the o
 * and G of that previous lobe vertex, and multiplies the same branch probabilities in the same order; p_l = P inv_area t^2 / cos as before.
 * The pick's P of a light and the weight walk's P of that light are the same float.
 * Two limits: P is a product of rounded branch probabilities, not an exact count of u0 values as P_sel is (the P of all lights sum to 1
 * within depth 2^-22), and the 24 bits of u0 cannot reach a leaf whose probability is below 2^-24. */
/* the tree (host only, as pt_debug_light_table): *n_nodes, *n_lights = the counts; the first min(node_cap, *n_nodes) nodes, 8 floats each {c.xyz,
 * r, phi, bits(first), bits(count), bits(right child; the left one is node + 1; count 1: a leaf)}, and the first min(light_cap, *n_lights)
 * tree-order lights as add-order triangle indices are written (either array may be NULL) */
int pt_debug_light_tree(pt_context* ctx, float* nodes, int64_t node_cap, int64_t* n_nodes, int32_t* orig_tri, int64_t light_cap, int64_t* n_lights);
typedef struct pt_light_tree_eval {
    int32_t tri;        /* the add-order triangle the walk picked (-1: an empty table) */
    float p;            /* its probability P */
    float p_weight;     /* the weight walk's P of tris[i] (0 where tris[i] is no light) */
    int32_t slot;       /* the picked light's tree-order index */
} pt_light_tree_eval;   /* 16 bytes */
/* both walks on given numbers, n items: points (o, 3 floats each), normals (G, 3 floats each), u0 and tris (add-order triangle indices) in,
 * out[i] as above; on_device = 0: by the library's host code (any context with the scene uploaded, host-only too), 1: by the kernel
 * k_debug_light_tree, which calls what the light-tree instances of k_nee call.  Option "light_tree" need not be on */
int pt_debug_light_tree_eval(pt_context* ctx, const float* points, const float* normals, const float* u0, const int32_t* tris, int64_t n,
                             pt_light_tree_eval* out, int32_t on_device);

/* ---- smooth shading from vertex normals for pt_render_nee (new: opt-in with option "smooth_normals"; the reference shades with the
 * triangle's geometric normal only) -----------
 * Authoring (host data; all of it works on a host-only context, none of it rebuilds the BVH).  Triangles are counted in add order over
 * the whole scene, the order of pt_debug_scene_copy.  A triangle HAS vertex normals iff all nine values recorded for it are finite and
 * none of its three vectors is zero; every other triangle (never set, cleared, added later) has none.  Normals need not be unit length.
 * The recorded normals survive pt_upload_triangles / pt_upload_materials.  They are repacked LAZILY: the first pt_render_nee /
 * pt_render_adaptive_ex (path NEE) / pt_debug_shading_normal that runs with the option on after the normals or the uploaded triangles
 * changed copies them to the device and runs k_pack_vertex_normals (pt_smooth.hip) on the context's stream: per PACKED triangle (the
 * permutation `orig` of pt_debug_bvh_copy) three float4 {n.xyz, flag}, n = the corner's normal divided by its length in float64 and
 * rounded once to float32, flag != 0 iff the triangle has vertex normals.
 *   pt_set_vertex_normals      normals = count x 9 floats, n1 n2 n3 per triangle, for triangles [first_triangle, first_triangle + count);
 *                              PT_EINVAL when the range is not inside the triangles added so far
 *   pt_clear_vertex_normals    no triangle has vertex normals
 *   pt_compute_vertex_normals  object = index of an object (pt_end_obj order) or -1 for all (each object on its own).  Per corner: the sum,
 *                              in float64 and add order, of angle x face normal (the record's N divided by its float64 length; angle = the
 *                              triangle's interior angle at that corner, acos of the clamped float64 cosine) over the triangles of the same
 *                              object that have a corner at the same position bit for bit (+0 == -0) and whose face normal is within
 *                              crease_degrees of this triangle's (float64 dot >= cos(crease_degrees) - 1e-12; the triangle itself always counts),
 *                              normalised, rounded to float.  crease_degrees = 0: the face normal on every corner.  A triangle whose N is zero or
 *                              not finite gets none.  PT_EINVAL: crease_degrees not in [0, 180], object out of range
 *   pt_add_obj                 a face whose corners all carry a vn index (i//k, i/j/k) that exists records, for its fan triangles, those
 *                              normals transformed by the inverse transpose of the positions' linear map -- x negated, rotate_x(pitch),
 *                              rotate_y(yaw), DIVIDED by scale -- in float64, normalised, rounded to float.  The triangles are unchanged.
 *   pt_debug_vertex_normals    normals: 9 floats per added triangle as recorded (0 where none), has: 1 / 0 per triangle; either may be NULL
 * Option "smooth_normals" = 1 (default 0: every path computes what it computed before, bit for bit): pt_render_nee (every strategy, with
 * and without an environment) and pt_render_adaptive_ex with path PT_ADAPT_PATH_NEE shade with the interpolated normal; pt_render,
 * pt_generate_rays, pt_trace_rays, pt_render_adaptive and pt_render_adaptive_ex with PT_ADAPT_PATH_RENDER (every variant) return
 * PT_EINVAL naming the option.  pt_render_aovs keeps the geometric normal; pt_render_aovs_ex with PT_AOV_SHADED writes Ns into the guides
 * the denoisers and pt_temporal_accumulate read.
 * The estimator is pt_render_nee's with these changes at a hit of segment k (float32, fma where dot3 / cross3 / madd have it:
 * dot3(a, b) = fma(a.z, b.z, fma(a.y, b.y, a.x b.x)), cross3(a, b).x = fma(a.y, b.z, -(a.z b.y)) and cyclic, madd(u, s, w) = fma(u, s, w)):
 *   N = the record's normal, Ng = N flipped against the ray (as before), hp = madd(D, t, P), vertices r1 r2 r3, packed normals n1 n2 n3;
 *   a1 = max0(dot3(cross3(r3 - r2, hp - r2), N)), a2 = max0(dot3(cross3(r1 - r3, hp - r3), N)), a3 = max0(dot3(cross3(r2 - r1, hp - r1), N))
 *        (max0(c) = c > 0 ? c : 0: the three terms of the exact triangle test, each the weight of the opposite vertex);
 *   s = madd(n3, a3, madd(n2, a2, n1 * a1)), l2 = dot3(s, s), Ns = s * (1.0f / sqrtf(l2)) (both IEEE); Ns = -Ns if dot3(Ns, Ng) < 0;
 *   Ns = Ng, the same bits, when the triangle has no vertex normals, when not 0 < l2 < inf, or when not dot3(-D, Ns) > 0.
 * Ns replaces the flipped normal in: the emitter cosine, the cosine-sampled frame and direction, factor_L's cosine, the halfway term,
 * Fresnel, the mirror direction and the refraction, the light sample's cosine and p_b (and fL' / fB'), and the p_b of W_b at the next
 * hit or miss.  Offsets use the geometric normal: the new origin is hp +- 0.001 Ng and the light sample's origin o = hp + 0.001 Ng.
 * Geometric side -- specular vertices (types 1, 2): the vertex is evaluated with Ns; if the new direction w BEFORE normalisation has
 * dot3(w, Ng) <= 0 (reflection) or >= 0 (refraction), the whole vertex -- Fresnel, the choice between reflection and refraction, the
 * direction, the factors -- is evaluated again with Ng in place of Ns and the same LCG value, and that evaluation stands (one LCG draw,
 * factors applied once).  Lobe vertices (types 0, 3): a light sample counts only if dot3(w, Ng) > 0 as well as dot3(w, Ns) > 0; after the
 * vertex's light sample, its two LCG draws and its own update (type 0: the factors; type 3: its emission), the path ends -- no further
 * segment, draw or light sample in this sample -- if the sampled direction before normalisation has dot3(w, Ng) <= 0; rays[] then holds
 * that direction and origin.
 * With the option on and no triangle carrying vertex normals the frame (colors, rnds, rays) is the option-off frame bit for bit.  With
 * normals present the paths differ from pt_render's, so rnds and rays no longer equal pt_render's. */
int pt_set_vertex_normals(pt_context* ctx, int64_t first_triangle, int64_t count, const float* normals);
int pt_clear_vertex_normals(pt_context* ctx);
int pt_compute_vertex_normals(pt_context* ctx, int32_t object, float crease_degrees);
int pt_debug_vertex_normals(const pt_context* ctx, float* normals, int32_t* has);
/* the shading normal of the closest hit of each ray, by the device function the smooth k_nee instances call (any setting of the option):
 * out_tri[i] = add-order triangle or -1, out_ns[4 i ..] = {Ns.xyz, t} ({0, 0, 0, -1} for a miss) */
int pt_debug_shading_normal(pt_context* ctx, const pt_ray* rays, int64_t n, int32_t* out_tri, float* out_ns);

/* ---- albedo textures with UV coordinates for pt_render_nee (new: opt-in with option "textures"; the reference has one kd per
 * material and throws vt / map_Kd away) -----------
 * Authoring (host data; all of it works on a host-only context, none of it rebuilds the BVH).
 * Textures.  pt_add_texture returns the new texture's index (0, 1, ...) or a negative code.  rgb = w x h x 3 floats, ROW 0 IS THE TOP of
 * the image (where v is just below 1); p = NULL: pt_texture_defaults = {filter 1, srgb 0}.  filter 0 = nearest, 1 = bilinear; srgb = 1
 * applies the sRGB EOTF on the host first: c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4), in double, rounded to float.
 * PT_EINVAL: w or h below 1 or above PT_TEX_MAX_SIZE, already PT_TEX_MAX_COUNT textures, a texel that is not finite, negative or above
 * 65504 (with srgb = 1 also after the EOTF), filter or srgb outside {0, 1}, more than 2^31 - 1 texels over all textures.  Stored form (host and device): a texel is 8 bytes, three
 * IEEE half values r g b (each the float rounded to nearest-even) and 16 zero bits; all textures live in one device buffer, each with a
 * descriptor {first texel, w, h, filter}.  Textures and bindings survive pt_upload_triangles / pt_upload_materials.
 *   pt_clear_textures          drops all textures and all bindings
 *   pt_set_material_texture    binds texture (an index, or -1: none) to a material added so far; PT_EINVAL when either index is out of
 *                              range.  A binding on a material whose type is not 0 is accepted and ignored
 *   pt_debug_texture           the stored halves widened to float: *w, *h, *filter (any may be NULL); with rgb != NULL w x h x 3 floats,
 *                              cap = the texels rgb holds (PT_EINVAL when too small)
 * UV coordinates.  Triangles are counted in add order over the whole scene, as for pt_set_vertex_normals; the range rules are the same.
 * A triangle HAS uvs iff all six values recorded for it are finite and at most 65536 in magnitude; every other triangle has none.
 *   pt_set_vertex_uvs          uvs = count x 6 floats, u1 v1 u2 v2 u3 v3 per triangle, for triangles [first_triangle, first_triangle + count)
 *   pt_clear_vertex_uvs        no triangle has uvs
 *   pt_debug_vertex_uvs        uvs: 6 floats per added triangle as recorded where it has uvs, 0 where it has none; has: 1 / 0; either may be NULL
 *   pt_add_obj                 parses vt u v [w]; a face whose corners all carry a vt index that exists (i/j, i/j/k; the index rules of v)
 *                              records those uvs for its fan triangles.  map_Kd <file> in the MTL: the last blank-separated token is
 *                              the file name, resolved against the MTL's directory; a line with a -option token is skipped; .ppm (binary
 *                              P6, srgb = 1) and .pfm (srgb = 0, rows flipped to top-first) load with filter 1, extensions compared
 *                              without case, each file once per call, and the texture is bound to the material pt_add_obj creates.  Any
 *                              other extension or a read failure leaves the material untextured and pt_add_obj succeeds (statistics
 *                              "obj_textures_loaded" / "obj_textures_skipped" count the map_Kd lines of the last pt_add_obj either way).
 *                              Triangles and material records are what they were.
 * Bindings, textures and uvs take effect LAZILY: the first textured launch after any of them, the uploaded triangles or the uploaded
 * materials changed copies them to the device on the context's stream and runs k_pack_vertex_uvs (pt_texture.hip): per PACKED
 * triangle two float4 {u1, v1, u2, v2}, {u3, v3, flag, 0}, flag != 0 iff the triangle has uvs.
 * Option "textures" = 1 (default 0: every path computes what it computed before, bit for bit): pt_render_nee (every strategy, with and
 * without an environment, with and without smooth_normals) and pt_render_adaptive_ex with path PT_ADAPT_PATH_NEE use the textured
 * albedo; pt_render, pt_generate_rays, pt_trace_rays, pt_render_adaptive and pt_render_adaptive_ex with PT_ADAPT_PATH_RENDER return
 * PT_EINVAL naming the option.  pt_render_aovs keeps the material's kd; pt_render_aovs_ex with PT_AOV_SHADED writes kd' into the guides
 * the denoisers and pt_temporal_accumulate read.
 * The textured albedo kd' of a hit at hp = madd(D, t, P) on packed triangle ti whose material has type 0 and texture T bound and which
 * has uvs (float32; fma as dot3 / cross3 / madd have it, see the smooth-normals block above):
 *   a1, a2, a3 = the three weights of the shading normal above (max0 included), A = (a1 + a2) + a3; not 0 < A < inf: kd' = kd;
 *   inv = 1.0f / A (IEEE); u = fmaf(u3, a3, fmaf(u2, a2, u1 * a1)) * inv, v likewise; fu = u - floorf(u), fv = v - floorf(v) (repeat);
 *   nearest:  x = min(w - 1, (int)floorf(fu * w)), y = min(h - 1, (int)floorf((1.0f - fv) * h)), tex = texel(x, y);
 *   bilinear: px = fmaf(fu, w, -0.5f), x0 = floorf(px), tx = px - x0, columns ((int)x0 mod w + w) mod w and the next one mod w; rows the
 *             same with py = fmaf(1.0f - fv, h, -0.5f); per channel top = fmaf(tx, c10 - c00, c00), bot = fmaf(tx, c11 - c01, c01),
 *             tex = fmaf(ty, bot - top, top)  (cXY: column X, row Y of the 2 x 2 taps);
 *   kd' = kd * tex, component-wise; kd is the value the untextured vertex uses.
 * Every other case -- option off, no texture bound, no uvs, a type other than 0 -- yields kd, the same bits.  kd' replaces kd in the
 * preview colour of iterations == 1 (kd' + emission), in the factor_L update of the type-0 vertex and in fL' of that vertex's light
 * sample (triangle light and sky), and nowhere else: ks, emission and the light table are untouched, and no LCG draw and no pt_nee_rand
 * value depends on kd', so a textured frame leaves rnds and rays as the untextured frame does. */
typedef struct { int32_t filter, srgb; } pt_texture_params;
#define PT_TEX_MAX_SIZE 8192
#define PT_TEX_MAX_COUNT 1024
void pt_texture_defaults(pt_texture_params* p);
int pt_add_texture(pt_context* ctx, const float* rgb, int32_t w, int32_t h, const pt_texture_params* p);
int pt_clear_textures(pt_context* ctx);
int pt_set_material_texture(pt_context* ctx, int32_t material, int32_t texture);
int pt_debug_texture(const pt_context* ctx, int32_t texture, float* rgb, int64_t cap, int32_t* w, int32_t* h, int32_t* filter);
int pt_set_vertex_uvs(pt_context* ctx, int64_t first_triangle, int64_t count, const float* uvs);
int pt_clear_vertex_uvs(pt_context* ctx);
int pt_debug_vertex_uvs(const pt_context* ctx, float* uvs, int32_t* has);
/* the albedo of the closest hit of each ray, by the device function the textured k_nee instances call (any setting of the option):
 * out_tri[i] = add-order triangle or -1, out_rgbt[4 i ..] = {kd'.rgb, t} ({0, 0, 0, -1} for a miss) */
int pt_debug_albedo(pt_context* ctx, const pt_ray* rays, int64_t n, int32_t* out_tri, float* out_rgbt);

/* ---- a rough-metal (GGX) material for pt_render_nee (new: opt-in with option "glossy"; the reference has chalk, a perfect mirror, perfect
 * glass and a lamp, and leaves the ray alone at any other material type) -----------
 * Option "glossy" = 1 (default 0: every path computes what it computed before, bit for bit, and type 4 stays inert): pt_render_nee (every
 * strategy, with and without an environment, smooth_normals and textures) and pt_render_adaptive_ex with PT_ADAPT_PATH_NEE shade a hit on
 * a material of type 4 as the lobe vertex below; pt_render, pt_generate_rays, pt_trace_rays, pt_render_adaptive and pt_render_adaptive_ex
 * with PT_ADAPT_PATH_RENDER return PT_EINVAL naming the option, checked before the device (PT_ENODEVICE).  With the option on and no
 * material of type 4 among those uploaded last, the host launches the kernels it launches with the option off: the frame (colors, rnds,
 * rays) is the option-off frame bit for bit.
 * Roughness.  alpha = pt_material_roughness(shininess) = the float nearest to min(1, max(0.03, sqrt(2 / (shininess + 2)))) evaluated in
 * double; 1 when shininess is not finite or negative.  pt_upload_materials writes it into field n of the DEVICE copy of a type-4 material
 * (n is read for type 2 only); the host records are what they were.  kd, ks, emission and a texture binding of a type-4 material are
 * ignored; F0 (pt_material_init: from N and K) is its colour.
 * The vertex (float32; fma where dot3 / cross3 / madd have it, see the smooth-normals block above; sqrtf and / IEEE;
 * normalize(v) = v * (1.0f / sqrtf(dot3(v, v)))).  A type-4 hit is a lobe vertex for every rule that speaks of lobe vertices: it takes a
 * light sample when k + 1 < iterations, the next emitter hit or sky miss is weighted by W_b, under smooth_normals it follows the
 * geometric-side rules of lobe vertices and offsets use Ng.  It draws exactly two LCG values rnd1, rnd2 after its light sample.
 *   N = the shading normal (Ns under smooth_normals), (Z, X) the frame diffuse_direction builds from N (prog.cl:205-212; X = cross3(N, Z));
 *   local coordinates v = (dot3(v, X), dot3(v, Z), dot3(v, N)); o = local(-D).
 *   Sampling (visible normals, Heitz 2018):
 *     Vh = normalize(alpha o.x, alpha o.y, o.z); l2 = fmaf(Vh.y, Vh.y, Vh.x Vh.x);
 *     T1 = l2 > 0 ? (-Vh.y / sqrtf(l2), Vh.x / sqrtf(l2), 0) : (1, 0, 0); T2 = cross3(Vh, T1);
 *     r = sqrtf(rnd1); (s, c) = the sine and cosine diffuse_direction takes of (float)(6.283185307179586 * (double)rnd2);
 *     t1 = r c; t2 = r s; q = 0.5f (1.0f + Vh.z); t2 = fmaf(q, t2, (1.0f - q) sqrtf(max0(fmaf(-t1, t1, 1.0f))));
 *     Nh = madd(Vh, sqrtf(max0(fmaf(-t2, t2, fmaf(-t1, t1, 1.0f)))), madd(T2, t2, T1 * t1));
 *     h = normalize(alpha Nh.x, alpha Nh.y, max0(Nh.z)); w = madd(h, 2.0f dot3(o, h), -o), local;
 *     the world direction before normalisation is madd(Z, w.y, madd(N, w.z, X * w.x)), handed to the tail every vertex shares.
 *   Lobe terms (unit local vectors; a2 = alpha alpha):
 *     D(h) = a2 / (pi (d d)) with d = fmaf(a2, h.z h.z, fmaf(h.y, h.y, h.x h.x));
 *     G1(v) = (2.0f v.z) / (v.z + sqrtf(fmaf(a2, fmaf(v.y, v.y, v.x v.x), v.z v.z))), 0 unless v.z > 0;
 *     p_b(w) = (G1(o) D(h)) / (4.0f o.z), 0 unless o.z > 0; for a given w (a light sample), h = normalize(o + w);
 *     g(w) = F G1(w), F = fresnel(F0, h, -o): Schlick on |dot3(h, o)| (prog.cl:219-222), the separable Smith term (G2 / G1(o) = G1(w)).
 *   Update: factor_S *= g(w), the factor a mirror multiplies by F.  Unless w.z > 0 the path ends after the two draws, as a lobe direction
 *   below the geometric surface ends it (rays[] holds that direction and origin).  The new origin is hp + 0.001 Ng.
 *   Light sample at the vertex (triangle light and sky): as pinned for pt_render_nee, with p_b = p_b(w) in place of max(0, N.w) / pi and,
 *   for the factors the vertex's own update with w would give, fS' = fS g(w) (fL, fB unchanged); rejected unless w.z > 0 (and, under
 *   smooth_normals, dot3(w, Ng) > 0) and unless p_b(w) > 0.
 *   W_b of the next emitter hit or sky miss uses the p_b the vertex sampled its direction with (kept from the vertex, through the one
 *   device function that states the density).
 *   Preview (iterations == 1): F0 + emission.
 * The light table, the pt_nee_rand keys, ks, kd and textures are untouched.
 * Guides: pt_render_aovs_ex with PT_AOV_SHADED and the option on gives a terminal type-4 hit the albedo tint x F0 (as a terminal mirror; it
 * is not followed as a specular step) and the normal Ns; with the option off, and in geometric guides, the buffers are what they were.
 * Changing the option makes no guides stale. */
float pt_material_roughness(float shininess);
/* the device functions of the vertex (host-only context: PT_ENODEVICE).  Per item 9 floats in: N (unit), D (unit, toward the surface),
 * alpha, rnd1, rnd2; 8 out: the world direction w before normalisation (3), p_b as sampled, G1(w), F.x for F0 = 0.04, p_b evaluated again
 * from normalize(w) the way a light sample evaluates it, o.z */
int pt_debug_glossy(pt_context* ctx, int64_t n, const float* N_D_alpha_rnd, float* out);

/* ---- a coated-diffuse (plastic) material for pt_render_nee (new: opt-in with option "coated") -----------
 * Option "coated" = 1 (default 0: every path computes what it computed before, bit for bit, and type 5 stays inert): pt_render_nee (every
 * strategy, with and without an environment, smooth_normals, textures and glossy) and pt_render_adaptive_ex with PT_ADAPT_PATH_NEE shade a
 * hit on a material of type 5 as the two-lobe vertex below, a diffuse base under a rough dielectric coat; pt_render, pt_generate_rays,
 * pt_trace_rays, pt_render_adaptive and pt_render_adaptive_ex with PT_ADAPT_PATH_RENDER return PT_EINVAL naming the option, checked before
 * the device (PT_ENODEVICE).  With the option on and no material of type 5 among those uploaded last, the host launches the kernels it
 * launches with the option off (those of option glossy included): the frame (colors, rnds, rays) is the option-off frame bit for bit.
 * Whether type 4 is the rough metal in a frame that shades type 5 follows option glossy, as everywhere else.
 * Material.  alpha = pt_material_roughness(shininess), written into field n of the DEVICE copy of a type-5 material as for type 4; F0 from
 * pt_material_init (N = 1.5, K = 0: 0.04); kd' = kd, times the bound texture's texel under option textures (the lookup runs for type 0 or
 * 5 in these frames; pt_set_material_texture accepts any material).  ks and emission of a type-5 material are ignored; it is no light.
 * The vertex (float32, the conventions of the rough-metal block above, whose D, G1, p_glossy(h) = (G1(o) D(h)) / (4.0f o.z) and
 * fresnel it reuses; F(c) = fresnel on the cosine |c|).  A type-5 hit is a lobe vertex for every rule that speaks of lobe vertices: light
 * sample when k + 1 < iterations, W_b at the next emitter hit or sky miss, the geometric-side rules under smooth_normals, offsets along Ng,
 * exactly two LCG values rnd1, rnd2 after its light sample.  N, the frame (Z, X), local coordinates and o = local(-D) as for type 4.
 *   Lobe choice:  Fo = F(o.z); fm = ((Fo.x + Fo.y) + Fo.z) / 3.0f; km = ((kd'.x + kd'.y) + kd'.z) / 3.0f; s = fmaf(1.0f - fm, km, fm);
 *     ps = s > 0 ? fm / s : 0.5f, clamped to [0.1f, 0.9f]; u_sel = (pt_nee_rand(~key, k, 1) >> 8) * 2^-24 (key as for the light samples; ~key
 *     with dimension 0 is the environment's selection); the coat lobe is chosen iff u_sel < ps.  Nothing is drawn from the LCG for it.
 *   Coat lobe: w and h by the visible-normal sequence of type 4 on the same disc point of rnd1, rnd2.
 *   Base lobe: w = (r c, r s, sqrt(1.0f - rnd1)), diffuse_direction's cosine lobe (the bits of a type-0 lane); h = normalize(o + w).
 *   The world direction before normalisation is madd(Z, w.y, madd(N, w.z, X * w.x)) for both.
 *   Terms, for w with half vector h (c = max0(w.z)):
 *     pg = p_glossy(h); p_b(w) = fmaf(ps, pg, ((1.0f - ps) c) * (1/pi)f)                       -- the mixture, whichever lobe drew w
 *     spec(w) = (F(|dot3(h, o)|) G1(w)) * pg                                                    [= F D(h) G1(o) G1(w) / (4 o.z)]
 *     diff(w) = (((1 - F(o.z)) * (1 - F(c))) * kd') * (c * (c * (1/pi)f))                       (componentwise)
 *     g(w) = (spec(w) + diff(w)) * (1.0f / p_b(w)), 0 unless p_b(w) > 0
 *   Update: factor_S *= g(w); factor_L and factor_B are untouched.  Unless w.z > 0 and p_b(w) > 0 the path ends after the two draws, as at
 *   a type-4 vertex.  The new origin is hp + 0.001 Ng.
 *   Light sample at the vertex (triangle light and sky): as pinned for type 4 with the mixture: for the sample's unit w, ps as above and
 *   h = normalize(o + w), p_b = p_b(w), fS' = fS g(w) (fL, fB unchanged); rejected unless w.z > 0 (and, under smooth_normals,
 *   dot3(w, Ng) > 0) and unless p_b(w) > 0.  It is evaluated after the shadow ray.
 *   W_b of the next emitter hit or sky miss uses the mixture's p_b of the sampled w, kept from the vertex (one device function states
 *   the density for the sampler, the light sample and W_b).
 *   Preview (iterations == 1): kd' + emission.
 * A texture draws no random number here either, but ps is a function of kd': a texture on a type-5 material can change which lobe a
 * vertex picks and so the rest of the path; rnds and rays are those of the untextured frame exactly when it leaves km unchanged.
 * The light table, the OBJ reader and every existing pt_nee_rand key are untouched.
 * Guides: pt_render_aovs_ex with PT_AOV_SHADED and the option on gives a terminal type-5 hit the albedo tint x kd' and the normal Ns; with
 * the option off, and in geometric guides, the buffers are what they were.  Changing the option makes no guides stale. */
/* the device functions of the vertex (host-only context: PT_ENODEVICE), one thread per item, item i on lane i % 64.  Per item 12 floats
 * in: N (unit), D (unit, toward the surface), alpha, F0 (grey), kd (grey), rnd1, rnd2, u_sel; 10 out: the world direction w before
 * normalisation (3), ps, 1 if the coat lobe drew w else 0, p_b as sampled, g.x as sampled, p_b and g.x evaluated again from normalize(w)
 * the way a light sample evaluates them, o.z */
int pt_debug_coated(pt_context* ctx, int64_t n, const float* in, float* out);

/* ---- a thin-lens camera (depth of field) for pt_render_nee (new: opt-in with pt_set_lens) -----------
 * pt_camera stays the reference's 80-byte pinhole record; the lens lives in the context, as the environment does.  With no lens set, after
 * pt_clear_lens, or with aperture == 0 every path launches the kernels it launched before and computes what it computed before, bit for
 * bit.  While a lens with aperture > 0 is set, pt_render_nee (every strategy, with and without an environment and every option) and
 * pt_render_adaptive_ex with PT_ADAPT_PATH_NEE start each sample's path on the lens ray below; pt_render, pt_generate_rays, pt_trace_rays,
 * pt_render_adaptive and pt_render_adaptive_ex with PT_ADAPT_PATH_RENDER return PT_EINVAL naming pt_clear_lens, checked before the device
 * (PT_ENODEVICE).  pt_render_aovs, pt_render_aovs_ex, the denoisers and pt_temporal_accumulate keep the pinhole view and run as before:
 * the guides are sharp where the frame is not.  Setting or clearing the lens makes no guides stale.
 * The lens ray (float32; fma wherever dot3, madd and normalize3 use it: dot3(a, b) = fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)),
 * madd(u, s, w) = fmaf(u, s, w) per component, normalize3(a) = a * (1.0f / sqrtf(dot3(a, a))); division and sqrtf are IEEE).  Per sample, S
 * is the pixel's LCG state at the start of the sample (the light samples' key); the two LCG draws rnd1, rnd2 of the sub-pixel position
 * happen exactly as without a lens, and pp is the pinhole's point on the image plane (prog.cl:86-90):
 *   d  = pp - eye                                       (the pinhole direction before normalisation)
 *   f  = normalize3(lookat - eye);  Rh = normalize3(right);  Uh = normalize3(up)             (constants of a launch)
 *   Q  = madd(d, focus_distance / dot3(d, f), eye)      (the point in focus: on the plane at axial distance focus_distance)
 *   u1 = (pt_nee_rand(~S, -1, 0) >> 8) * 2^-24;  u2 = (pt_nee_rand(~S, -1, 1) >> 8) * 2^-24
 *   r  = sqrtf(u1);  (s, c) = the sine and cosine the cosine lobe takes of (float)(6.283185307179586 * (double)u2)   
 *   O  = madd(Uh, aperture * (r * s), madd(Rh, aperture * (r * c), eye))
 *   P  = O;  D = normalize3(Q - O)
 * Segment -1 of the complemented key is free: ~S carries dimension 0 (the environment's selection) and dimension 1 (the coat's lobe
 * choice) of segments >= 0, and the hash's counter 3 segment + dim + 1 is -2 or -1 for the lens, so every light sample and lobe choice
 * keeps its number.  The lens draws nothing from the LCG: rnds ends where a float64 replay with the same seeds ends.  The eye of the
 * type-0 highlight stays cam.eye.  The sample weight is 1 (a thin lens with a uniform disc needs no factor). */
typedef struct {
    float aperture;        /* lens radius in scene units, >= 0 and finite; 0 = pinhole */
    float focus_distance;  /* > 0 and finite: distance of the plane in focus from cam.eye, measured ALONG the optical axis */
    float _pad[2];
} pt_lens_params;
void pt_lens_defaults(pt_lens_params* p);      /* {0, 1, 0, 0} */
/* PT_EINVAL for an aperture that is negative, NaN or infinite, or a focus_distance that is not finite and > 0 */
int pt_set_lens(pt_context* ctx, const pt_lens_params* p);
int pt_clear_lens(pt_context* ctx);
/* autofocus: the axial distance of the first hit of pixel (x, y)'s centre ray (camera_get_ray(gid, cam, 0.5f, 0.5f), gid = y XM + x; row 0
 * as in the buffers): t * dot3(D, f); +inf on a miss.  Needs an uploaded scene and a device (host-only context: PT_ENODEVICE). */
int pt_focus_at(pt_context* ctx, const pt_camera* cam, int32_t x, int32_t y, float* distance);
/* the device's lens ray on caller-supplied items (as pt_debug_glossy; host-only context: PT_ENODEVICE): per item {gid, S} (two int32; the
 * two LCG draws are taken from S), out 6 floats P, D.  The kernel calls the device function the lens instances of k_nee call. */
int pt_debug_lens(pt_context* ctx, const pt_camera* cam, const pt_lens_params* lens, int64_t n, const int32_t* gid_state, float* out);

/* ---- a rough-dielectric (frosted glass) material for pt_render_nee (new: opt-in with option "frosted") -----------
 * Option "frosted" = 1 (default 0: every path computes what it computed before, bit for bit, and type 6 stays inert): pt_render_nee (every
 * strategy, with and without an environment, a lens, smooth_normals, textures, glossy and coated) and pt_render_adaptive_ex with
 * PT_ADAPT_PATH_NEE shade a hit on a material of type 6 as the vertex below, GGX microfacet reflection and refraction (Walter et al.
 * 2007); pt_render, pt_generate_rays, pt_trace_rays, pt_render_adaptive and pt_render_adaptive_ex with PT_ADAPT_PATH_RENDER return
 * PT_EINVAL naming the option, checked before the device (PT_ENODEVICE).  With the option on and no material of type 6 among those
 * uploaded last, the host launches the kernels it launches with the option off: the frame (colors, rnds, rays) is the option-off frame
 * bit for bit.
 * Material.  n and F0 are what pt_material_init gives a type-2 material from N and K; alpha = pt_material_roughness(shininess), written
 * into field shininess of the DEVICE copy of a type-6 material (field n holds the index of refraction; only type 0 reads shininess
 * otherwise); host records stay as they are.  kd, ks, emission and a texture binding of a type-6 material are ignored; it is no light.
 * The vertex (float32, the conventions of the rough-metal block above, whose visible-normal sampler, D, G1, p_glossy(h) and fresnel it
 * reuses).  A type-6 hit is a lobe vertex for these rules: it takes a light sample when k + 1 < iterations; it draws exactly two LCG
 * values rnd1, rnd2 after its light sample; under smooth_normals it follows the geometric-side rules.  N, the frame (Z, X), local
 * coordinates and o = local(-D) as for type 4; eta = n, or 1.0f / n when the path is inside (as type 2 does it).
 *   Half vector: h by the visible-normal sequence of type 4 on (rnd1, rnd2), the bits of a type-4 lane given the same inputs.
 *   Fresnel: c = dot3(o, h); F = fresnel(F0, h, -o); disc = 1.0f - (fmaf(-c, c, 1.0f) / eta) / eta; Fm = ((F.x + F.y) + F.z) / 3.0f;
 *     when disc <= 0 (total internal reflection) Fm = 1 and F = (1, 1, 1).
 *   Lobe choice: u_sel = (pt_nee_rand(~key, k, 1) >> 8) * 2^-24, the key a type-5 vertex uses for its choice (a vertex has one type);
 *     the vertex reflects iff u_sel < Fm.  Nothing is drawn from the LCG for it.
 *   Reflection: w = madd(h, 2.0f c, -o); p_b(w) = Fm * p_glossy(h); g(w) = (F G1(w)) * (1.0f / Fm).  The path ends unless w.z > 0 (under
 *     smooth_normals also unless dot3(w, Ng) > 0).  The new origin is hp + 0.001 Ng.
 *   Refraction: w = madd(h, c / eta - sqrtf(disc), (-o) / eta) (type 2's direction with h for the normal, componentwise divisions);
 *     g(w) = ((1 - F) G1((w.x, w.y, -w.z))) * (1.0f / (1.0f - Fm)); no 1 / eta^2 factor, as type 2 has none.  The path ends unless
 *     w.z < 0 (under smooth_normals also unless dot3(w, Ng) < 0).  `inside` toggles.  The new origin is hp - 0.001 Ng.
 *   Update: factor_R *= g(w); factor_L, factor_B and factor_S are untouched.  The world direction before normalisation,
 *   madd(Z, w.y, madd(N, w.z, X * w.x)), goes to the tail every vertex shares.
 *   Light sample at the vertex (triangle light and sky), reflection side only: for the sample's unit w with w.z > 0 (and, under
 *   smooth_normals, dot3(w, Ng) > 0), h = normalize(o + w); c, F, disc and Fm as above; p_b = Fm * p_glossy(h), fR' = fR g(w) (fL, fB, fS
 *   unchanged); rejected unless p_b > 0; evaluated after the shadow ray.  A sample with w.z <= 0 is rejected: light sampling does not
 *   reach through the surface.
 *   Weight of the next hit: after a reflected direction W_b of the next emitter hit or sky miss uses the p_b the vertex sampled with (one
 *   device function states it for the sampler and the light sample); after a refracted direction the next emitter hit or sky miss has
 *   weight 1 in every strategy, as after a type-1 / type-2 vertex: no light sample produces that direction.
 *   Preview (iterations == 1): kd + emission, as for an inert type.
 * Guides: pt_render_aovs_ex with PT_AOV_SHADED and the option on gives a terminal type-6 hit the albedo tint x 1 (as a terminal
 * dielectric) and the normal Ns; it is not followed as a specular step.  With the option off, and in geometric guides, the buffers are
 * what they were.  Changing the option makes no guides stale. */
/* the device functions of the vertex (host-only context: PT_ENODEVICE), one thread per item, item i on lane i % 64.  Per item 12 floats
 * in: N (unit), D (unit, toward the surface), alpha, F0 (grey), eta, rnd1, rnd2, u_sel; 10 out: the world direction w before
 * normalisation (3), Fm, 1 if the vertex reflects else 0, p_b as sampled (0 for a refraction), g.x as sampled, p_b and g.x evaluated again
 * from normalize(w) the way a light sample evaluates them (0, 0 for a refraction), o.z */
int pt_debug_frosted(pt_context* ctx, int64_t n, const float* in, float* out);

/* ---- per-pixel variance of the mean luminance (new: opt-in with option "moments"; the reference keeps the mean only) -------
 * With option "moments" = 1 every render path (pt_render in every variant, schedule and node mode, pt_trace_rays,
 * pt_render_adaptive, pt_render_nee, tiled ranks) also folds each sample's squared luminance into colors[].w, float32 in this order:
 *   l(c) = fmaf(0.0722f, c.b, fmaf(0.7152f, c.g, 0.2126f * c.r))
 *   q = l(x_s) * l(x_s), x_s = the colour of sample s (the value the running mean folds in)
 *   m2 = fmaf(m2, (float)s, q) / (float)(s + 1)      (the running mean of prog.cl:379; sample 0 starts from 0)
 * .xyz, rnds and rays are the same bits either way; with "moments" = 0 (default) .w = 0 exactly as before.
 * A frame starts at a launch whose first sample is 0 (pt_render / pt_render_nee at current_sample 0, pt_render_adaptive,
 * pt_trace_rays with current_sample 0); it is valid while every launch of it had "moments" = 1 (switching it on mid-frame makes
 * the frame invalid until the next one starts).  Per local pixel, with n = what pt_read_sample_counts reports (a caller driving
 * pt_trace_rays keeps that counter with pt_set_current_sample) and mu = l(colors.xyz):
 *   v = fmaxf(fmaf(-mu, mu, m2), 0.0f) / (float)(n - 1), +inf when n < 2
 * computed on the device (k_variance) into a 4 B/px buffer allocated on first use.  PT_EINVAL when the current frame is not
 * valid or has no samples (current_sample 0); any context, tiled ranks included (their local pixels). */
int pt_read_variance(pt_context* ctx, float* out, int64_t npix);
void* pt_device_variance(pt_context* ctx);                           /* the same, left on the device; NULL on failure (pt_last_error) */

/* ---- guide buffers and an edge-avoiding a-trous denoiser (new: the reference has no denoiser) ------------------------
 * Guide buffers ("AOVs") of the frame seen through cam.  Per local pixel, subpixels x subpixels (1..8) camera rays with the
 * sub-pixel offsets rnd1 = ((float)i + 0.5f) / (float)n, rnd2 = ((float)j + 0.5f) / (float)n fed to camera_get_ray
 * (prog.cl:82-92); no LCG draw.  Each ray follows at most specular_depth (0..16) mirror (type 1) / dielectric (type 2) hits
 * with the next ray shade_hit would build (flipped N, mirror direction, normalisation, +-0.001 offset); a dielectric refracts
 * iff disc > 0 and reflects otherwise, toggling `inside` as prog.cl:228-245 does; a mirror multiplies the running tint
 * (1,1,1 at first) by its F0, a dielectric leaves it.  The terminal hit (the first of any other type, or the one where the
 * depth runs out) gives albedo = tint x (kd + emission) (prog.cl:323-325; F0 at a terminal mirror, 1 at a terminal
 * dielectric) and its N flipped against the incoming ray; a miss anywhere on the chain gives albedo 0 and normal 0.
 * Per pixel, sub-pixels in raster order (j outer, i inner): albedo = sum / (float)(n*n); normal = sum s times
 * 1.0f / sqrtf((s.x*s.x + s.y*s.y) + s.z*s.z) (0 when s is 0); depth = the sum of the primary rays' t over the sub-pixels
 * that hit, / (float)hits, -1 when none hit.  Touches neither colors, rnds, rays nor current_sample, and is allowed while an
 * adaptive frame is held.  Any context (tiled ranks: their local pixels, at global pixel ids).  Arguments are checked
 * before the device: out-of-range ones give PT_EINVAL, a host-only context PT_ENODEVICE. */
int pt_render_aovs(pt_context* ctx, const pt_camera* cam, int32_t subpixels, int32_t specular_depth);
/* albedo_rgbm: {r, g, b, material index of the first sub-pixel's terminal hit or -1; lit guides: -2 - j where its chain ended on record
 * j of the area set}; normal_depth: {nx, ny, nz, depth};
 * 16 B each per local pixel, either pointer may be NULL */
int pt_read_aovs(pt_context* ctx, float* albedo_rgbm, float* normal_depth, int64_t npix);
/* Shaded guides (new: the guides of what pt_render_nee shades with under options "smooth_normals" and "textures").
 * pt_aov_defaults: subpixels 1, specular_depth 4, shading PT_AOV_GEOMETRIC.  pt_render_aovs_ex with PT_AOV_GEOMETRIC IS
 * pt_render_aovs(ctx, cam, subpixels, specular_depth): the same kernel instance, the same bits.  With PT_AOV_SHADED it follows the two
 * options as they are at the call, the way pt_render_nee does, and runs their lazy repack (k_pack_vertex_normals / k_pack_vertex_uvs,
 * the texture copies) on the context's stream first.  Sub-pixel rays, raster order, sums, normalisation, depth, the material index, the
 * miss rule and the layout are pt_render_aovs's; float32, fma where dot3 / cross3 / madd have it (the smooth-normals block above).
 * At every hit of a chain, with the ray (P, D) and the hit distance t:
 *   N = the record's normal, Ng = N flipped against the ray (dot3(D, N) > 0 ? -N : N), hp = madd(D, t, P);
 *   (Ns, kd') = the shading normal and the textured albedo of the two blocks above, from ONE evaluation of a1, a2, a3 (the device
 *   function shading_normal_albedo that k_nee calls); Ns = Ng, the same bits, when "smooth_normals" is off or the triangle has no vertex
 *   normals (or by the fall-backs of that block); kd' = kd, the same bits, when "textures" is off, nothing is bound, the triangle has
 *   no uvs or the type is not 0.
 * Specular step (type 1 or 2 at chain depth d < specular_depth), evaluated with X = Ns:
 *   w = D - (X * dot3(X, D)) * 2.0f; for type 2, n = the material's n (1.0f / n when inside), cosa = dot3(-D, X),
 *   disc = 1.0f - (fmaf(-cosa, cosa, 1.0f) / n) / n, and iff disc > 0 the step refracts: w = madd(X, cosa / n - sqrtf(disc), D / n);
 *   geometric side (the rule of the estimator, without the LCG draw): if dot3(w, Ng) <= 0 for a reflection or >= 0 for a refraction, the
 *   whole step -- direction, cosa, disc, the choice -- is evaluated again with X = Ng, and that evaluation stands;
 *   the next ray is D' = normalize(w) from hp + 0.001f Ng (reflection) or hp - 0.001f Ng (refraction); a mirror multiplies the tint by
 *   its F0, a refraction toggles `inside`, as in pt_render_aovs.
 * Terminal hit: albedo = tint x a with a = kd' + emission (type 0), kd + emission (type 3), F0 (a terminal mirror), 1 (a terminal
 * dielectric); the normal is Ns.
 * With both options off -- or on, with no vertex normals recorded and nothing bound -- the shaded guides are pt_render_aovs's bit for bit.
 * Touches neither colors, rnds, rays nor current_sample; allowed while an adaptive frame is held; any context (tiled ranks: their
 * local pixels, at global pixel ids).  PT_EINVAL, checked before the device (PT_ENODEVICE on a host-only context): params NULL,
 * subpixels outside 1..8, specular_depth outside 0..16, shading outside {0, 1}.
 * Consumers (pt_denoise, pt_denoise_variance, pt_temporal_accumulate, pt_denoise_temporal, pt_read_aovs) use whichever guides were
 * rendered last.  Shaded guides are a snapshot of the scene's shading data: pt_set_vertex_normals, pt_clear_vertex_normals,
 * pt_compute_vertex_normals, pt_set_vertex_uvs, pt_clear_vertex_uvs, pt_add_texture, pt_clear_textures and pt_set_material_texture make
 * them stale exactly as an upload does (the consumers return PT_EINVAL until guides are rendered again, and the first guides after that
 * drop the temporal history); geometric guides are not affected by those calls, and changing the two options invalidates neither. */
enum { PT_AOV_GEOMETRIC = 0, PT_AOV_SHADED = 1 };
/* Lit guides (new: opt-in with option "aov_lights" = 0 | 1, default 0; other values PT_EINVAL).  A guide call -- pt_render_aovs,
 * pt_render_aovs_ex with either shading -- renders lit guides iff, at the call, the option is on and the context holds an area set with a
 * non-black light (pt_set_area_lights; the condition that selects NEE family 12).  Otherwise it launches the kernel instances of before
 * and writes the same bits.  Stat "aov_lights": 1 iff the last guide launch used a lit instance, else 0.  pt_aov_params::shading stays
 * {0, 1}.  Everything not named here is pt_render_aovs / PT_AOV_SHADED as pinned above (sub-pixel rays, raster order, sums,
 * normalisation, layout).  The records are the set's table (spheres before suns, each kind in the order given; pt_debug_area_lights).
 * Sphere test, after EVERY closest-hit search of a chain (the primary ray and every ray after a specular step), with the ray (P, D) and
 *   t_tri = the triangle's distance or +inf on a miss: j = area_sphere_hit(set, P, D, t_tri, -1, &t_s), the nearest sphere with
 *   0 < t_s < t_tri whose outside holds P (an origin inside a sphere does not see it), in the operations of the area-light block.  If
 *   j >= 0 the chain ends on that sphere, whatever the triangle's type and however much specular depth is left:
 *   albedo = tint x L_j; normal = normalize3(madd(D, t_s, P) - C_j), the same in geometric and shaded guides; material = -2 - j (exact in
 *   float, distinct from a miss's -1).
 * Primary ray: a sphere that ends it makes it a hit -- t_s joins the depth sum and the hit count, also where no triangle was hit.
 * Miss with no sphere, anywhere on a chain: mask = area_sun_mask(set, D) (the suns with dot3(D, axis) >= cos a).  If it is non-zero:
 *   albedo = tint x the sum of L over the suns of the mask in ascending record order (from 0); normal 0; material = -2 - j of the lowest
 *   such record.  A primary ray that ends so is still a miss: it is left out of the hit count, and the depth is -1 when no sub-pixel hit.
 *   So the filters' hit / miss rule and step 1 of the temporal pass stay as pinned: a sun's disc gets no history and no depth edge.  With
 *   an empty mask the miss is what it was.
 * Consumers are unchanged and read whichever guides were rendered last.  Lit guides are a snapshot of the set: pt_set_area_lights and
 * pt_clear_area_lights make them stale exactly as an upload does (the consumers return PT_EINVAL until guides are rendered again, and the
 * first guides after that drop the temporal history); unlit guides are not affected by those two calls, and changing the option
 * invalidates nothing.  The lens, the fog and the interiors stay out of the guides. */
typedef struct { int32_t subpixels, specular_depth, shading; } pt_aov_params;
void pt_aov_defaults(pt_aov_params* p);
int pt_render_aovs_ex(pt_context* ctx, const pt_camera* cam, const pt_aov_params* params);
/* The filter (Dammertz et al. 2010, the spatial part of SVGF), L = iterations:
 *   x0 = c / max(a, 1e-3) per channel with demodulate (a: the guides' albedo), else c;
 *   iteration i = 0..L-1, step s = 2^i, taps q = p + s (dx, dy), dx, dy in -2..2; taps outside the frame are skipped:
 *     x(i+1)(p) = sum h wc wn wz x(i)(q) / sum h wc wn wz,  h = k[dx] k[dy], k = (1/16, 1/4, 3/8, 1/4, 1/16)
 *     wc = exp(-|x(i)(p) - x(i)(q)|^2 4^i / sigma_color^2)
 *     wn = max(0, n_p . n_q)^sigma_normal, 1 if either normal is 0
 *     wz = 1 if both primary rays miss, 0 if exactly one does, else exp(-|z_p - z_q| / (sigma_depth s max(|dx|,|dy|) z_p))
 *   the centre tap q = p weighs 9/64 (every term 1), so the denominator never vanishes; sigma = +inf turns its term off
 *   (weight 1), and so does sigma_normal = 0;
 *   output x(L) max(a, 1e-3) with demodulate, else x(L); .w = 1.
 * Float32 on the device (expf / powf), deterministic (no atomics): two runs give the same bits. */
typedef struct { int32_t iterations; float sigma_color, sigma_normal, sigma_depth; int32_t demodulate; } pt_denoise_params;
/* iterations 3, sigma_color 0.125, sigma_normal 8, sigma_depth 0.05, demodulate 1: the best value of every axis of the 16-spp
 * sweep of tools/denoise_bench.py at 1920x1080, 8 bounces -- the same on the Cornell box and on MESH-100k.  The RMSE gain is
 * small (3-4 %: caustic fireflies dominate the error), see profiles/denoise/README.md */
void pt_denoise_defaults(pt_denoise_params* p);
/* Filters the context's colors (the bound framebuffer, if any) with the last pt_render_aovs / pt_render_aovs_ex guides into a buffer
 * of its own; colors is never written.  World-1 contexts only.  PT_EINVAL without guides, after pt_upload_triangles /
 * pt_upload_materials (or, for shaded guides, an authoring call listed above) made them stale, for iterations outside 1..10 or negative / NaN sigmas.  Two launches' worth of
 * buffers (32 B/px) are allocated on first use. */
int pt_denoise(pt_context* ctx, const pt_denoise_params* p);
int pt_read_denoised(pt_context* ctx, float* out_rgba, int64_t npix);   /* float3 @ 16 B, colors' layout (row 0 = bottom) */
/* The variance-guided filter (the spatial part of SVGF, Schied et al. 2017) on the same guides, L = iterations:
 *   x0 = the colour, demodulated per channel as pt_denoise does when demodulate is set; v0 = pt_read_variance's v,
 *   / max(l(a), 1e-3)^2 with demodulate (l as pinned for the moments);
 *   taps, h, wn, wz, the hit / miss rule, the centre tap (every term 1) and the skipped out-of-frame taps are pt_denoise's; the
 *   luminance term replaces the colour term:
 *     g(p) = the 3x3 blur of v(i) with weights (1/4, 1/2, 1/4)^2, one pixel apart at every iteration, normalised over the in-frame taps
 *     wl = exp(-|l(x(i)(p)) - l(x(i)(q))| / (sigma_luminance sqrt(g(p)) + 1e-6)), 1 when the difference is 0, g(p) = +inf or
 *     sigma_luminance = +inf;
 *   x(i+1)(p) = sum w x(i)(q) / sum w,  v(i+1)(p) = sum w^2 v(i)(q) / (sum w)^2  (w = h wl wn wz; a tap of weight 0 adds nothing);
 *   output x(L), remodulated with demodulate; .w = v(L), times max(l(a), 1e-3)^2 with demodulate.
 * Float32 on the device, deterministic.  World-1 contexts only.  PT_EINVAL without guides or with stale ones, when the frame's moments
 * are not valid or it has no samples (pt_read_variance), for iterations outside 1..10 or negative / NaN sigmas.  The result is
 * read like pt_denoise's (pt_read_denoised / pt_device_denoised, the same two buffers); the variance read-out is refreshed. */
typedef struct { int32_t iterations; float sigma_luminance, sigma_normal, sigma_depth; int32_t demodulate; } pt_denoise_variance_params;
/* iterations 2, sigma_luminance 4, sigma_normal 8, sigma_depth 0.05, demodulate 0: normal and depth as pt_denoise; the rest from the
 * 16-spp sweep of tools/denoise_variance_bench.py at 1920x1080 on the Cornell box and MESH-100k, the best sum of the two RMSE ratios
 * to raw (0.35 and 0.74).  Demodulation loses on both: a dark albedo (clamped at 1e-3) scales the pixel and its variance up, and the
 * luminance term then lets it spread (profiles/denoise/README.md) */
void pt_denoise_variance_defaults(pt_denoise_variance_params* p);
int pt_denoise_variance(pt_context* ctx, const pt_denoise_variance_params* p);
void* pt_device_denoised(pt_context* ctx);                               /* NULL until pt_denoise ran */

/* ---- temporal accumulation with reprojection (new: the temporal part of SVGF; the reference restarts at every camera move) -----
 * pt_temporal_accumulate blends the current frame into a history kept by the context, reprojected from the view the history was made
 * in.  Per local pixel p of the frame seen through cam (the camera its launches and its guides used), with the guides of the last
 * pt_render_aovs, float32 on the device (one lane per pixel, k_temporal), in this order:
 *   1. depth < 0 (the primary ray missed): no history.
 *   2. X = fmaf(depth, D, eye), D = the direction camera_get_ray(p, cam, 0.5f, 0.5f) gives (normalize3: d times 1.0f / sqrtf(d.d)).
 *   3. v = X - eye_prev, ahead = lookat_prev - eye_prev; by Cramer's rule with triple products (dot / cross with fmaf as the kernels'
 *      dot3 / cross3): det = ahead.(right x up), a = v.(right x up) / det, b = ahead.(v x up) / det, c = ahead.(right x v) / det
 *      (right, up: prev's).  a <= 0 (X behind prev) or not finite: no history.  u = b / a, w = c / a,
 *      x' = ((u + 1) XM) 0.5 - 0.5, y' = ((w + 1) YM) 0.5 - 0.5: continuous coordinates relative to pixel centres, row 0 at the bottom.
 *   4. x0 = floorf(x'), fx = x' - x0 (same for y); fx < 2^-10 -> fx = 0; fx > 1 - 2^-10 -> fx = 0 and x0 + 1.  Taps q in the order
 *      (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), weights (1 - fx)(1 - fy), fx (1 - fy), (1 - fx) fy, fx fy; a tap of
 *      weight 0 is neither read nor tested (a camera at rest reads exactly one tap: the pixel itself).
 *   5. q is valid iff it is in the frame, depth_q > 0, material_q == material_p, the normals agree (both 0: yes; exactly one 0: no;
 *      else dot(n_p, n_q) >= normal_cos) and |sqrtf(v.v) - depth_q| <= depth_tolerance depth_q (q's values: the previous set's guides).
 *   6. W = sum of the valid taps' weights (in tap order); W < 0.01: no history; else colour_h, m2_h, n_h = sum fmaf(value_q, w_q, .) / W.
 *   Blend, counted in samples: k = the frame's samples at p (pt_read_sample_counts), n_h' = min(n_h, max_history); n_h' = 0 (no
 *   history, or max_history = 0: how a caller restarts) -> the frame's own .xyz and .w bit for bit and n = k; else n = n_h' + k,
 *   c = fmaf(n_h', c_h, k c_frame) / n per channel, the same for m2.  v = fmaxf(fmaf(-l(c), l(c), m2), 0) / (n - 1), +inf when n < 2
 *   (pt_read_variance's read-out with a fractional n).  The result (c, m2, n and the guides it was made with: 40 B/px) becomes the
 *   history, cam its camera.  Two history sets (80 B/px) and the variance (4 B/px) are allocated on first use; nothing is copied.
 * World-1 contexts only.  Checked in this order: arguments (max_history >= 0, normal_cos in [-1, 1], depth_tolerance >= 0, none NaN)
 * and world, PT_EINVAL; the device, PT_ENODEVICE; then PT_EINVAL without guides or with stale ones, when the frame's moments are not
 * valid or it has no samples (pt_read_variance's rule), when a launch of the frame used a camera that differs in any byte from the one
 * it started with, when the guides' camera differs from the frame's, and when this frame was already accumulated.
 * pt_upload_triangles / pt_upload_materials drop the history: the next accumulate gives n = k everywhere. */
typedef struct { int32_t max_history; float normal_cos, depth_tolerance; } pt_temporal_params;
/* max_history 64, normal_cos 0.9, depth_tolerance 0.02: from the sweep of tools/temporal_bench.py at 1920x1080, 8 bounces, 16 frames of
 * 4 spp on the Cornell box and MESH-100k.  64 has the best sum of the two RMSE ratios to raw (0.235 + 0.501); normal_cos and
 * depth_tolerance move them by less than 0.3 % over 0.8-0.95 and 0.01-0.05, so the stricter trial values stay
 * (profiles/temporal/README.md) */
void pt_temporal_defaults(pt_temporal_params* p);
int pt_temporal_accumulate(pt_context* ctx, const pt_temporal_params* p);
/* the last accumulate's result: rgbv {r, g, b, v} 16 B per local pixel, n the samples behind it (float: bilinear histories are
 * fractional); either pointer may be NULL */
int pt_read_temporal(pt_context* ctx, float* rgbv, float* n, int64_t npix);
void* pt_device_temporal(pt_context* ctx);      /* that colour on the device: {r, g, b, m2} 16 B per local pixel; NULL before an accumulate */
/* pt_denoise_variance's filter (same parameters, same guides, same output: pt_read_denoised / pt_device_denoised) run on the last
 * accumulate's colour and variance instead of colors and pt_read_variance's.  PT_EINVAL unless an accumulate ran on the current guides. */
int pt_denoise_temporal(pt_context* ctx, const pt_denoise_variance_params* p);
/* host only: steps 2-3 for pixel (x, y) of cur at depth into prev: out = {x', y', sqrtf(v.v)}; PT_EINVAL when a <= 0 */
int pt_debug_reproject(const pt_camera* cur, const pt_camera* prev, int32_t x, int32_t y, float depth, float out[3]);

/* ---- variance-gated firefly filter (new: a post-process stage between a frame, or a temporal result, and the variance-guided filter;
 * the estimator is untouched) -----
 * pt_despeckle finds pixels whose luminance stands out of a robust statistic of their neighbourhood, confirms them with the pixel's
 * own variance (a converged small highlight has a small relative variance, a firefly a relative standard deviation of about 1), scales
 * them down to the limit and, with spread on, hands the removed energy to the window around them, so the frame's sum is kept.
 * Input per pixel p = (x, y) of a W x H frame, index y W + x: colour c(p) and the variance of the mean luminance v(p), >= 0 or +inf.
 * All arithmetic float32, fmaf where written (kernel k_despeckle):
 *   1. l(p) = fmaf(0.0722f, b, fmaf(0.7152f, g, 0.2126f * r)) (the l pinned for the moments).  p is live iff l(p) is finite.  A pixel
 *      that is not live is copied through bit for bit, colour and v, and gets flag 2; it is treated as outside the frame everywhere
 *      below: nobody's neighbour, not counted, gives nothing and receives nothing.
 *   2. The neighbours of p: the live in-frame q != p with |dx|, |dy| <= radius; K(p) their number; m(p) the rank-th largest l(q) among
 *      them, counted with multiplicity, the smallest of them when K < rank; T(p) = fmaf(threshold, m(p), floor).
 *   3. p is flagged (flag 1) iff it is live, K > 0, l(p) > T(p) and the variance gate passes: min_rel_sigma == 0, or v(p) == +inf, or
 *      v(p) >= (min_rel_sigma * l(p)) * (min_rel_sigma * l(p)).
 *   4. Flagged: s = T / l (IEEE divide), c' = c * s, e = c - c' per channel, v' = +inf if v == +inf, else (v * s) * s.  Not flagged:
 *      c' = c, e = 0, v' = v.
 *   5. spread == 0: the output is c', v'.
 *   6. spread == 1: n(p) = the live in-frame pixels with |dx|, |dy| <= radius, p included; share(p) = e(p) / (float)n(p) per channel.
 *      For every live q, over p = q + (dx, dy) in raster order (dy outer from -radius, dx inner, the centre included), flagged p only:
 *      acc_c += share(p), acc_v = fmaf(ls, ls, acc_v) with ls = l(share(p)), both from 0.  The output is c'(q) + acc_c, v'(q) + acc_v.
 *      A flagged pixel receives its own share.  The excess counts as a one-sample event, so its variance is its square: the luminance
 *      term of the filter that follows is loose where energy landed, and spreads it further.  Windows are symmetric over live pixels,
 *      so the sum of the output is the sum of c up to rounding.
 * No atomics, deterministic: two runs give the same bits.  The result does not depend on how the kernel tiles the frame. */
typedef struct { int32_t source, radius, rank; float threshold, floor, min_rel_sigma; int32_t spread; } pt_despeckle_params;   /* 28 bytes */
enum { PT_DESPECKLE_FRAME = 0, PT_DESPECKLE_TEMPORAL = 1 };
/* source FRAME, radius 2, rank 2, threshold 4, floor 0, min_rel_sigma 0.5, spread 1: trial values, not yet replaced by the best point
 * of the sweep of tools/despeckle_bench.py (profiles/despeckle/README.md) */
void pt_despeckle_defaults(pt_despeckle_params* p);
/* Source PT_DESPECKLE_FRAME reads colors (the bound framebuffer, if any) and pt_read_variance's v; PT_DESPECKLE_TEMPORAL the last
 * pt_temporal_accumulate's colour and variance.  It needs no guides.  The result goes to a buffer of its own (colour + variance, the
 * variance once more for the filter, flags: 24 B/px, allocated on first use); colors, rnds, the denoised buffers and the temporal sets
 * are never written, and the variance read-out is refreshed as by pt_read_variance.  World-1 contexts only.  Checked in this order:
 * PT_EINVAL for params NULL, radius or rank outside 1..3, threshold < 1, floor < 0, min_rel_sigma < 0 (or any of them NaN), spread or
 * source outside {0, 1}, and world; PT_ENODEVICE on a host-only context; then PT_EINVAL under the source's rule: pt_read_variance's
 * (moments not valid, no samples) for FRAME, no accumulate yet for TEMPORAL. */
int pt_despeckle(pt_context* ctx, const pt_despeckle_params* p);
/* the last pt_despeckle's result: rgbv {r, g, b, v} 16 B per local pixel, flags 0 / 1 / 2; either pointer may be NULL */
int pt_read_despeckled(pt_context* ctx, float* rgbv, int32_t* flags, int64_t npix);
void* pt_device_despeckled(pt_context* ctx);    /* {r, g, b, v} 16 B per local pixel on the device; NULL before the first pt_despeckle */
/* pt_denoise_variance's filter (same parameters, same guides, same output: pt_read_denoised / pt_device_denoised) run on the despeckled
 * colour and variance, as pt_denoise_temporal runs it on the temporal result.  PT_EINVAL under the filter's rules (parameters, guides),
 * without a despeckled result, and when the result is stale: a launch has written colors or a frame has started since, a newer
 * accumulate ran (source TEMPORAL), or the scene was uploaded. */
int pt_denoise_despeckled(pt_context* ctx, const pt_denoise_variance_params* p);
/* the same kernel on a caller's frame rgbv_in ({r, g, b, v} per pixel, 1 <= w, h <= 4096) -> rgbv_out, flags; source is ignored, the
 * other parameters are checked as above (PT_EINVAL before PT_ENODEVICE) */
int pt_debug_despeckle(pt_context* ctx, const float* rgbv_in, int32_t w, int32_t h, const pt_despeckle_params* p, float* rgbv_out, int32_t* flags);

/* ---- display stage (new: a post-process from any of the four HDR results to an LDR image, on the device, no host round trip; the
 * path-tracing kernels, the estimator, pt_resolve_ldr and pt_write_ppm are untouched) -----
 * pt_display meters an exposure, adds bloom, applies a tone curve and an encoding, and writes {r, g, b, 1} per pixel plus three bytes per
 * pixel in PPM row order.  Input: a W x H frame, colour c(p) = .xyz, index y W + x, row 0 the bottom of the view.  All arithmetic float32;
 * products and sums are rounded one by one (no fused multiply-add) except where fmaf is written (kernels in pt_display.hip):
 *   0. l(p) = fmaf(0.0722f, b, fmaf(0.7152f, g, 0.2126f * r)) (the l pinned for the moments).  p is live iff r, g, b and l are all finite.
 *      A pixel that is not live takes no part in metering or bloom, is written as {0, 0, 0, 1} with bytes 0, and is counted in n_nonfinite.
 *   1. Exposure E.  A 256-bin histogram of the live pixels is always taken: l < 2^-16 (zero, negatives) counts in n_dark and in no bin;
 *      otherwise bin = min((bits(l) >> 20) - 888, 255): eight bins per stop from 2^-16 to 2^16, everything brighter in bin 255.  Counts
 *      are uint32.  N = sum of the bins; lo = N low_permille / 1000, hi = N high_permille / 1000 (uint64, integer division); walking the
 *      bins upward, k_b = the samples of bin b with rank in [lo, hi); K = sum k_b; S = fmaf((float)k_b, lambda_b, S) over b ascending
 *      from S = 0, lambda_b = (float)((b >> 3) - 16) + T[b & 7], T = PT_DISPLAY_LOG2_TABLE; M = S / (float)K (0 when K = 0).
 *      PT_METER_MANUAL: E = exp2f(ev).  PT_METER_AUTO: E* = key * exp2f(ev - M), clamped to [exp2f(min_ev), exp2f(max_ev)]; E* =
 *      exp2f(ev) when K = 0.  The context remembers the E of its last pt_display; with a remembered E_prev and adapt < 1,
 *      E = exp2f((1 - adapt) * log2f(E_prev) + adapt * log2f(E*)), else E = E*.  pt_display_reset, pt_upload_triangles and
 *      pt_upload_materials forget E_prev.  The reduction runs on the device; the later kernels read E from device memory.
 *   2. Bloom, skipped entirely (no launches, out = h bit for bit) when bloom_intensity = 0.  h(p) = E * c(p) for a live p, else 0;
 *      lh = l(h); bright pass B(p) = (h * (lh - threshold)) / lh per channel if lh > threshold, else 0.  Level sizes W_0 = W,
 *      W_k = (W_(k-1) + 1) / 2, the same for H.  Down, k = 1 .. levels, D_0 = B:
 *      D_k(x, y) = sum_j a_j (sum_i a_i D_(k-1)(clamp(2x - 1 + i), clamp(2y - 1 + j))), i, j = 0..3 ascending, a = {1, 3, 3, 1} / 8,
 *      coordinates clamped to the source level.  Up, separable: target x reads s = x >> 1 with weight 0.75 and s + (x odd ? 1 : -1),
 *      clamped to the source level, with weight 0.25; rows first, then the two rows the same way.  U_levels = D_levels,
 *      U_k = D_k + up(U_(k+1)) for k = levels - 1 .. 1; out(p) = h(p) + (bloom_intensity / (float)levels) * up(U_1)(p).
 *      The result does not depend on how a kernel tiles a level.
 *   3. Curve per channel on x = out > 0 ? out : 0.  PT_CURVE_LINEAR: x.  PT_CURVE_REINHARD: x * ((1 + L / (white * white)) / (1 + L)),
 *      L = l(x) (no division by L: black stays black; white = +inf: 1 / (1 + L)).  PT_CURVE_ACES: (x (2.51 x + 0.03)) / (x (2.43 x + 0.59) + 0.14).
 *      Then v = the curve clamped to [0, 1] (a NaN, which only an overflow of E c or of the curve's squares can give, becomes 0), then
 *      PT_ENCODE_SRGB: 12.92 v below 0.0031308, else 1.055 powf(v, 1 / 2.4f) - 0.055; PT_ENCODE_LINEAR: v.
 *      Written: {r, g, b, 1} per pixel in the frame's order, and bytes (uint8)floorf(255 v + 0.5) r, g, b per pixel, top row first. */
typedef struct {
    int32_t source, metering; float ev, key; int32_t low_permille, high_permille; float min_ev, max_ev, adapt;
    int32_t bloom_levels; float bloom_threshold, bloom_intensity; int32_t curve; float white; int32_t encoding;
} pt_display_params;   /* 60 bytes */
enum { PT_DISPLAY_FRAME = 0, PT_DISPLAY_DENOISED = 1, PT_DISPLAY_TEMPORAL = 2, PT_DISPLAY_DESPECKLED = 3 };
enum { PT_METER_MANUAL = 0, PT_METER_AUTO = 1 };
enum { PT_CURVE_LINEAR = 0, PT_CURVE_REINHARD = 1, PT_CURVE_ACES = 2 };
enum { PT_ENCODE_SRGB = 0, PT_ENCODE_LINEAR = 1 };
/* T[j] = log2(1 + (j + 0.5) / 8) rounded to float32: the centre of the j-th eighth of a stop */
#define PT_DISPLAY_LOG2_TABLE { 0.0874628425f, 0.247927517f, 0.392317414f, 0.523561954f, 0.643856168f, 0.754887521f, 0.857980967f, 0.954196334f }
/* {E, M, K, n_dark, n_nonfinite, bloom levels actually run (0 when bloom_intensity = 0)} of the last pt_display */
struct pt_display_info { float exposure, mean_log2; uint32_t n_metered, n_dark, n_nonfinite; int32_t levels; };   /* 24 bytes */
/* source FRAME, metering AUTO, ev 0, key 0.18, permille 100 / 950, ev range -16 .. 16, adapt 1, 4 levels, threshold 1, intensity 0,
 * curve ACES, white +inf, encoding sRGB: trial values, not yet replaced by a sweep over rendered scenes (profiles/display/README.md) */
void pt_display_defaults(pt_display_params* p);
/* Source PT_DISPLAY_FRAME reads colors (the bound framebuffer, if any), DENOISED what pt_read_denoised serves, TEMPORAL what
 * pt_read_temporal serves, DESPECKLED what pt_read_despeckled serves (.xyz of each).  The stage writes only its own buffers (allocated on
 * first use: 19 B/px for the result, 64 / 3 B/px for the pyramid once bloom runs); colors, rnds, the guides, the denoised buffer, the
 * temporal sets and the despeckled result are never written.  It does not synchronise with the host.  World-1 contexts only.  Checked
 * in this order: PT_EINVAL for params NULL; source, metering, curve or encoding out of range; a NaN in any float; key <= 0; permille
 * outside 0 <= low < high <= 1000; min_ev > max_ev; adapt outside (0, 1]; bloom_levels outside 1..6; bloom_threshold < 0;
 * bloom_intensity < 0; white <= 0; world != 1.  Then PT_ENODEVICE on a host-only context.  Then PT_EINVAL under the source's own rule:
 * pt_denoise / pt_temporal_accumulate / pt_despeckle has not run (FRAME is always there). */
int pt_display(pt_context* ctx, const pt_display_params* p);
/* the last pt_display's result: rgba {r, g, b, 1} 16 B per pixel (row 0 = bottom), rgb8 3 B per pixel (top row first); either may be NULL */
int pt_read_display(pt_context* ctx, float* rgba, uint8_t* rgb8, int64_t npix);
void* pt_device_display(pt_context* ctx);       /* the float4 result on the device, the bytes right behind it; NULL before the first pt_display */
/* the numbers of the last pt_display; this is where a host that wants them synchronises */
int pt_display_info(pt_context* ctx, struct pt_display_info* out);
int pt_debug_display_histogram(pt_context* ctx, uint32_t out[256]);     /* the last pt_display's 256 bins */
int pt_display_reset(pt_context* ctx);          /* forgets the remembered exposure: the next pt_display adapts from nothing */
/* the last pt_display's bytes as a binary P6 file with pt_write_ppm's conventions (maxval 255, top row first) */
int pt_write_display_ppm(pt_context* ctx, const char* path);
/* the same kernels on a caller's frame rgba_in ({r, g, b, .} per pixel, 1 <= w, h <= 4096); source is ignored, the other parameters are
 * checked as above (PT_EINVAL before PT_ENODEVICE); prev_exposure > 0 stands in for the remembered exposure, <= 0: none; the context's
 * own is neither read nor written.  Any of rgba_out, rgb8_out, hist (256 bins) and info may be NULL. */
int pt_debug_display(pt_context* ctx, const float* rgba_in, int32_t w, int32_t h, const pt_display_params* p, float prev_exposure,
                     float* rgba_out, uint8_t* rgb8_out, uint32_t* hist, struct pt_display_info* info);

/* ---- multi-GPU frame assembly (SURVEY 8b "RCCL communicator per context", 8e) ----------
 * The reference is single-device (main.cpp:466-476); a host that tiles the frame over N contexts with
 * pt_create_tiled assembles it with these.  One process (or thread) per GPU:
 *   rank 0: pt_comm_unique_id(id); every rank receives the 128 bytes by the host's own means (MPI,
 *   a file, torch.distributed ...); every rank: pt_comm_init(ctx, id); after rendering, every rank:
 *   pt_gather_frame(ctx) -- ONE ncclAllGather of the ranks' radiance slabs over RCCL/xGMI on the context's
 *   stream + a de-interleave kernel -- leaves the whole width x height frame (float3 @ 16 B, global pixel
 *   order) in device memory on every rank.  world = 1 needs no communicator.
 * The gathered frame is served (pt_device_frame, pt_read_frame, pt_write_*) only until the next call that renders: after
 * that a one-rank context serves its colors buffer (which IS the frame) and a tiled context returns NULL / PT_EINVAL
 * until pt_gather_frame has run again -- never a frame older than colors. */
#define PT_COMM_ID_BYTES 128
/* PT_OK if librccl could be bound in this process (dlopen + the five entry points), PT_ECOMM otherwise (pt_last_error(NULL)
 * says why).  Touches no collective: every rank can ask BEFORE any of them enters ncclCommInitRank, so that a rank that cannot
 * take part is found while the others can still be told (a rank missing from ncclCommInitRank blocks all the others). */
int pt_comm_available(void);
int pt_comm_unique_id(void* id128);                                  /* ncclGetUniqueId */
int pt_comm_init(pt_context* ctx, const void* id128);                /* ncclCommInitRank(world, id, rank) of pt_create_tiled */
int pt_gather_frame(pt_context* ctx);
void* pt_device_frame(pt_context* ctx);                              /* the assembled frame (world = 1 without a fresh gather: the colors buffer); NULL if stale */
int pt_frame_size(const pt_context* ctx, int32_t* width, int32_t* height, int64_t* npix);
int pt_read_frame(pt_context* ctx, float* out_rgba, int64_t npix);   /* npix = width * height of the GLOBAL frame */

/* ---- image files: what the reference shows through its GL blit, main.cpp:1019-1039 -------
 * PFM = the HDR `colors` (the parity target) of the assembled frame; PPM = an LDR resolve (`which` as in
 * pt_resolve_ldr; the tone map's NaN for black pixels, prog.cl:265-267, is written as 0), world = 1 only.
 * The pt_image_* forms write a caller-supplied host buffer (float3 @ 16 B, row 0 = bottom of the view). */
int pt_write_pfm(pt_context* ctx, const char* path);
int pt_write_ppm(pt_context* ctx, const char* path, int32_t which);
int pt_image_write_pfm(const char* path, const float* rgba, int32_t width, int32_t height);
int pt_image_write_ppm(const char* path, const float* rgba, int32_t width, int32_t height);
/* Reads what pt_image_write_pfm writes ("PF" colour or "Pf" grey, either byte order): *width, *height from the header; with rgba_out
 * != NULL the pixels in the file's row order (the writer's: row 0 = bottom; flip the rows for a map whose row 0 is the +y pole),
 * float3 @ 16 B with .w = 0; cap = the pixels rgba_out holds (PT_EINVAL when too small).  PT_EIO: unreadable, mis-headed or truncated */
int pt_image_read_pfm(const char* path, float* rgba_out, int64_t cap, int32_t* width, int32_t* height);
/* Reads a binary PPM (P6; `#` comments in the header; maxval 1..65535, two-byte samples big-endian above 255): *width, *height from the
 * header; with rgb_out != NULL the pixels top row first as 3 floats each, sample / maxval (a float division), no colour transform; cap =
 * the pixels rgb_out holds (PT_EINVAL when too small).  PT_EIO: unreadable, mis-headed or truncated */
int pt_image_read_ppm(const char* path, float* rgb_out, int64_t cap, int32_t* width, int32_t* height);

/* ---- plumbing: device memory, streams, options, statistics --------------------------- */
/* Use caller-owned device buffers (e.g. torch tensors) for colors (16 B/px) and rnds (4 B/px)
 * of the LOCAL pixels; current contents are copied in.  NULL keeps the internal buffer.  In a tiled
 * context the colors buffer must hold pt_slab_pixel_count() pixels (the largest rank's count: the
 * all-gather sends equal slabs). */
int pt_bind_framebuffer(pt_context* ctx, void* d_colors, void* d_rnds);
void* pt_device_colors(pt_context* ctx);
void* pt_device_rnds(pt_context* ctx);
int pt_set_stream(pt_context* ctx, void* hip_stream);                /* hipStream_t; NULL = default stream */
/* options (key, value):
 *   "variant"      0 megakernel (default), 1 wavefront (stream-compacted, path state in HBM)
 *   "bvh_policy"   WHICH tree: 0 binned SAH with SAH leaf termination (default), 2 / 3 the same with every subtree of <= 4 /
 *                  <= 8 triangles forced into a leaf, 4 Morton order + PLOC merges (device only, a cheaper and worse tree),
 *                  5 = 0 built on the device whatever the scene size; set before the triangles are uploaded
 *   "bvh_device"   WHERE the SAH tree of policies 0..3 is built -- the result is the same, node for node: -1 (default) on the
 *                  device for scenes of >= 16,384 triangles, 0 on the host, 1 on the device.  The host builds whatever the
 *                  device hands back (non-finite triangles, ranges that need the median split)
 *   "sah_grain"    device SAH builder: ranges of at most this many triangles are finished by one wave each (default 256; 8..65536)
 *   "wide_on_device" device-built trees: 1 (default) the 4-wide collapse runs on the device too (the same nodes), 0 on the host
 *   "lds_scene"    2 (default) every workgroup stages BVH nodes in LDS: the whole tree when it fits (<= 64 KB,
 *                  <= 4096 triangles), otherwise its top if "treelet" asks for one (else the nodes are read through
 *                  L1/L2, see "wide_nodes"); 0 every node through L1/L2
 *   "treelet"      nodes of a LARGE tree to stage in LDS (the ones with the biggest boxes, renumbered to the front):
 *                  0 (default) none -- slower than 4-wide nodes through L1/L2 --, -1 what fits next to one
 *                  1,024-thread workgroup's stacks (~750-1,000), 2..2048; set before the triangles are uploaded
 *   "schedule"     megakernel: 1 a lane whose path ended starts its next sample at once and the wave leaves a traversal
 *                  when at most "suspend_lanes" lanes are unfinished (they resume in the next trip); 0 lockstep: all
 *                  lanes of a wave start a sample together; 2 like 1, and a lane whose pixel has had its samples of the
 *                  wave's work item moves on to its pixel of the wave's next item instead of waiting for the item's
 *                  slowest pixel (persistent launches; "migrate_lanes": how many such lanes must have gathered, default 1);
 *                  -1 (default) by tiles per resident wave: from 3 (one or two GPUs at 1080p) 2 -- for a tree in LDS only from
 *                  64 samples per launch, below that 1 --, else 0
 *   "suspend_lanes" -1 (default: 16 for a tree in LDS, else 24), 0..63
 *   "chunk_taper"  persistent launches with chained passes: > 0 the last "chunk_spp" samples of a launch are cut in halves down
 *                  to this many (64 samples in passes of 32, taper 8: 32, 16, 8, 8), so that the launch ends on short work items;
 *                  0 all passes "chunk_spp" long; -1 (default) 8 / 4 under schedule 2 from 64 / 32 samples per launch, else 0
 *   "lbvh_cluster" device-built trees (bvh_policy 4): the top of the tree above clusters of at most this many triangles is
 *                  rebuilt with the host's SAH over the cluster boxes (default 64; 0: the LBVH as the device built it);
 *                  set before the triangles are uploaded
 *   "build_threads" host SAH builder: 0 (default) as many threads as the machine has (at most 16), 1..256; the tree is
 *                  the same, node for node, for any number
 *   "wide_nodes"   trees read from global memory as 4-wide nodes with 8-bit child boxes (one 64-byte fetch decides two
 *                  BVH2 levels): 1 (default) when the tree does not fit LDS, 0 never, 2 every tree; set before the
 *                  triangles are uploaded
 *   "wide_lds_entries" 4-wide traversal: per-lane stack entries kept in LDS (default 20; the rest of the worst case lives in
 *                  global memory and is touched only by rays that get there); even, 4..20; set before the triangles are uploaded
 *   "waves_per_simd" kernels that read nodes from global memory: register budget for 4, 5, 6 or 7 resident waves per SIMD
 *                  (128 / 96 / 80 / 72 VGPRs); -1 (default) the most that the per-lane stacks in LDS leave room for
 *   "persistent"   1 (default) megakernel grid only fills the chip and every wave pulls its next 8x8
 *                  tile from a global counter; 0 one workgroup per group of tiles
 *   "chunk_spp"    persistent megakernel work items: n > 0 (pass, tile) items of n samples, chained per tile
 *                  through memory inside ONE launch; 0 whole tiles; -1 (default) by tiles per resident wave: 32 from 5
 *                  (64 when a launch has >= 256 samples), 16 from 3, 8 above 1.5, otherwise whole tiles
 *   "sah_visit_cost"  SAH price of one node visit in tenths of a triangle test (default 10; set before
 *                  the triangles are uploaded.  Measured: 5 / 10 / 15 / 20 -> 1006 / 1448 / 1393 / 1266 Msamples/s)
 *   "cost_binning" 0/1 wavefront: separate ray streams for rays touching a complex object's box
 *   "moments"      0 (default) / 1 fold each sample's squared luminance into colors[].w (pt_read_variance)
 *   "timing"       0/1 record HIP events around the dominant kernel ("kernel_ms" statistic)
 *   "count_work"   0/1 also count node visits / triangle tests (slower kernel instance)
 *   "reset_stats"  1 zero all statistics
 *   "debug_repeat" 0..1000 extra timed launches in pt_debug_closest_hit */
int pt_set_option(pt_context* ctx, const char* key, int64_t value);
/* stats: "segments" path segments executed since the last reset, "samples", "kernel_ms" (sum of
 * HIP-event durations of the dominant kernel), "kernel_launches", "bvh_nodes", "bvh_depth", "stack_entries"
 * (per-lane BVH2 traversal stack: deepest interior node + 2), "bvh_build_ms" (pt_upload_triangles as a whole),
 * "bvh_on_device", "bvh_median_splits" (ranges the host builder split at the median in the last pt_upload_triangles --
 * coincident centroids, a cost that is not finite, or a depth the traversal stack could not take; the device SAH builder
 * hands such a scene back to the host, so the count is 0 whenever "bvh_on_device" is 1), "triangles", "lds_bytes",
 * "waves_per_simd", "node_mode" (0 whole tree in LDS, 1 BVH2 nodes through L1/L2, 2 treelet, 3 4-wide nodes through
 * L1/L2), "nee_family" / "nee_form" / "nee_block" (what the last launch of
 * pt_render_nee or of an NEE round of pt_render_adaptive_ex took: the kernel family 0..10 -- plain, smooth, tex, glossy,
 * coated, lens, frosted, lights, medium, grid (a medium with a live density grid), interior (a material holds an interior) --, the form -- bit 0 an environment is drawn, bit 1 tiled -- and the workgroup
 * size; -1 each before the first such launch), "treelet_nodes", "wide_nodes" (how many 4-wide nodes),
 * "wide_pending" (their worst-case stack), "flat_triangles", "flat_boxes" (their distinct bounding boxes), "obj_pieces" (into how
 * many pieces the last pt_add_obj cut its file for the parallel parse; 0 before the first), and with
 * count_work: "node_visits", "tri_tests", "wave_node_steps", "wave_tri_steps", "tile_lane_steps", "wave_shade_steps",
 * "wave_trips", "wave_rounds" */
int pt_get_stat(pt_context* ctx, const char* key, double* out);

/* ---- introspection for tests (host data; no device work) ----------------------------- */
/* Packed BVH as uploaded: nodes (64 B each), triangle packets (48 B each), per-triangle
 * {rank, mati} pairs, and the add-order index of every packed triangle. */
int pt_debug_bvh_sizes(const pt_context* ctx, int64_t* nnodes, int64_t* ntris);
int pt_debug_bvh_copy(const pt_context* ctx, float* nodes, float* tris, int32_t* meta, int32_t* orig);
/* the 4-wide quantised nodes built from that tree (64 B each: {origin.xyz, exponents | nchild << 24}, {qlo_x, qhi_x,
 * qlo_y, qhi_y}, {qlo_z, qhi_z, -, -}, {4 child references}); *count = how many there are (0: not built), at most
 * `capacity` are copied */
int pt_debug_wide_nodes(const pt_context* ctx, void* out, int64_t capacity, int64_t* count);
/* The big-triangle list as the traversal tests it (stat "flat_triangles" entries, in packed order): packets = 12 floats each,
 * {r1, r2, r3, N} -- the packed triangle with its corners possibly rotated cyclically, never anything else; bit i of *pair_mask
 * = entries i and i + 1 are the halves of one wall (same N words, same r1 words) and are tested in one evaluation. */
int pt_debug_flat_list(const pt_context* ctx, float* packets, uint32_t* pair_mask);
/* Closest hit of n caller-supplied rays through the device traversal (kd_intersect, prog.cl:144-184):
 * out_t[i] = t (-1 on a miss), out_tri[i] = add-order index of the triangle hit (-1 on a miss). */
int pt_debug_closest_hit(pt_context* ctx, const pt_ray* rays, int64_t n, float* out_t, int32_t* out_tri);
/* The IEEE divide / sqrt fast paths of the render kernels against the compiler's expansions, on the device of ctx:
 * inputs first .. first + n - 1 of enumeration fn (PT_MATH_SQRT, PT_MATH_RSQRT: x = the input's low 32 bits as a float;
 * PT_MATH_DIV_GRID: a / b over every exponent pair, 8 mantissas each (0, 1, 2, half, max - 1, max, 2 hashed) and 4 sign pairs,
 * input k = ea | eb << 8 | ia << 16 | ib << 19 | signs << 22, 2^24 in all; PT_MATH_DIV_RANDOM: hashed bit patterns;
 * PT_MATH_DIV_NORMAL: hashed normal pairs with exponents -63 .. 63).  out[0] = inputs whose result differs in any bit
 * (or whose window admits a zero, denormal, inf or NaN), out[1] = inputs inside the fast path's window, out[2] = out[0];
 * bad[2 j], bad[2 j + 1] = the bit patterns (x or a, b) of up to bad_cap of the mismatching inputs.
 * PT_MATH_LCG: the device LCG (prog.cl:72-77) on seed = the input's low 32 bits as an int32: the new seed and the float it returns
 * against n = (uint64)(int64)seed * 48271 % 2147483647 written out with a 64-bit multiply and remainder, (float)n / 2147483648.0f;
 * "inside the window" = seed >= 0, the seeds that take the hand-reduced Mersenne path; bad[2 j] = the seed, bad[2 j + 1] = the new
 * seed the device gave. */
enum { PT_MATH_SQRT = 0, PT_MATH_RSQRT = 1, PT_MATH_DIV_GRID = 2, PT_MATH_DIV_RANDOM = 3, PT_MATH_DIV_NORMAL = 4, PT_MATH_LCG = 5 };
int pt_debug_math(pt_context* ctx, int32_t fn, int64_t first, int64_t n, int64_t out[3], uint32_t* bad, int64_t bad_cap);
/* The spec math and sampling primitives of the render kernels on caller-supplied items, so that each can be
 * compared bit for bit with its counterpart in the CPU oracle without a render.  `in` holds n items of a fixed number of 32-bit words
 * (floats as their bit patterns), `out` receives a fixed number of words per item; every fn calls the device function the kernels
 * call and restates nothing:
 *   fn                                      words in                         words out
 *   PT_SPEC_SINCOS, PT_SPEC_SINCOS_SK       1: theta                         2: sin, cos       spec_sincos<false> / <true>
 *   PT_SPEC_POW, PT_SPEC_POW_SK             2: x, y                          1: pow(x, y)      spec_pow<false> / <true>
 *   PT_SPEC_POW5                            1: x                             1: x^5            spec_pow5
 *   PT_SPEC_LCG                             1: seed (int32)                  2: new seed (int32), the float returned   lcg_rand
 *   PT_SPEC_DIFFUSE, PT_SPEC_DIFFUSE_SK     8: P.xyz, N.xyz, rnd1, rnd2      8: the new ray {P.xyz, 0, D.xyz, 0} as a diffuse hit builds it
 *                                                                               (prog.cl:205-218): D = normalize(diffuse_direction<false> /
 *                                                                               <true>(N, rnd1, rnd2)), P = madd(N, 0.001f, P)
 *   PT_SPEC_DIFFUSE_REC, PT_SPEC_DIFFUSE_REC_SK   as above                   as above, through diffuse_direction_rec<false> / <true> with the
 *                                                                               frame of N laid out as a shading record holds it
 *   PT_SPEC_FRESNEL                         9: F0.xyz, N.xyz, D.xyz          3: fresnel(F0, N, D) (prog.cl:219-222)
 * The _SK functions are the instances whose double constants are pinned to scalar registers (the kernels with 72-96 VGPRs run them),
 * the others leave the constants to the compiler (the 128-VGPR instance).
 * Item layout: one thread per item in blocks of 256 threads, no grid-stride loop: item i runs on lane i % 64 of wave i / 64 (four
 * waves per block), and a last wave that n does not fill runs with its remaining lanes off.  So the caller decides which inputs share
 * a wave -- the cosine-lobe functions pick their square-root cores with one branch per wave.
 * PT_EINVAL: unknown fn, n < 0, or a NULL array with n > 0 (checked before the context's device is, so a host-only context reports
 * them too); n = 0 does nothing and returns PT_OK; otherwise a host-only context gives PT_ENODEVICE. */
enum {
    PT_SPEC_SINCOS = 0, PT_SPEC_SINCOS_SK = 1, PT_SPEC_POW = 2, PT_SPEC_POW_SK = 3, PT_SPEC_POW5 = 4, PT_SPEC_LCG = 5,
    PT_SPEC_DIFFUSE = 6, PT_SPEC_DIFFUSE_SK = 7, PT_SPEC_DIFFUSE_REC = 8, PT_SPEC_DIFFUSE_REC_SK = 9, PT_SPEC_FRESNEL = 10
};
int pt_debug_spec(pt_context* ctx, int32_t fn, int64_t n, const uint32_t* in, uint32_t* out);
/* One iteration body of the path (prog.cl:317-366) on caller-supplied items: the device function the render kernels call at a hit
 * (shade_hit in pt_device.hpp, without a light hook), so that the vertex -- flip, preview colour, diffuse / mirror / glass / emitter
 * branch, factor weights, the shared normalise-and-step-off tail -- can be compared bit for bit with the CPU oracle without a render.
 * The scene is the context's own (uploaded triangles and materials); cam and iterations are what pt_render would be given (the vertex
 * reads cam->eye for the specular lobe and iterations == 1 for the preview colour).  instance picks the template instance:
 * PT_SHADE_SK set = double constants pinned to scalar registers, PT_SHADE_REC set = per-triangle shading records (kd, tangent frame and
 * the `plain` flag come from the record, as in the fused kernels with the tree in LDS).
 *   words in, PT_SHADE_WORDS_IN = 25 per item (floats as bit patterns):
 *     0-2 ray P.xyz   3-5 ray D.xyz   6 t of the hit   7 ti, index of the PACKED triangle hit (pt_debug_bvh_copy's order; int32)
 *     8 LCG state (int32)   9 inside-glass flag (0 / non-zero)   10-12 factor_L   13-15 factor_B   16-18 factor_S   19-21 factor_R
 *     22-24 colour
 *   words out, PT_SHADE_WORDS_OUT = 23 per item:
 *     0-2 new P.xyz   3-5 new D.xyz   6 LCG state   7 inside (0 / 1)   8-10 factor_L   11-13 factor_B   14-16 factor_S   17-19 factor_R
 *     20-22 colour
 * Item layout as for pt_debug_spec: one thread per item in blocks of 256 threads, no grid-stride loop: item i runs on lane i % 64 of
 * wave i / 64, and the lanes of a last wave past n leave before any wave-level vote -- the caller decides which hits share a wave
 * (the vertex runs one normalisation for a wave that holds several kinds of hit, and its divide / square-root cores are picked with
 * one branch per wave).
 * PT_EINVAL, all checked on the host before anything is launched and before the context's device is asked for: unknown instance bits,
 * n < 0, a NULL array with n > 0, a NULL camera or one whose XM / YM are not the context's frame, triangles or materials not uploaded,
 * a ti outside [0, packed triangles) -- never a device read.  n = 0 then returns PT_OK.  Otherwise a host-only context gives
 * PT_ENODEVICE, and PT_SHADE_REC on a context whose launches carry no shading records (tree not staged in LDS) PT_EINVAL. */
enum { PT_SHADE_SK = 1, PT_SHADE_REC = 2 };
#define PT_SHADE_WORDS_IN 25
#define PT_SHADE_WORDS_OUT 23
int pt_debug_shade(pt_context* ctx, const pt_camera* cam, int32_t iterations, int32_t instance, int64_t n, const uint32_t* in, uint32_t* out);
/* The authored scene (what the reference keeps in Scene::tris / Scene::mats, main.cpp:366-371):
 * triangles in add order, materials, and the first triangle of every object. */
int pt_debug_scene_sizes(const pt_context* ctx, int64_t* ntris, int64_t* nmats, int64_t* nobjs);
int pt_debug_scene_copy(const pt_context* ctx, pt_triangle* tris, pt_material* mats, int32_t* obj_begin);
/* the reference's traversal encounter rank of each triangle, in add order */
int pt_debug_encounter_rank(const pt_context* ctx, int32_t* out, int64_t n);
/* the list of active tiles the last decision of the held adaptive frame left (ascending local-frame tile indices): *n = its length
 * (0 without an adaptive frame, or before its first decision), the first min(cap, *n) entries go to out */
int pt_debug_adaptive_list(pt_context* ctx, int32_t* out, int64_t cap, int64_t* n);
/* after a counting launch (option count_work = 1, pt_render; schedules 0 and 1 -- under schedule 2 a wave works on two tiles at
 * once and leaves this zero): per 8x8 tile of the local frame, shader-clock cycles / 64 spent on it */
int pt_debug_tile_cost(pt_context* ctx, uint32_t* out, int64_t n_tiles);
/* What pt_render(nsamples) would launch on a device of cu_count compute units (0: the context's own; works on a host-only
 * context): out[8] = { threads per workgroup, waves per SIMD, schedule (0 lockstep, 1 suspend, 2 migrate), samples per (pass, tile)
 * work item (0: whole tiles), resident waves, tiles, node mode, dynamic LDS bytes }.  Lets CPU tests pin the launch policy
 * of a rank of an N-GPU job. */
int pt_debug_launch_plan(pt_context* ctx, int32_t nsamples, int32_t cu_count, int64_t out[8]);
/* frame assembly: out[gid] = index into the rank-major all-gather buffer (slab_stride pixels per rank) that
 * global pixel gid is read from -- the host statement of the de-interleave kernel's map (no device work) */
int pt_debug_gather_index(int32_t width, int32_t height, int32_t world, int32_t rows_per_block, int64_t slab_stride, int64_t* out);
/* runs ONLY the de-interleave kernel of pt_gather_frame on a caller-supplied all-gather buffer
 * (world x slab pixels, float4 each) with the context's frame size and tiling */
int pt_debug_deinterleave(pt_context* ctx, const float* gathered_rgba, int64_t n_pixels, float* out_frame_rgba);

#ifdef __cplusplus
}
#endif
#endif
