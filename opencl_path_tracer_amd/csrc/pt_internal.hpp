// pt_internal.hpp -- shared between the host side (pt_host.cpp, pt_builder.cpp, pt_launch.cpp: see pt_context.hpp) and the device side
// (pt_kernels.hip) of libptamd.so.  Not part of the public ABI (that is include/pt_api.h).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pt_api.h"

namespace ptamd {

// ---- packed scene layout in HBM ----------------------------------
// BVH2 node, 64 B = 4 x float4.  A node stores the boxes of BOTH children so one fetch
// decides both descents:
//   q[a] (a = 0,1,2 = x,y,z) = { Lmin[a], Lmax[a], Rmin[a], Rmax[a] }
//   q[3] = { bits(left), bits(right), 0, 0 }
// child reference >= 0: interior node index; < 0: leaf, ~ref = (first << 3) | (count - 1).
struct Node64 {
    float q[3][4];
    int32_t left, right;
    int32_t pad[2];
};
static_assert(sizeof(Node64) == 64, "Node64 must be 64 B");

// Triangle packet, 48 B = 3 x float4: { r1.xyz r2.x | r2.yz r3.xy | r3.z N.xyz } -- exactly the
// twelve floats prog.cl:94-112 reads, nothing derived (the hit test is bit-defined by them).
struct TriPacket {
    float v[12];
};
static_assert(sizeof(TriPacket) == 48, "TriPacket must be 48 B");

// per packed triangle: encounter rank in the reference's traversal (tie-break), material index
struct TriMeta {
    int32_t rank;
    int32_t mati;
};

// per packed triangle: what shade_hit needs of the triangle and of its material, 96 B = 6 x float4 (pt_shaderec.hip builds it on the
// device after every upload of triangles or materials; shade_hit<SK, REC = true> reads it).  All of it is constant between uploads:
//   { N.xyz, bits(type) }          the geometric normal as packed (packet floats 9..11), the material's type
//   { kd.xyz, bits(mati | plain) } the material's kd; its index, with kShadeRecPlain set when a diffuse hit needs nothing else of
//                                  the material: _pad is set (pt_upload_materials) and ks is +0 in all three components
//   frame[o] = { Z.xyz, X.x | X.yz, 0, 0 }    tangent_frame() of N (o = 0) and of -N (o = 1): both are computed, never one derived
//                                  from the other -- Z has a literal +0 component, so the signs of zeros in X do not simply flip
struct ShadeRec {
    float N[3];
    int32_t type;
    float kd[3];
    uint32_t mati;
    float frame[2][8];
};
static_assert(sizeof(ShadeRec) == 96, "ShadeRec must be 96 B");
constexpr uint32_t kShadeRecPlain = 0x80000000u;
constexpr int32_t kShadeRecNoMaterial = 0x7fffffff;   // type of a record whose mati is outside the uploaded materials (never a lobe or a specular type)
// Which k_render instances read the record: the fused ones (SPLIT = false) with the tree in LDS, the VALU-bound launches.  The
// launches that read nodes from global memory wait for memory, not for the VALU, and a mesh's records would be 96 B per triangle
// next to packets that already miss L2: no record is built for them.
constexpr bool shade_records_for(int node_mode) { return node_mode == 0 /* kNodesLds */; }

// 4-wide node, 64 B = 4 x float4 (pt_wide.cpp builds it from the BVH2; Trav<kNodesWide>::wide_step reads it):
//   { origin.xyz, exp_x | exp_y << 8 | exp_z << 16 | nchild << 24 }      grid of the node: plane = origin + q * 2^(exp - 127)
//   { qlo_x, qhi_x, qlo_y, qhi_y }   { qlo_z, qhi_z, -, - }              byte k of each word = child k's plane on that grid
//   { ref[0..3] }                    child references as in Node64; kWideNoChild (and an inverted box) where there is no child
struct Node4q {
    float origin[3];
    uint8_t exp[3];
    uint8_t nchild;
    uint32_t qlo_x, qhi_x, qlo_y, qhi_y;
    uint32_t qlo_z, qhi_z;
    uint32_t spare[2];
    int32_t ref[4];
};
static_assert(sizeof(Node4q) == 64, "Node4q must be 64 B");
constexpr int32_t kWideNoChild = ~0;      // the leaf {packet 0, 1 triangle}: always present (an empty scene holds one all-zero packet)
constexpr int kWideLdsEntries = 20;   // 20 x 4 B x 256 lanes = 20 KB per workgroup: seven workgroups per CU next to the big-triangle list
bool build_wide_nodes(const std::vector<Node64>& bvh2, std::vector<Node4q>* out, int* max_pending, int threads);   // pt_wide.cpp

// Where the traversal reads BVH nodes from (Trav<MODE> in pt_device.hpp)
enum : int { kNodesLds = 0, kNodesGlobal = 1, kNodesTreelet = 2, kNodesWide = 3 };

// Packets and nodes are addressed with 32-bit byte offsets on the device (index * 48, index << 6) and a
// leaf reference holds first << 3 in 31 bits: 2^26 triangles (hence < 2^26 nodes) keep all three in range.
constexpr int64_t kMaxTriangles = (int64_t)1 << 26;

constexpr int64_t kDeviceBuildFrom = 16384;   // SAH trees of scenes this big are built on the device by default (same tree; mesh6k: 2.4 vs 2.8 ms, 1M: 15 vs 99)
constexpr int kMaxLeaf = 4;        // triangles per leaf (<= 8 by the reference encoding)
constexpr int kMaxDepth = 30;      // builder guarantees depth <= kMaxDepth
constexpr int kTileCounterError = 16;  // word of RenderParams::tile_counter that holds 1 + tile of a lost hand-over (word 17: the pass) -- on a cache
                                       // line of its own: the waves that poll for a hand-over look at it now and then, and the line of words 0 / 1
                                       // takes every work-item fetch of the launch
constexpr int kMaxTaperPasses = 30;   // passes of a launch whose lengths are tabled (RenderParams::taper_end)
constexpr int kTileCounterWords = 32;  // words of the work counter (two 64-byte lines)
constexpr int kStatRows = 256;     // statistics counters are spread over this many rows of kStatCols
constexpr int kStatCols = 16;
// k_render instances whose register budget is set for this many waves per SIMD or more carry nothing across a traversal
// that can be recomputed or fetched (LEAN, pt_kernels.hip) -- A/B switch: 8 = never.  7: at 80 VGPRs (six waves) the two
// forms measure the same (2,347 / 2,354 on the Cornell box, 787 / 794 on MESH-100k, profiles/r03/r_*), and the plain one
// leaves the frame buffer alone until the end of a pass.
// Round 4: 6.  Under schedule 2 the plain 80-VGPR instance spills four registers of path state around every traversal -- stores in
// the hot loop, whose dirty lines every agent-scope release of a chained pass writes back: 17.3 GB of WRITE_SIZE per 64-spp launch
// of the Cornell box, against 4.0 GB for the lean form (whose frame-buffer lines are what is flushed), at +1 % (profiles/r04/u_*).
#ifndef PT_LEAN_FROM_WPS
#define PT_LEAN_FROM_WPS 6
#endif
constexpr int kLeanFromWps = PT_LEAN_FROM_WPS;
// The k_render instances for a tree staged whole in LDS (two workgroups per CU either way): 2 x 768 threads at an 80-VGPR
// budget = six waves per SIMD when the LDS has room for it (12 waves per workgroup = 3 per SIMD: any placement of the two
// workgroups fits; 2 x 640 at 96 VGPRs does not -- 10 waves land 3+3+2+2 and the second workgroup finds two SIMDs full,
// which is what made "five waves" lose 30 % in round 2), otherwise 2 x 512 at 128 VGPRs.  Cornell box: 2,050 -> 2,349
// Msamples/s (profiles/r03/f_*).
constexpr int kLdsBlockWide = 768, kLdsWpsWide = 6;
constexpr int kLdsBlockBase = 512, kLdsWpsBase = 4;
// a node of a tree staged whole in LDS (kNodesLds): three swizzled box quads + both 16-bit child references in one word,
// 52 B padded to 56.  Not 64: a 14-dword stride puts the same field of 32 different nodes on 32 different bank pairs
// (a 16-dword stride on 4), and 7.5 KB less per workgroup is what lets two 768-thread workgroups share a CU
#ifndef PT_LDS_NODE_BYTES
#define PT_LDS_NODE_BYTES 56
#endif
constexpr int kLdsNodeBytes = PT_LDS_NODE_BYTES;
constexpr int kStackEntries = 36;  // upper bound of the per-lane traversal stack: sentinel + far children + one slot above the top

// ---- kernel parameter block (passed by value, like `Camera` in prog.cl:292-304) ----------
struct RenderParams {
    const float4* nodes;
    const float4* tris;
    const TriMeta* meta;
    const pt_material* mats;
    int32_t* rnds;          // local pixels
    float4* colors;         // local pixels, float3 @ 16 B
    pt_ray* rays;           // local pixels
    unsigned long long* stats;   // [kStatRows][kStatCols]: 0 segments, 1 samples, 2 node visits, 3 tri tests, 4/5 wave-level body runs,
                                 // 6 tile lane steps, 7 wave-level shade runs, 8 wave-level trips of the segment loop, 9 wave-level rounds
    pt_camera cam;
    int32_t width, height;       // GLOBAL frame
    int32_t local_rows;          // rows owned by this context
    int32_t rank, world, rows_per_block;
    int32_t iterations, first_sample, nsamples;
    int32_t n_nodes, n_tris;
    int32_t n_flat;              // packets [0, n_flat) are the big-triangle list: tested by every ray before the tree
    int32_t n_fbox;              // their distinct boxes (the two triangles of a wall share one): box b is that of packet fbox_rep[b]
    uint8_t fbox_rep[32];        // and covers the listed triangles in fbox_mask[b]
    uint32_t fbox_mask[32];
    uint32_t fpair_mask;         // bit i: listed triangles i and i + 1 share plane words and r1 words in the staged copy: one test (Trav::flat_pass)
    uint32_t fpair_canon;        // bit i: the staged copy of listed triangle i has +0 where the packet's N has -0
    uint64_t fpair_rot;          // two bits per listed triangle: the staged copy's corners are the packet's, rotated by that many (setup_traversal)
    int32_t node_mode;           // kNodesLds / kNodesGlobal / kNodesTreelet / kNodesWide: where the traversal reads BVH nodes from (and which)
    int32_t treelet_nodes;       // kNodesTreelet: nodes [0, treelet_nodes) are staged in LDS
    int32_t stack_entries;       // per-lane stack entries in LDS: all a BVH2 traversal can need (sentinel + deepest interior node + the slot
                                 // above the top); kNodesWide: at most kWideLdsEntries, the rest of the worst case in stack_ovf
    uint32_t* stack_ovf;         // kNodesWide: [entries past the LDS part][lane of the grid], or null when LDS holds the worst case
    int32_t stack_ovf_lanes;     // lanes stack_ovf has room for (every launch's grid must fit)
    uint32_t* tile_counter;      // != 0: persistent launch, waves pull tile indices from word 0; word 1 counts the waves that left (the last resets
                                 // both); words 16 / 17: 1 + tile and pass of a hand-over that never came (kTileCounterError), left for the host
    uint32_t poll_ticks;         // chained passes: how long a wave waits for a tile's previous pass, in 10-ns ticks of s_memrealtime, before it
                                 // reports the tile in word 4 and the launch winds down (pt_sync then returns PT_EHIP)
    int32_t debug_stall_tile;    // tests: pass 0 of this tile is rendered but never published (-1: none)
    int32_t n_tiles;             // tiles of the launch: those of the local frame, or the n_tiles entries of tile_list
    // passes of DIFFERENT lengths (option chunk_taper): n_taper > 0 -> pass k of a tile is samples [taper_end[k-1], taper_end[k]) of the
    // launch (taper_end[-1] = 0), n_taper passes in all; the last passes are short, so that the launch does not end on whole long items
    int32_t n_taper;
    uint16_t taper_end[kMaxTaperPasses];
    int32_t chunk_spp;           // > 0: a work item is (pass, tile) = chunk_spp samples of a tile; passes of one
                                 // tile are chained through tile_done[] (agent-scope release / acquire)
    uint32_t* tile_done;         // [n_tiles] number of passes completed, zeroed before the launch
    int32_t suspend_lanes;       // megakernel: leave the traversal when at most this many lanes are unfinished (0: never)
    int32_t node_min_lanes;      // Trav::round: the node phase ends early when at most this many lanes still descend and another holds a leaf (0: never)
    int32_t leaf_min_lanes;      // ... and the leaf phase when at most this many lanes still hold leaves and another has a node (0: never)
    int32_t migrate_lanes;       // kSchedMigrate: lanes that are done with the wave's current work item move to the next one when this many have gathered
    uint32_t* tile_cost;         // counting instances only, or null: [n_tiles] += shader-clock cycles / 64 the wave spent on each work item of the tile (pt_debug_tile_cost)
    const int32_t* tile_list;    // != 0 (adaptive frames, pt_render_adaptive): tile t of the launch is frame tile tile_list[t]; work items,
                                 // tile_done[] and debug_stall_tile count list positions, tile_cost frame tiles
    const float4* shaderec;      // [n_tris] ShadeRec, or null where the launch's instance does not read it (shade_records_for)
    int32_t moments;             // option "moments": 1 folds every sample's squared luminance into colors[].w (running_moment), 0 writes .w = 0
};

// local row -> row of the frame: the frame's rows are dealt out to the `world` ranks in blocks of rows_per_block
// (P: RenderParams on the device, pt_context on the host)
template <class P>
__host__ __device__ __forceinline__ int global_row(const P& p, int lrow) {
    return ((lrow / p.rows_per_block) * p.world + p.rank) * p.rows_per_block + lrow % p.rows_per_block;
}

// ---- wavefront (stream-compacted) formulation
// Ray streams, one per (bounce parity, cost class), addressed by POSITION (compact, written and read coalesced), 48 B per
// ray:   rsA = {P.xyz, D.x}   rsB = {D.y, D.z, bits(li), bits(flags)}   rsC = {factor_L.xyz, bits(LCG state)}
// What changes at (almost) every segment rides the stream: the ray, factor_L (every diffuse hit multiplies it) and the LCG
// state (every diffuse / emitter / glass hit draws) -- round 3 kept the last two in per-PIXEL arrays, 12-B and 4-B accesses
// scattered by the compaction order, which cost a 64-byte sector each way each.  wf_intersect reads rsA and half of rsB only.
// Per local pixel (index li): the other three factors and the colour, arrays of 12-B records sP[field][li] (kWfB .. kWfC; the
// kWfL slot is unused).  A field is read only if it was written in this sample and written only by the material that changes it
// (PathInHbm, pt_wavefront.hip): mirrors factor_S, glass factor_R, emitters the colour; factor_B only where a material has a
// specular lobe -- with ks = 0 it becomes +0 at the first diffuse hit and stays there, which is one flag bit, not 12 bytes.
// rnds[li] is read by wf_generate and written when the path ends.
//                                    flags: bit f (f < 5) = field f of sP is valid; bit 5 = the path is inside glass;
//                                    bit 6 = factor_B is +0 in all three components (nothing stored)
// Hit stream, parallel to the ray stream of the current bounce, 8 B:  hit = {t, bits(tri)}
// Class queues (shade input): entries (cost << 31) | position.
// Counter rows (kWfCounterStride words each), see wf_row(): 0 n_ray cheap, 1 n_ray expensive,
// 2..4 n_class A/B/C, 5 / 6 next unassigned ray of the cheap / expensive stream (wf_intersect's work fetch).
// Row 0 belongs to bounce 0 (filled by wf_generate, cleared by a memset in
// front of it); bounce b >= 1 uses row b + 1 (cleared by wf_generate).
constexpr int kWfCounterStride = 8;
constexpr int kWfMaxBounces = 1023;
constexpr int kWfGenRow = 0;
__host__ __device__ inline int wf_row(int bounce) { return bounce == 0 ? kWfGenRow : bounce + 1; }
constexpr int kWfMaxCostBoxes = 8;
constexpr int kWfMaxChains = 8;
constexpr int kWfDefaultChains = 4;
enum : int { kWfL = 0, kWfB = 1, kWfS = 2, kWfR = 3, kWfC = 4, kWfFields = 5, kWfInsideBit = 1 << 5, kWfBZeroBit = 1 << 6 };
struct WfParams {
    RenderParams rp;
    float* sP;             // [kWfFields][npix] x 3 floats
    float4* rsA[2][2];     // [bounce parity][cost class]
    float4* rsB[2][2];
    float4* rsC[2][2];
    float2* hit[2];        // [cost class]
    int32_t* q_cls[3];     // shade input queues: 0 diffuse/emitter, 1 mirror/dielectric/other, 2 miss
    uint32_t* counters;    // [(iterations + 3) * kWfCounterStride]
    float cbox[kWfMaxCostBoxes][6];   // bounding boxes of the complex objects (min xyz, max xyz)
    int32_t n_cbox;
    int32_t npix;          // pixels of this CHAIN (the local pixels are cut into wf_streams contiguous chains, each with its own
                           // streams, queues and counters, run on its own HIP stream: one chain's launch tails under another's work)
    int32_t pix0;          // first local pixel of the chain
    int32_t npix_all;      // local pixels of the context (stride of sP's fields)
    int32_t sample;        // current_sample of this pass
};

// device-side BVH construction (pt_lbvh.hip); all pointers are device memory owned by the caller
struct LbvhResult {
    float4* d_nodes = nullptr;
    int n_nodes = 0;
    float4* d_tris = nullptr;
    TriMeta* d_meta = nullptr;
    int32_t* d_orig = nullptr;
    int depth = 0;
};
// all triangles of a scene in device memory, for the device builders (pt_sahdev.hip: stage_*)
struct DeviceStage {
    char* base = nullptr;            // the one allocation behind the pointers below
    pt_triangle* d_tris = nullptr;   // add order
    int32_t* d_rank = nullptr;       // encounter ranks, add order
    int32_t* d_sel = nullptr;        // add-order indices of the triangles that go into the tree (stage_select)
    float* d_area = nullptr;         // half area of every triangle's padded bounds
    int* d_misc = nullptr;
    int n = 0;
};
hipError_t stage_upload(const pt_triangle* h_tris, const int32_t* h_rank, int n, hipStream_t stream, DeviceStage* st, float* h_area, int* nonfinite);
hipError_t stage_rest_box(const DeviceStage& st, const int32_t* h_top, int cand, hipStream_t stream, float box[6]);
hipError_t stage_select(const DeviceStage& st, const int32_t* h_flat, int nf, hipStream_t stream);
void stage_free(DeviceStage* st);
hipError_t lbvh_build(const pt_triangle* d_tris, const int32_t* d_rank, int n_all, const int32_t* d_sel, int n, int ploc_radius, hipStream_t stream, LbvhResult* out);
// the host builder's binned-SAH tree, built on the device (pt_sahdev.hip); *unsupported: a range needs the host's median split
hipError_t sah_device_build(const pt_triangle* d_tris, const int32_t* d_rank, int n_all, const int32_t* d_sel, int n, int max_leaf, bool force_leaf, float visit_cost, int grain,
                            hipStream_t stream, LbvhResult* out, bool* unsupported);

// build_wide_nodes() on the device (pt_widedev.hip): the same 4-wide nodes for a BVH2 that is in device memory
hipError_t wide_device_build(const float4* d_bvh2, int n_nodes, hipStream_t stream, float4** d_out, int* n_out, int* max_pending, bool* failed);

struct LaunchConfig {
    int block = 256;                   // traversal_block(node_mode)
    size_t lds_bytes = 0;              // traversal_lds_bytes()
    int persistent_blocks = 1 << 30;   // grid size of a persistent launch (workgroups that fit the chip): what launch_cfg expects to be resident
    int cu_count = 0;                  // compute units of the device (> 0: the grid is also capped by what the runtime says can co-reside)
    bool count_work = false;           // also count node visits / triangle tests into stats[2..9]
    int schedule = 0;                  // megakernel: 0 lockstep per sample, 1 restart + tail suspension (pt_kernels.hip)
    int waves_per_simd = 4;            // register budget of the k_render instance: 4, or 5 / 6 / 7 for nodes from global memory
};

// Dynamic LDS above 64 KB needs hipFuncAttributeMaxDynamicSharedMemorySize on the kernel.  Set ONCE per kernel instance
// and device (a high-water mark), not per launch: the reference's own loop shape launches a kernel per sample
// (main.cpp:683-687) and a per-launch runtime call shows there.  `mark` = one static array per template instantiation.
constexpr int kMaxDevicesPerProcess = 16;
struct LdsMark {
    std::atomic<size_t> bytes[kMaxDevicesPerProcess];
};
inline hipError_t ensure_dynamic_lds(const void* kern, LdsMark& mark, size_t lds_bytes) {
    if (lds_bytes <= 64 * 1024) return hipSuccess;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= kMaxDevicesPerProcess) return hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (mark.bytes[dev].load(std::memory_order_acquire) >= lds_bytes) return hipSuccess;
    e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) return e;
    size_t seen = mark.bytes[dev].load(std::memory_order_relaxed);
    while (seen < lds_bytes && !mark.bytes[dev].compare_exchange_weak(seen, lds_bytes, std::memory_order_release)) {}
    return hipSuccess;
}

// Workgroups of `kern` (BLOCK threads, lds_bytes of dynamic LDS) that can be resident on one CU according to the runtime, asked
// once per kernel instance, device and LDS size.  A persistent grid is capped by it: launch_cfg's own figure is derived from the
// register budget the instance was compiled for, and a grid LARGER than what is co-resident would leave workgroups queued behind
// waves that poll for a hand-over (harmless for correctness -- a producer is always dequeued before its consumer -- but it is not
// the launch shape the schedules were tuned for).  0: the runtime gave no answer.
struct OccMark {
    std::atomic<long long> key[kMaxDevicesPerProcess];      // (lds_bytes << 8) | blocks per CU
};
inline int resident_blocks_per_cu(const void* kern, OccMark& mark, int block, size_t lds_bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevicesPerProcess) return 0;
    const long long seen = mark.key[dev].load(std::memory_order_acquire);
    if (seen != 0 && (size_t)(seen >> 8) == lds_bytes) return (int)(seen & 0xff);
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, block, lds_bytes) != hipSuccess || n <= 0) return 0;
    mark.key[dev].store(((long long)lds_bytes << 8) | (long long)std::min(n, 255), std::memory_order_release);
    return n;
}

// PTAMD_TRACE=1: phase times of the host-side scene path on stderr (pt_add_obj, pt_upload_triangles; tools/obj_load_time.py)
struct PhaseClock {
    const char* who;
    const bool on = std::getenv("PTAMD_TRACE") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit PhaseClock(const char* w) : who(w) {}
    void lap(const char* what) {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[%s] %-32s %8.1f ms\n", who, what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

// launchers (pt_kernels.hip, pt_wavefront.hip, pt_debug.hip); all asynchronous on `stream`
int traversal_block(int node_mode, bool wide_lds_block);       // threads per workgroup of k_render
size_t traversal_lds_bytes(const RenderParams& p, int block);  // stacks + staged nodes
hipError_t launch_gen_ray(const RenderParams& p, hipStream_t stream);
hipError_t launch_trace_ray(const RenderParams& p, const LaunchConfig& lc, hipStream_t stream);
hipError_t launch_render_mega(const RenderParams& p, const LaunchConfig& lc, hipStream_t stream);
hipError_t launch_resolve_reinhard(const float4* colors, float4* out, int64_t n, hipStream_t stream);
hipError_t launch_filt_im(const float4* colors, float4* out, int32_t width, int32_t height, hipStream_t stream);
// the per-triangle shading records of n packed triangles (pt_shaderec.hip)
hipError_t launch_shade_records(const float4* tris, const TriMeta* meta, const pt_material* mats, int32_t n_mats, int32_t n, ShadeRec* out, hipStream_t stream);
hipError_t launch_wf_generate(const WfParams& p, hipStream_t stream);
hipError_t launch_wf_intersect(const WfParams& p, int bounce, int cu_count, hipStream_t stream);
hipError_t launch_wf_shade(const WfParams& p, int bounce, hipStream_t stream);
// adaptive frames (pt_adaptive.hip): per tile of `list` (null: every tile of the frame, n_list of them) -- mode 0 tile_spp = spp; 1 also
// snap = colors; 2 also the noise estimate against snap -> tile_err, active (0: retired), and snap = colors where the tile stays active
hipError_t launch_adaptive_tiles(const float4* colors, float4* snap, const int32_t* list, int32_t n_list, int32_t width, int32_t rows, int mode,
                                 float threshold, int32_t spp, float* tile_err, int32_t* tile_spp, uint8_t* active, hipStream_t stream);
// metric PT_ADAPT_VARIANCE (pinned in include/pt_api.h): per tile of `list` the root mean square of the pixels' variance of the mean
// luminance at spp samples (colors[].w: option "moments") -> tile_err, active (0: retired), tile_spp = spp; reads and writes no snapshot
hipError_t launch_adaptive_variance(const float4* colors, const int32_t* list, int32_t n_list, int32_t width, int32_t rows, float threshold,
                                    int tonemapped, int32_t spp, float* tile_err, int32_t* tile_spp, uint8_t* active, hipStream_t stream);
// the frame tiles whose flag is set, ascending, into list[0, *count) (one workgroup)
hipError_t launch_compact_tiles(const uint8_t* active, int32_t n, int32_t* list, int32_t* count, hipStream_t stream);
hipError_t launch_debug_closest_hit(const RenderParams& p, const pt_ray* rays, int64_t n, float* out_t, int32_t* out_tri, int cu_count, hipStream_t stream);
hipError_t launch_debug_math(int fn, unsigned long long first, unsigned long long n, unsigned long long* out, uint32_t* bad, long long bad_cap, int cu_count,
                             hipStream_t stream);
// pt_debug_spec (pt_debug.hip): 32-bit words per item of function fn (PT_SPEC_* in pt_api.h), 0 for an unknown fn
constexpr int spec_words_in(int fn) {
    return fn == PT_SPEC_SINCOS || fn == PT_SPEC_SINCOS_SK || fn == PT_SPEC_POW5 || fn == PT_SPEC_LCG ? 1
         : fn == PT_SPEC_POW || fn == PT_SPEC_POW_SK ? 2
         : fn >= PT_SPEC_DIFFUSE && fn <= PT_SPEC_DIFFUSE_REC_SK ? 8
         : fn == PT_SPEC_FRESNEL ? 9 : 0;
}
constexpr int spec_words_out(int fn) {
    return fn == PT_SPEC_SINCOS || fn == PT_SPEC_SINCOS_SK || fn == PT_SPEC_LCG ? 2
         : fn == PT_SPEC_POW || fn == PT_SPEC_POW_SK || fn == PT_SPEC_POW5 ? 1
         : fn >= PT_SPEC_DIFFUSE && fn <= PT_SPEC_DIFFUSE_REC_SK ? 8
         : fn == PT_SPEC_FRESNEL ? 3 : 0;
}
hipError_t launch_debug_spec(int fn, const uint32_t* in, int64_t n, uint32_t* out, hipStream_t stream);
// pt_debug_shade (pt_debug.hip): 32-bit words per item in and out (layout in pt_api.h); instance = PT_SHADE_SK | PT_SHADE_REC bits
constexpr int kShadeWordsIn = PT_SHADE_WORDS_IN, kShadeWordsOut = PT_SHADE_WORDS_OUT;
hipError_t launch_debug_shade(const RenderParams& p, int instance, const uint32_t* in, int64_t n, uint32_t* out, hipStream_t stream);
// guide buffers and the a-trous filter (pt_denoise.hip; the filter is pinned in include/pt_api.h next to pt_denoise).  lights: the area set
// of the lit guides (option aov_lights), or nullptr for the unlit instances
struct AreaLightsView;
hipError_t launch_aovs(const RenderParams& p, int32_t subpixels, int32_t specular_depth, int64_t npix, float4* albedo_rgbm, float4* normal_depth,
                       const AreaLightsView* lights, int cu_count, hipStream_t stream);
struct AtrousStep {
    int32_t step;            // 2^i
    int32_t demodulate;
    int32_t color_on, normal_on, depth_on;   // 0: that weight is 1 (sigma +inf; sigma_normal 0)
    float color_scale;       // 4^i
    float sigma_color2, sigma_normal, sigma_depth;
};
// one iteration: first reads colors (demodulated when s.demodulate), last remodulates; out must not alias in
hipError_t launch_atrous(const float4* in, float4* out, const float4* albedo, const float4* nd, int32_t W, int32_t H, const AtrousStep& s,
                         bool first, bool last, hipStream_t stream);
// one iteration of the variance-guided filter (pt_denoise_variance): {x, v} float4 in / out; FIRST reads colors + the variance read-out
// (demodulated when s.demodulate), LAST remodulates both; out must not alias in
struct AtrousVarStep {
    int32_t step;            // 2^i
    int32_t demodulate;
    int32_t lum_on, normal_on, depth_on;   // 0: that weight is 1 (sigma +inf; sigma_normal 0)
    float sigma_luminance, sigma_normal, sigma_depth;
};
hipError_t launch_atrous_var(const float4* in, const float* var, float4* out, const float4* albedo, const float4* nd, int32_t W, int32_t H,
                             const AtrousVarStep& s, bool first, bool last, hipStream_t stream);
// per local pixel, the variance of its mean luminance from colors[].xyz / .w (option "moments"); n from tile_spp (adaptive frames, per 8x8
// tile of the local frame) or n_all (tile_spp null): pt_read_variance, pinned in include/pt_api.h
hipError_t launch_variance(const float4* colors, const int32_t* tile_spp, int32_t n_all, int32_t W, int64_t npix, float* out, hipStream_t stream);
// next-event estimation (pt_nee.hip; the estimator is pinned in include/pt_api.h next to pt_render_nee)
struct NeeTable {
    const int32_t* tri;          // [n] packed triangle of each light
    const float* cdf;            // [n]
    const float* pdf_area;       // [packed triangles] P_sel / area, 0 for non-lights
    int32_t n;                   // 0: no lights (every strategy is PT_NEE_BSDF)
    int32_t strategy;
};
// the environment of pt_render_nee (pt_set_environment; pinned in include/pt_api.h)
struct EnvView {
    const float4* texels;        // [h][w] {r, g, b, p_env = P(texel) / Omega(row)}
    const float* row_cdf;        // [h]
    const float* col_cdf;        // [h][w]
    int32_t w, h;
    float scale, yaw;            // yaw in radians
    float p_env;                 // the effective P_env (a multiple of 2^-24)
};
// albedo textures of pt_render_nee (option textures; pinned in include/pt_api.h)
struct TexDesc {
    uint32_t first;              // the texture's first texel in the shared buffer
    int32_t w, h, filter;        // filter 0 nearest, 1 bilinear
};
struct TexView {
    const float4* uv;            // [packed triangles][2] {u1, v1, u2, v2}, {u3, v3, flag, 0} (k_pack_vertex_uvs, pt_texture.hip)
    const uint2* texels;         // 8 B each: halves r | g << 16, b
    const TexDesc* desc;         // [textures]
    const int32_t* mat_tex;      // [materials on the device] texture of a type-0 material, else -1
};
// the thin lens of pt_render_nee (pt_set_lens; pinned in include/pt_api.h): the parameters and the launch's constants f, Rh, Uh
struct LensView {
    float aperture, focus;
    float f[3], Rh[3], Uh[3];
};
// the analytic lights of pt_render_nee (pt_set_lights; pinned in include/pt_api.h).  A record is four float4s:
//   { position.xyz, bits(type) }  { axis.xyz, cos_inner }  { intensity.rgb, cos_outer }  { P_light, 0, 0, 0 }
// axis: unit, the way the light points (POINT with a cone) or travels (DIRECTIONAL); zero for a point light without a cone
struct LightsView {
    const float4* rec;           // [n][4]
    const float* cdf;            // [n], proportional to the selection weights; the last entry is 1
    int32_t n;
    float p_ana;                 // the effective P_ana of the launch (a multiple of 2^-24)
};
// the homogeneous medium of pt_render_nee (pt_set_medium; pinned in include/pt_api.h): pt_medium's fields as the kernel reads them, all
// wave-uniform (a kernel argument by value, so they stay in scalar registers)
struct MediumView {
    float sigma_t;               // > 0 in every launch of the medium instances
    float albedo[3];
    float g;
    float lo[3], hi[3];          // -inf / +inf: unbounded on that side
};
// the density grid of the medium (pt_set_medium_density; pinned in include/pt_api.h): nx x ny x nz equal cells of the medium's box, which is
// finite in every launch that reads one.  A kernel argument by value: the pointer, the dimensions and the cell sizes stay in scalar registers
struct GridView {
    const float* rho;            // density[(k * ny + j) * nx + i], each finite and >= 0
    int32_t n[3];                // nx, ny, nz, each in [1, PT_GRID_MAX_DIM]
    float cell[3];               // (hi - lo) / n per axis, float32
    float inv_cell[3];           // n / (hi - lo) per axis, float32
};
// the interiors bound to materials (pt_set_material_interior; pinned in include/pt_api.h): per material on the device two float4,
// {sigma_a.rgb, sigma_s} and {g, bound (1 or 0), 0, 0}; bound is 0 wherever the material is not of type 2 or 6 or holds no binding
struct InteriorView {
    const float4* rec;
};
// the light hierarchy over the light table (option light_tree; pinned in include/pt_api.h; built by pt_lighttree.cpp).
// A node is two float4, {c.xyz, r} and {phi, bits(first), bits(count), bits(right)}: the sphere around the box of its lights' vertices, the sum
// of their weights, its range [first, first + count) of tree-order light indices and its right child (the left one is node + 1; count 1: a leaf)
struct LightTreeView {
    const float4* nodes;         // [2 * n_nodes]
    const int32_t* tri;          // [n_lights] packed triangle of each light, in tree order
    const float* inv_area;       // [n_lights] (float)(1 / area), in tree order
    const int32_t* slot;         // [packed triangles] tree-order light index, -1 for non-lights
    int32_t n_nodes, n_lights;   // 0, 0: no lights
};
// the area lights of pt_render_nee (pt_set_area_lights; pinned in include/pt_api.h; built by pt_arealights.cpp): spheres
// first, then suns.  A record is three float4s:
//   sphere  { centre.xyz, R }                          { radiance.rgb, P_light }  { 0, 0, 0, 0 }
//   sun     { axis.xyz (unit, towards the sun), cos a } { radiance.rgb, P_light }  { q = 2 sin^2(a / 2), 0, 0, 0 }
// A kernel argument by value: the pointers and the counts stay in scalar registers, and a loop over the records has wave-uniform addresses
struct AreaLightsView {
    const float4* rec;           // [n][3]
    const float* cdf;            // [n], proportional to the selection weights; 1 from the last pickable light on
    int32_t n_sphere, n;         // the spheres are records [0, n_sphere), the suns [n_sphere, n)
    float p_area;                // the effective P_area of the launch (a multiple of 2^-24)
};
constexpr unsigned kAreaKey = 0x9e3779b9u;     // u_area's key is S ^ kAreaKey (PT_AREA_KEY, include/pt_api.h)
constexpr int kLightTreeMaxDepth = 64;     // the loop bound of both walks; the builder keeps every leaf at or above it
__host__ __device__ __forceinline__ int lt_bits(float f) { return __builtin_bit_cast(int, f); }
// the importance of the child {q0 = (c, r), phi} from the origin o with the cull normal G (0: nothing is culled): 0 if its sphere lies
// entirely below the horizon, else phi / max(|c - o|^2, r^2); dot3's fma placement
__host__ __device__ __forceinline__ float lt_importance(const float4 q0, float phi, float ox, float oy, float oz, float gx, float gy, float gz) {
    const float dx = q0.x - ox, dy = q0.y - oy, dz = q0.z - oz;
    if (__builtin_fmaf(gz, dz, __builtin_fmaf(gy, dy, gx * dx)) < -q0.w) return 0.0f;
    const float d2 = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)), r2 = q0.w * q0.w;
    return phi / (d2 > r2 ? d2 : r2);
}
// pL, the probability of the left of two children: iL / (iL + iR), with the two phi in place of importances whose sum is not a positive
// finite number (both culled, or a light at the origin); 0.5 if that has no value either
__host__ __device__ __forceinline__ float lt_branch(const float4 l0, float phiL, const float4 r0, float phiR, float ox, float oy, float oz, float gx, float gy,
                                                    float gz) {
    float iL = lt_importance(l0, phiL, ox, oy, oz, gx, gy, gz), iR = lt_importance(r0, phiR, ox, oy, oz, gx, gy, gz);
    float s = iL + iR;
    if (!(s > 0.0f && s < __builtin_inff())) {
        iL = phiL;
        iR = phiR;
        s = iL + iR;
    }
    const float pL = iL / s;
    return pL >= 0.0f && pL <= 1.0f ? pL : 0.5f;
}
// The walk.  PICK: the leaf that u draws (returned: its tree-order light index, *P its probability); else the probability of the leaf `target`
// (*P; the same branch probabilities multiplied in the same order).  -1 and *P = 0 where there is no such leaf.  A loop of at most
// kLightTreeMaxDepth trips; every node index is tested against the count before the loads that use it
template <bool PICK>
__host__ __device__ __forceinline__ int lt_walk(const LightTreeView& v, float ox, float oy, float oz, float gx, float gy, float gz, float u, int target, float* P) {
    *P = 0.0f;
    if (v.n_nodes <= 0 || (!PICK && (unsigned)target >= (unsigned)v.n_lights)) return -1;
    float prob = 1.0f;
    int node = 0;
    float4 q1 = v.nodes[1];
    for (int trip = 0; trip <= kLightTreeMaxDepth; ++trip) {
        if (lt_bits(q1.z) <= 1) {          // a leaf
            const int s = lt_bits(q1.y);
            if ((unsigned)s >= (unsigned)v.n_lights || (!PICK && s != target)) return -1;
            *P = prob;
            return s;
        }
        const int L = node + 1, R = lt_bits(q1.w);
        if ((unsigned)L >= (unsigned)v.n_nodes || (unsigned)R >= (unsigned)v.n_nodes) return -1;
        const float4 l0 = v.nodes[2 * L], l1 = v.nodes[2 * L + 1], r0 = v.nodes[2 * R], r1 = v.nodes[2 * R + 1];
        const float pL = lt_branch(l0, l1.x, r0, r1.x, ox, oy, oz, gx, gy, gz);
        bool left;
        if constexpr (PICK) left = u < pL;
        else left = target < lt_bits(l1.y) + lt_bits(l1.z);
        if (left) {
            if constexpr (PICK) u = u / pL;
            prob *= pL;
            node = L;
            q1 = l1;
        } else {
            const float pR = 1.0f - pL;
            if constexpr (PICK) u = (u - pL) / pR;
            prob *= pR;
            node = R;
            q1 = r1;
        }
        if constexpr (PICK) if (!(u < 1.0f)) u = 0.99999994f;      // (1 - 2^-24)
    }
    return -1;
}
// normalize3 of pt_device.hpp on the host: dot3's fma placement, then a * (1.0f / sqrtf(l2)), IEEE
inline void lens_normalize(const float* a, float* out) {
    const float l2 = __builtin_fmaf(a[2], a[2], __builtin_fmaf(a[1], a[1], a[0] * a[0]));
    const float s = 1.0f / __builtin_sqrtf(l2);
    for (int i = 0; i < 3; ++i) out[i] = a[i] * s;
}
inline LensView lens_view(const pt_camera& cam, float aperture, float focus) {
    LensView lv;
    lv.aperture = aperture;
    lv.focus = focus;
    const float ahead[3] = {cam.lookat.s[0] - cam.eye.s[0], cam.lookat.s[1] - cam.eye.s[1], cam.lookat.s[2] - cam.eye.s[2]};
    lens_normalize(ahead, lv.f);
    lens_normalize(cam.right.s, lv.Rh);
    lens_normalize(cam.up.s, lv.Uh);
    return lv;
}
// the shaded guides (pt_render_aovs_ex with PT_AOV_SHADED; pt_denoise.hip): vn == nullptr: option smooth_normals is off, tv.uv == nullptr:
// option textures is off, glossy: option glossy (a terminal type-4 hit gives tint x F0), coated: option coated (a terminal type-5 hit gives tint x kd'),
// frosted: option frosted (a terminal type-6 hit gives tint x 1); lights as in launch_aovs
hipError_t launch_aovs_shaded(const RenderParams& p, int32_t subpixels, int32_t specular_depth, int64_t npix, float4* albedo_rgbm, float4* normal_depth,
                              const float4* vn, const TexView& tv, int glossy, int coated, int frosted, const AreaLightsView* lights, int cu_count,
                              hipStream_t stream);
// one launch of the NEE kernels (pt_nee.hip), as nee_launch_for (pt_context.hpp) fills it from the context.  Each family is the one before it
// with one more feature compiled in; a launch takes the first family that covers what the frame needs
enum NeeFamily { kNeePlain, kNeeSmooth, kNeeTex, kNeeGlossy, kNeeCoated, kNeeLens, kNeeFrosted, kNeeLights, kNeeMedium, kNeeGrid, kNeeInterior, kNeeLightTree, kNeeAreaLights };
// the families compiled in translation units of their own, as the preprocessor needs them (pt_nee.hip's PT_NEE_TU)
#define PT_NEE_FAMILY_MEDIUM 8
#define PT_NEE_FAMILY_GRID 9
#define PT_NEE_FAMILY_INTERIOR 10
#define PT_NEE_FAMILY_LIGHTTREE 11
#define PT_NEE_FAMILY_AREALIGHTS 12
static_assert(PT_NEE_FAMILY_AREALIGHTS == kNeeAreaLights, "the PT_NEE_FAMILY_* macros are the NeeFamily values");
static_assert(PT_NEE_FAMILY_MEDIUM == kNeeMedium && PT_NEE_FAMILY_GRID == kNeeGrid && PT_NEE_FAMILY_INTERIOR == kNeeInterior && PT_NEE_FAMILY_LIGHTTREE == kNeeLightTree,
              "the PT_NEE_FAMILY_* macros are the NeeFamily values");
// NeeLaunch::flags: what is live in the launch, for the families in which that is a run-time answer (a family below reads none of it: there the
// feature is either compiled out or what the family was chosen for)
enum NeeFlag : int {
    kNeeFlagGlossy = 1,          // option glossy: type 4 is live (read from kNeeCoated on)
    kNeeFlagCoated = 2,          // option coated: type 5 is live (from kNeeLens on)
    kNeeFlagLens = 4,            // a lens with aperture > 0 is set (from kNeeFrosted on; else each sample starts on the pinhole ray)
    kNeeFlagFrosted = 8,         // option frosted with a type-6 material uploaded: type 6 is live (from kNeeLights on)
    kNeeFlagLights = 16,         // a light set with a pickable light is held (from kNeeMedium on; else `lights` is an empty set with P_ana = 0)
    kNeeFlagMedium = 32,         // a medium with sigma_t > 0 is held (from kNeeInterior on, which serves frames without one)
    kNeeFlagGrid = 64,           // ... and its density grid is live (from kNeeInterior on)
    kNeeFlagInterior = 128,      // an interior binding is live (kNeeLightTree; else `interior` is never read)
    kNeeFlagLightTree = 256,     // option light_tree with a non-empty light table: the tree is walked (kNeeAreaLights, which serves frames without
                                 // one; else `ltree` is never read and the table's cdf picks)
};
struct NeeLaunch {
    const EnvView* env;          // null: the instances without an environment
    bool tiled;                  // the rounds of pt_render_adaptive_ex: the tiled instances over the p.n_tiles 8x8 frame tiles of p.tile_list (null:
                                 // the frame's tiles in order), one lane per pixel of a tile; npix is then not read
    int family;                  // NeeFamily.  An option whose material type is not uploaded asks for nothing; a lens with aperture > 0 takes
                                 // kNeeLens whatever the options say; option frosted with a type-6 material takes kNeeFrosted, lens or not;
                                 // a light set with a pickable light (pt_set_lights) takes kNeeLights whatever else is on; a medium with
                                 // sigma_t > 0 (pt_set_medium) takes kNeeMedium whatever else is on, lights or not; a live density grid
                                 // (pt_set_medium_density with such a medium) takes kNeeGrid whatever else is on; a live interior binding
                                 // (pt_set_material_interior) takes kNeeInterior whatever else is on, medium and grid or not; option light_tree
                                 // with a non-empty light table takes kNeeLightTree whatever else is on, an interior binding or not; an area
                                 // set with a non-black light (pt_set_area_lights) takes kNeeAreaLights whatever else is on, a tree or not
    const float4* vn;            // the packed vertex normals (from kNeeSmooth on); null: option smooth_normals is off, which the families from
                                 // kNeeTex on read as "no triangle has vertex normals" (the pinned rule "no vertex normals: Ns = Ng, the same bits"
                                 // makes that exact)
    TexView tv;                  // from kNeeTex on; uv == null: option textures is off (no lookup in the families from kNeeGlossy on)
    int flags;                   // NeeFlag bits
    LensView lens;               // read from kNeeLens on
    LightsView lights;           // read from kNeeLights on
    MediumView medium;           // read from kNeeMedium on
    GridView grid;               // read from kNeeGrid on
    InteriorView interior;       // read from kNeeInterior on
    LightTreeView ltree;         // read from kNeeLightTree on
    AreaLightsView area;         // read by kNeeAreaLights
    int* block;                  // out, may be null: the workgroup size the launch took, as launch_lanes / launch_lanes_wide chose it (0: nothing
                                 // was launched, an empty tile list)
};
hipError_t launch_nee(const RenderParams& p, const NeeTable& lt, const NeeLaunch& nl, int64_t npix, int cu_count, hipStream_t stream);
// thin lens (pt_lens.hip): pt_debug_lens's kernel, {gid, S} in and 6 floats out per item; pt_focus_at's, the axial distance of pixel gid's
// centre-ray hit into *out (+inf: a miss)
hipError_t launch_debug_lens(const pt_camera& cam, const LensView& lv, const int32_t* gid_state, int64_t n, float* out, hipStream_t stream);
hipError_t launch_focus_at(const RenderParams& p, const LensView& lv, int32_t gid, float* out, int cu_count, hipStream_t stream);
// albedo textures (pt_texture.hip): add-order uvs (6 floats per triangle, n_src triangles; the rest has none) -> 2 float4 per packed triangle
hipError_t launch_pack_vertex_uvs(const float* src, int64_t n_src, const int32_t* orig, int32_t n, float4* out, hipStream_t stream);
hipError_t launch_debug_albedo(const RenderParams& p, const float4* vn, const TexView& tv, const pt_ray* rays, int64_t n, int32_t* out_tri, float4* out_rgbt,
                               int cu_count, hipStream_t stream);
// rough metal (pt_glossy.hip): pt_debug_glossy's kernel, 9 floats in and 8 out per item
hipError_t launch_debug_glossy(const float* in, int64_t n, float* out, hipStream_t stream);
// homogeneous medium (pt_medium.hip): pt_debug_medium's kernel, 12 floats in and 10 out per item
hipError_t launch_debug_medium(const MediumView& mv, const float* in, int64_t n, float* out, hipStream_t stream);
// density grid (pt_medium.hip): pt_debug_grid's kernel, 12 floats in and 8 out per item
hipError_t launch_debug_grid(const MediumView& mv, const GridView& gv, const float* in, int64_t n, float* out, hipStream_t stream);
// interiors (pt_medium.hip): pt_debug_interior's kernel, 12 floats in and 10 out per item
hipError_t launch_debug_interior(const float* in, int64_t n, float* out, hipStream_t stream);
// light hierarchy (pt_nee_lighttree.hip): pt_debug_light_tree_eval's kernel, per item {o, G, u0} (7 floats) and a tree-order target in,
// {picked tree-order light, bits(P), bits(the weight walk's P of the target), 0} out
hipError_t launch_debug_light_tree(const LightTreeView& v, const float* in, const int32_t* target, int64_t n, int32_t* out, hipStream_t stream);
// area lights (pt_nee_arealights.hip): pt_debug_area_light_eval's kernel: n_s sample items {o, bits(light), u1, u2} (6 floats) -> {w, p_omega, t_s,
// bits(accept)} (6 words) and n_h hit items {o, d, t_max} (7 floats) -> {sphere, bits(t), suns lo, suns hi} (4 words)
hipError_t launch_debug_area_light(const AreaLightsView& v, const float* s_in, int64_t n_s, int32_t* s_out, const float* h_in, int64_t n_h, int32_t* h_out,
                                   hipStream_t stream);
// coated diffuse (pt_glossy.hip): pt_debug_coated's kernel, 12 floats in and 10 out per item
hipError_t launch_debug_coated(const float* in, int64_t n, float* out, hipStream_t stream);
// rough dielectric (pt_glossy.hip): pt_debug_frosted's kernel, 12 floats in and 10 out per item
hipError_t launch_debug_frosted(const float* in, int64_t n, float* out, hipStream_t stream);
// smooth shading (pt_smooth.hip): add-order normals (9 floats per triangle, n_src triangles; the rest has none) -> 3 float4 per packed triangle
hipError_t launch_pack_vertex_normals(const float* src, int64_t n_src, const int32_t* orig, int32_t n, float4* out, hipStream_t stream);
hipError_t launch_debug_shading_normal(const RenderParams& p, const float4* vn, const pt_ray* rays, int64_t n, int32_t* out_tri, float4* out_ns, int cu_count,
                                       hipStream_t stream);
// the texel of unit direction (x, y, z): k_nee and pt_env_lookup
__host__ __device__ __forceinline__ void env_texel(int32_t w, int32_t h, float yaw, float x, float y, float z, int32_t* row, int32_t* col) {
    const float theta = acosf(fminf(fmaxf(y, -1.0f), 1.0f));
    const float phi = atan2f(z, x) - yaw;
    const int r = (int)floorf(theta / 3.14159265358979323846f * (float)h);
    const float turn = phi / 6.28318530717958647692f;
    const int c = (int)floorf((turn - floorf(turn)) * (float)w);
    *row = r < h - 1 ? (r < 0 ? 0 : r) : h - 1;
    *col = c < w - 1 ? (c < 0 ? 0 : c) : w - 1;
}
// the light samples' counter-based hash of (LCG state at the start of the sample, segment, dimension): k_nee and pt_nee_rand
__host__ __device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
__host__ __device__ __forceinline__ uint32_t nee_rand(uint32_t state, int segment, int dim) {
    return lowbias32(lowbias32(state) + 0x9e3779b9u * (uint32_t)(3 * segment + dim + 1));
}

// temporal accumulation (pt_temporal.hip; pinned in include/pt_api.h next to pt_temporal_accumulate)
struct TemporalArgs {
    pt_camera cur, prev;           // the frame's view, the history's view
    const float4* colors;          // the frame: .xyz the mean, .w the second moment
    const int32_t* tile_spp;       // samples per 8x8 tile of an adaptive frame, or null: n_all for every pixel
    int32_t n_all;
    const float4* albedo;          // the current guides: albedo_rgbm (.w the material index), normal_depth
    const float4* nd;
    const float4* prev_c;          // the previous set (read only when has_prev): {r, g, b, m2}, {nx, ny, nz, depth}, {n, material}
    const float4* prev_g;
    const float2* prev_nm;
    float4* out_c;                 // the new set, same layout, and the variance of the mean
    float4* out_g;
    float2* out_nm;
    float* out_v;
    int32_t W, H;                  // the frame (one rank: local pixel = global pixel id)
    int32_t has_prev;
    float max_history, normal_cos, depth_tolerance;
};
hipError_t launch_temporal(const TemporalArgs& a, hipStream_t stream);
// the variance-gated firefly filter (pt_despeckle.hip; pinned in include/pt_api.h next to pt_despeckle)
struct DespeckleArgs {
    const float4* c;               // the input colour, .xyz
    const float* v;                // the variance of its mean luminance, or null: c[].w
    float4* out;                   // {r, g, b, v}
    float* out_v;                  // v once more, 4 B per pixel (what the variance-guided filter's first iteration reads), or null
    int32_t* flags;
    int32_t W, H;
    int32_t rank;
    float threshold, floor_, min_rel_sigma;
};
hipError_t launch_despeckle(const DespeckleArgs& a, int32_t radius, int32_t spread, hipStream_t stream);
// the display stage (pt_display.hip; pinned in include/pt_api.h next to pt_display)
struct DisplayStat {               // what one pt_display leaves on the device: the histogram and the metering's numbers
    uint32_t hist[256];
    uint32_t n_dark, n_nonfinite, n_metered;
    float exposure, mean_log2;     // exposure is also the remembered E_prev of the next call
    uint32_t pad[3];
};
constexpr size_t kDisplayStatCounters = 259;       // the words launch_display clears: hist, n_dark, n_nonfinite, n_metered
constexpr int kDisplayMaxLevels = 6;
struct DisplayArgs {
    const float4* c;               // the input colour, .xyz
    int32_t W, H;
    DisplayStat* stat;
    float4* out;                   // {r, g, b, 1}
    uint8_t* rgb8;                 // 3 B per pixel, top row first; 4-byte aligned
    float4* pyr;                   // display_pyramid_elems(W, H, levels) float4: the levels D_1 .. D_levels, U_k written over D_k
    int32_t metering;
    float ev, key;
    int32_t low_permille, high_permille;
    float min_ev, max_ev, adapt;
    int32_t prev_mode;             // E_prev: 0 none, 1 stat->exposure as the last call left it, 2 prev_value
    float prev_value;
    int32_t levels;                // bloom levels to run, 0: no bloom
    float threshold, intensity;
    int32_t curve;
    float white;
    int32_t encoding;
};
inline size_t display_pyramid_elems(int32_t W, int32_t H, int32_t levels) {
    size_t n = 0;
    for (int k = 1; k <= levels; ++k) {
        W = (W + 1) / 2;
        H = (H + 1) / 2;
        n += (size_t)W * (size_t)H;
    }
    return n;
}
// clears the counters, then histogram, metering and (levels > 0) the pyramid, then the final kernel, all on stream; no host synchronise
hipError_t launch_display(const DisplayArgs& a, hipStream_t stream);
// float32 dot / cross with the fma placement of pt_device.hpp's dot3 / cross3
__host__ __device__ __forceinline__ float rp_dot(const float* a, const float* b) { return __builtin_fmaf(a[2], b[2], __builtin_fmaf(a[1], b[1], a[0] * b[0])); }
__host__ __device__ __forceinline__ void rp_cross(const float* a, const float* b, float* r) {
    r[0] = __builtin_fmaf(a[1], b[2], -(a[2] * b[1]));
    r[1] = __builtin_fmaf(a[2], b[0], -(a[0] * b[2]));
    r[2] = __builtin_fmaf(a[0], b[1], -(a[1] * b[0]));
}
// The reprojection of k_temporal and pt_debug_reproject: global pixel gid's centre ray under cur -- camera_get_ray(gid, cur, 0.5f, 0.5f)
// bit for bit (1 / sqrt rounds as normalize3's rsqrt_rn does) -- followed to depth, in prev's view: out = {x', y', |X - eye_prev|}.
// false when X is not in front of prev (a <= 0, or a is not finite).
__host__ __device__ inline bool reproject(const pt_camera& cur, const pt_camera& prev, int gid, float depth, float out[3]) {
    const int X = (int)cur.XM, Y = (int)cur.YM;
    const float sx = (2.0f * ((float)(gid % X) + 0.5f)) / (float)X - 1.0f;
    const float sy = (2.0f * ((float)(gid / X) + 0.5f)) / (float)Y - 1.0f;
    float d[3], v[3], ahead[3];
    for (int i = 0; i < 3; ++i) d[i] = ((cur.lookat.s[i] + cur.right.s[i] * sx) + cur.up.s[i] * sy) - cur.eye.s[i];
    const float inv = 1.0f / __builtin_sqrtf(rp_dot(d, d));
    for (int i = 0; i < 3; ++i) {
        v[i] = __builtin_fmaf(depth, d[i] * inv, cur.eye.s[i]) - prev.eye.s[i];
        ahead[i] = prev.lookat.s[i] - prev.eye.s[i];
    }
    // v = a ahead + b right + c up by Cramer's rule: det = ahead . (right x up), a = v . (right x up) / det,
    // b = ahead . (v x up) / det, c = ahead . (right x v) / det
    float ru[3], vu[3], rv[3];
    rp_cross(prev.right.s, prev.up.s, ru);
    rp_cross(v, prev.up.s, vu);
    rp_cross(prev.right.s, v, rv);
    const float det = rp_dot(ahead, ru);
    const float a = rp_dot(v, ru) / det;
    if (!(a > 0.0f && a < __builtin_inff())) return false;
    const float u = (rp_dot(ahead, vu) / det) / a, w = (rp_dot(ahead, rv) / det) / a;
    out[0] = ((u + 1.0f) * prev.XM) * 0.5f - 0.5f;
    out[1] = ((w + 1.0f) * prev.YM) * 0.5f - 0.5f;
    out[2] = __builtin_sqrtf(rp_dot(v, v));
    return true;
}

}  // namespace ptamd
