// pt_obj.cpp -- OBJ/MTL import with the reference's conventions (Scene::add_Obj,
// main.cpp:552-617).  The reference parses with the vendored tiny_obj_loader.h v1.0.3; this is
// an own minimal reader that reproduces the parts of its behaviour add_Obj depends on:
//   * v / f records; f accepts i, i/j, i//k, i/j/k; negative (relative) indices
//     (tiny_obj_loader.h:410-414); polygons are fan-triangulated (tiny_obj_loader.h:893-916)
//   * numbers: the token's shape is the reference's grammar (tiny_obj_loader.h:437-443: sign, digits, optional fraction,
//     optional non-empty exponent; anything else is the default 0, so `.5`, `nan`, `inf`, `1e`, `0x10` read as 0), its value
//     strtod's -- on the number forms exporters write the two give the same float (tests/golden/obj/numbers.obj)
//   * shapes are split on g / o (tiny_obj_loader.h:1509-1567); usemtl switches the per-face
//     material without starting a new shape (tiny_obj_loader.h:1452-1478)
//   * MTL: newmtl, Kd, Ks, Ke, Ns; every other "key value" line is kept as a string, first
//     occurrence wins (tiny_obj_loader.h:1258-1269); defaults per tiny_obj_loader.h:838-873
//   * add_Obj itself: custom keys Kn / Kk (three floats, split on single blanks, atof) and
//     Tp (atoi) are REQUIRED (main.cpp:568-571 uses .at()); x is negated, then rotate_x(pitch),
//     rotate_y(yaw), scale, translate (main.cpp:598-606); one end_Obj per shape (main.cpp:615).
// New (the reference throws vn away): a face whose corners all carry a vn index records those normals for its fan triangles
// (pt_set_vertex_normals; include/pt_api.h), transformed by the inverse transpose of the positions' linear map.  The triangles
// themselves are what they were.
// New as well (the reference throws vt and map_Kd away): a face whose corners all carry a vt index records those uvs for its fan
// triangles (pt_set_vertex_uvs), and a material's map_Kd -- a .ppm or .pfm next to the MTL -- becomes a texture bound to the material
// pt_add_obj creates (pt_add_texture / pt_set_material_texture; include/pt_api.h).  A map that cannot be used leaves the material as it was.
// In a vt or vn position an index 0 (or nothing behind the slash) means "no index" here; the reference's fixIndex reads it as the first element.
// Deviations, all turning undefined behaviour of the reference into errors: a missing
// Kn/Kk/Tp, a face without usemtl (material id -1) and an empty shape return PT_EIO.
#include "pt_context.hpp"
#include "pt_internal.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

namespace ptamd {
int fail_ctx(pt_context* ctx, int code, const std::string& msg);   // pt_host.cpp
int append_triangles(pt_context* ctx, int64_t n, pt_triangle** tail);
}

namespace {

struct MtlRec {
    std::string name;
    float diffuse[3] = {0, 0, 0}, specular[3] = {0, 0, 0}, emission[3] = {0, 0, 0};
    float shininess = 1.0f;                         // tiny_obj_loader.h:858
    std::map<std::string, std::string> unknown;
    std::string map_kd;                             // the file of the last usable map_Kd line
    int map_kd_skipped = 0;                         // map_Kd lines with a -option token
};

inline bool is_space(char c) { return c == ' ' || c == '\t'; }

// The whole file in one buffer, NUL-terminated; lines are visited in place (a 1M-triangle OBJ is 50 MB and 1.5 M lines:
// one std::string per line and per number was most of pt_add_obj's 1.3 s, profiles/r03/e_*).
bool read_file(const std::string& path, std::vector<char>* buf) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    if (n < 0) { std::fclose(f); return false; }
    buf->resize((size_t)n + 1);
    const size_t got = n ? std::fread(buf->data(), 1, (size_t)n, f) : 0;
    std::fclose(f);
    if (got != (size_t)n) return false;
    (*buf)[(size_t)n] = '\0';
    return true;
}

// Next line of the buffer: [*cur, end) with the terminator (\n, \r\n or a lone \r) replaced by NUL; false at the end.
// (An empty last line after the final terminator is not a line, as before.)
bool next_line(char** cur, char* end, char** line) {
    char* p = *cur;
    if (p >= end) return false;
    *line = p;
    while (p < end && *p != '\n' && *p != '\r') ++p;
    if (p < end) {
        const char c = *p;
        *p = '\0';
        ++p;
        if (c == '\r' && p < end && *p == '\n') ++p;
    }
    *cur = p;
    return true;
}

// One number: the token runs to the next blank / tab (lines are NUL-terminated in the buffer); its value is what strtod
// makes of the token's prefix where the reference's grammar accepts one, else 0.  strtod runs on the buffer itself -- it stops at the blank or NUL that
// ends the token, so the copy into a std::string that used to precede it bought nothing.  (std::from_chars is no
// alternative with this toolchain: libstdc++ 11 implements it as newlocale + strtod per call, slower and serialised on
// the locale lock -- the parallel parse did not scale at all with it, profiles/r03/e_*.)
float parse_float(const char** tok) {
    const char* t = *tok;
    t += std::strspn(t, " \t");
    const char* end = t + std::strcspn(t, " \t");
    *tok = end;
    if (t == end) return 0.0f;
    // the token's shape first, as the reference's grammar has it (tiny_obj_loader.h:437-443): [sign] digits [. [digits]]
    // [e|E [sign] digits], read greedily; no digit after the sign, or an e / E without digits behind it, gives the default 0
    // (`.5`, `nan`, `inf`, `1e`, `1e+`), and what follows a well-formed prefix is ignored (`1.5.3` is 1.5, `12abc` is 12).
    // strtod agrees with that on every prefix but a hexadecimal one, which the grammar ends after its `0`.
    const char* p = t;
    if (*p == '+' || *p == '-') ++p;
    const char* digits = p;
    while (*p >= '0' && *p <= '9') ++p;
    if (p == digits) return 0.0f;
    if ((*p == 'x' || *p == 'X') && p == digits + 1 && *digits == '0') return *t == '-' ? -0.0f : 0.0f;
    if (*p == '.') { ++p; while (*p >= '0' && *p <= '9') ++p; }
    if (*p == 'e' || *p == 'E') {
        ++p;
        if (*p == '+' || *p == '-') ++p;
        if (!(*p >= '0' && *p <= '9')) return 0.0f;
    }
    return (float)std::strtod(t, nullptr);
}

void parse_float3(float out[3], const char** tok) {
    out[0] = parse_float(tok);
    out[1] = parse_float(tok);
    out[2] = parse_float(tok);
}

// atoi: optional blanks, optional sign, digits; stops at the first other character
inline int parse_int(const char* t) {
    while (*t == ' ' || *t == '\t' || *t == '\n' || *t == '\v' || *t == '\f' || *t == '\r') ++t;
    bool neg = false;
    if (*t == '-' || *t == '+') { neg = *t == '-'; ++t; }
    unsigned v = 0;
    while (*t >= '0' && *t <= '9') { v = v * 10u + (unsigned)(*t - '0'); ++t; }
    return neg ? (int)(0u - v) : (int)v;
}

bool load_mtl(const std::string& path, std::vector<MtlRec>* mats, std::map<std::string, int>* index) {
    std::vector<char> buf;
    if (!read_file(path, &buf)) return false;
    char* cur_p = buf.data();
    char* const end_p = buf.data() + buf.size() - 1;
    char* raw = nullptr;
    MtlRec cur;
    bool have = false;
    while (next_line(&cur_p, end_p, &raw)) {
        const char* t = raw;
        t += std::strspn(t, " \t");
        if (*t == '\0' || *t == '#') continue;
        if (0 == std::strncmp(t, "newmtl", 6) && is_space(t[6])) {
            if (have || !cur.name.empty()) {
                index->insert(std::make_pair(cur.name, (int)mats->size()));
                mats->push_back(cur);
            }
            cur = MtlRec();
            t += 7;
            t += std::strspn(t, " \t");
            cur.name = std::string(t, std::strcspn(t, " \t"));
            have = true;
            continue;
        }
        if (t[0] == 'K' && t[1] == 'd' && is_space(t[2])) { t += 2; parse_float3(cur.diffuse, &t); continue; }
        if (t[0] == 'K' && t[1] == 's' && is_space(t[2])) { t += 2; parse_float3(cur.specular, &t); continue; }
        if (t[0] == 'K' && t[1] == 'e' && is_space(t[2])) { t += 2; parse_float3(cur.emission, &t); continue; }
        if (t[0] == 'N' && t[1] == 's' && is_space(t[2])) { t += 2; cur.shininess = parse_float(&t); continue; }
        if (0 == std::strncmp(t, "map_Kd", 6) && is_space(t[6])) {      // the last blank-separated token; a line with an option is skipped
            const char* q = t + 6;
            std::string last;
            bool option = false;
            for (;;) {
                q += std::strspn(q, " \t");
                if (*q == '\0') break;
                const size_t n = std::strcspn(q, " \t");
                if (*q == '-') option = true;
                last.assign(q, n);
                q += n;
            }
            if (option) ++cur.map_kd_skipped;
            else if (!last.empty()) cur.map_kd = last;
            continue;
        }
        // keys tinyobj knows but add_Obj never reads
        static const char* known[] = {"Ka", "Kt", "Tf", "Ni", "illum", "d", "Tr", "Pr", "Pm", "Ps", "Pc", "Pcr", "aniso", "anisor",
                                      "map_Ka", "map_Kd", "map_Ks", "map_Ns", "map_bump", "bump", "map_d", "disp", "refl",
                                      "map_Pr", "map_Pm", "map_Ps", "map_Ke", "norm"};
        bool skip = false;
        for (const char* k : known) {
            size_t n = std::strlen(k);
            if (0 == std::strncmp(t, k, n) && is_space(t[n])) { skip = true; break; }
        }
        if (skip) continue;
        const char* sp = std::strchr(t, ' ');
        if (!sp) sp = std::strchr(t, '\t');
        if (sp) cur.unknown.insert(std::make_pair(std::string(t, (size_t)(sp - t)), std::string(sp + 1)));
    }
    index->insert(std::make_pair(cur.name, (int)mats->size()));   // tinyobj flushes the last material unconditionally
    mats->push_back(cur);
    return true;
}

// main.cpp:72-86: split on single blanks, atof the first three fields
bool str_to_float3(const std::string& s, float out[3]) {
    std::vector<std::string> arr;
    std::stringstream ss(s);
    std::string item;
    while (std::getline(ss, item, ' ')) arr.push_back(item);
    if (arr.size() < 3) return false;
    for (int i = 0; i < 3; ++i) out[i] = (float)std::atof(arr[i].c_str());
    return true;
}

int fix_index(int idx, int n) {        // tiny_obj_loader.h:410-414
    if (idx > 0) return idx - 1;
    if (idx == 0) return 0;
    return n + idx;
}

void rot_x(float v[3], float gamma) {   // main.cpp:63-70
    gamma = gamma / 180.0f * 3.141593f;
    const double c = std::cos((double)gamma), s = std::sin((double)gamma);
    const float r1 = (float)((double)v[1] * c - (double)v[2] * s);
    const float r2 = (float)((double)v[1] * s + (double)v[2] * c);
    v[1] = r1; v[2] = r2;
}
void rot_y(float v[3], float beta) {    // main.cpp:55-62
    beta = beta / 180.0f * 3.141593f;
    const double c = std::cos((double)beta), s = std::sin((double)beta);
    const float r0 = (float)((double)v[0] * c + (double)v[2] * s);
    const float r2 = (float)(-(double)v[0] * s + (double)v[2] * c);
    v[0] = r0; v[2] = r2;
}

constexpr int kNoVn = INT32_MIN;      // a face corner without a vn index
// the vn of v//vn or v/vt/vn in the token at t (kNoVn: none)
inline int parse_vn(const char* t) {
    const char* e = t + std::strcspn(t, " \t");
    const char* s1 = (const char*)std::memchr(t, '/', (size_t)(e - t));
    if (!s1) return kNoVn;
    const char* s2 = (const char*)std::memchr(s1 + 1, '/', (size_t)(e - (s1 + 1)));
    if (!s2 || s2 + 1 >= e) return kNoVn;
    return parse_int(s2 + 1);
}

// the vt of v/vt or v/vt/vn in the token at t (kNoVn: none)
inline int parse_vt(const char* t) {
    const char* e = t + std::strcspn(t, " \t");
    const char* s1 = (const char*)std::memchr(t, '/', (size_t)(e - t));
    if (!s1 || s1 + 1 >= e || s1[1] == '/') return kNoVn;
    return parse_int(s1 + 1);
}

bool ends_with_nocase(const std::string& s, const char* ext) {
    const size_t n = std::strlen(ext);
    if (s.size() < n) return false;
    for (size_t i = 0; i < n; ++i)
        if (std::tolower((unsigned char)s[s.size() - n + i]) != ext[i]) return false;
    return true;
}

// a map_Kd file as a texture of ctx: its index, or -1 when it cannot be used (another format, unreadable, refused by pt_add_texture)
int load_albedo_map(pt_context* ctx, const std::string& path) {
    const bool ppm = ends_with_nocase(path, ".ppm"), pfm = ends_with_nocase(path, ".pfm");
    if (!ppm && !pfm) return -1;
    int32_t w = 0, h = 0;
    if ((ppm ? pt_image_read_ppm(path.c_str(), nullptr, 0, &w, &h) : pt_image_read_pfm(path.c_str(), nullptr, 0, &w, &h)) != PT_OK) return -1;
    if (w < 1 || h < 1 || w > PT_TEX_MAX_SIZE || h > PT_TEX_MAX_SIZE) return -1;
    const size_t n = (size_t)w * (size_t)h;
    std::vector<float> rgb(n * 3);
    if (ppm) {
        if (pt_image_read_ppm(path.c_str(), rgb.data(), (int64_t)n, &w, &h) != PT_OK) return -1;
    } else {
        std::vector<float> rgba(n * 4);
        if (pt_image_read_pfm(path.c_str(), rgba.data(), (int64_t)n, &w, &h) != PT_OK) return -1;
        for (int32_t y = 0; y < h; ++y)                      // the file's rows run bottom to top
            for (int32_t x = 0; x < w; ++x)
                for (int c = 0; c < 3; ++c) rgb[((size_t)y * w + x) * 3 + c] = rgba[((size_t)(h - 1 - y) * w + x) * 4 + c];
    }
    const pt_texture_params tp = {1, ppm ? 1 : 0};
    const std::string keep = pt_last_error(ctx);            // (a refused map is no error of pt_add_obj)
    const int t = pt_add_texture(ctx, rgb.data(), w, h, &tp);
    if (t < 0) ctx->err = keep;
    return t < 0 ? -1 : t;
}

struct Face3 { int v[3]; int mat; int vn[3]; int vt[3]; };      // vn, vt: resolved index, or -1
struct Shape { std::vector<Face3> faces; };

// run fn(begin, end) over [0, n) on up to 16 threads (element-wise work: any split gives the same result)
template <class F>
void parallel_ranges(size_t n, size_t grain, F fn) {
    unsigned hw = std::thread::hardware_concurrency();
    size_t nt = std::min<size_t>(std::min<size_t>(hw ? hw : 1, 16), (n + grain - 1) / std::max<size_t>(grain, 1));
    if (nt <= 1) { fn((size_t)0, n); return; }
    std::vector<std::thread> th;
    const size_t per = (n + nt - 1) / nt;
    for (size_t k = 0; k < nt; ++k) {
        const size_t b = k * per, e = std::min(n, b + per);
        if (b < e) th.emplace_back([=]() { fn(b, e); });
    }
    for (std::thread& t : th) t.join();
}

}  // namespace

extern "C" int pt_add_obj(pt_context* ctx, const char* file, const float pos[3], const float scale[3], float pitch, float yaw) {
    using ptamd::fail_ctx;
    if (!ctx || !file || !pos || !scale) return PT_EINVAL;
    const std::string path(file);
    const std::string matpath = path.substr(0, path.find_last_of('/') + 1);   // main.cpp:553
    std::vector<char> buf;
    ptamd::PhaseClock clk("pt_add_obj");
    if (!read_file(path, &buf)) return fail_ctx(ctx, PT_EIO, "cannot open OBJ file: " + path);
    clk.lap("read file");

    // ---- parse.  Three steps, so that a 50-MB file is read by every core and still means what tinyobj's single pass says:
    //  A (parallel)  the buffer is cut at line ends into pieces; each piece turns its `v` lines into floats and its `f`
    //                lines into fan triangles of RAW indices (tiny_obj_loader.h:893-916) and notes, in order, the lines
    //                that change state: usemtl, mtllib, g / o, and faces of fewer than three vertices;
    //  B (serial)    the state machine over those notes: current material, whether the face group is open, which
    //                shape a run of triangles belongs to and whether that shape survives (below);
    //  C (parallel)  relative indices are resolved against the number of vertices read in front of each face
    //                (tiny_obj_loader.h:410-414) and the runs are copied to their shapes.
    // tinyobj collects the faces of the current material in a group and exports it (exportFaceGroupToShape with
    // triangulate = true) when the material changes, at g / o and at the end of the file; g / o keeps the shape only if
    // the group it closes is not empty (tiny_obj_loader.h:1509-1567) -- faces exported by an earlier usemtl are lost
    // with it, which B reproduces.  A face of fewer than three vertices opens the group and exports nothing.
    struct RawTri { int idx[3]; int nv_local; int vn[3]; int nvn_local; int vt[3]; int nvt_local; };
    enum { kEvUsemtl = 0, kEvMtllib = 1, kEvShape = 2, kEvShortFace = 3 };
    struct Event { int kind; size_t tri_pos; std::string name; };
    struct Piece {
        char* begin = nullptr;
        char* end = nullptr;
        std::vector<float> v, vn, vt;
        std::vector<RawTri> tris;
        std::vector<Event> ev;
    };
    char* const file_begin = buf.data();
    char* const file_end = buf.data() + buf.size() - 1;
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t n_pieces = std::max<size_t>(1, std::min<size_t>((size_t)std::min<unsigned>(hw ? hw : 1u, 16u) * 4, (size_t)(file_end - file_begin) >> 16));
    std::vector<Piece> pieces(n_pieces);
    ctx->obj_pieces = (int)n_pieces;
    {
        char* start = file_begin;
        for (size_t k = 0; k < n_pieces; ++k) {
            pieces[k].begin = start;
            char* stop = file_end;
            if (k + 1 < n_pieces) {
                stop = std::max(start, file_begin + (size_t)(file_end - file_begin) * (k + 1) / n_pieces);
                while (stop < file_end && *stop != '\n' && *stop != '\r') ++stop;
                if (stop < file_end) {
                    const char c = *stop++;
                    if (c == '\r' && stop < file_end && *stop == '\n') ++stop;
                }
            }
            pieces[k].end = stop;
            start = stop;
        }
    }
    auto parse_piece = [](Piece& pc) {
        pc.v.reserve((size_t)(pc.end - pc.begin) / 24);
        pc.tris.reserve((size_t)(pc.end - pc.begin) / 20);
        char* cur_p = pc.begin;
        char* raw = nullptr;
        while (next_line(&cur_p, pc.end, &raw)) {
            const char* t = raw;
            t += std::strspn(t, " \t");
            if (*t == '\0' || *t == '#') continue;
            if (t[0] == 'v' && is_space(t[1])) {
                t += 2;
                float p[3];
                parse_float3(p, &t);
                pc.v.push_back(p[0]); pc.v.push_back(p[1]); pc.v.push_back(p[2]);
                continue;
            }
            if (t[0] == 'v' && t[1] == 'n' && is_space(t[2])) {
                t += 3;
                float p[3];
                parse_float3(p, &t);
                pc.vn.push_back(p[0]); pc.vn.push_back(p[1]); pc.vn.push_back(p[2]);
                continue;
            }
            if (t[0] == 'v' && t[1] == 't' && is_space(t[2])) {
                t += 3;
                const float u = parse_float(&t), vv = parse_float(&t);      // (an optional w is not read)
                pc.vt.push_back(u); pc.vt.push_back(vv);
                continue;
            }
            if (t[0] == 'f' && is_space(t[1])) {
                t += 2;
                t += std::strspn(t, " \t");
                const int nv_local = (int)(pc.v.size() / 3), nvn_local = (int)(pc.vn.size() / 3), nvt_local = (int)(pc.vt.size() / 2);
                int first = 0, prev = 0, count = 0, nfirst = kNoVn, nprev = kNoVn, tfirst = kNoVn, tprev = kNoVn;
                while (*t != '\0') {
                    const int idx = parse_int(t);                         // the v of v, v/vt, v//vn, v/vt/vn
                    const int nidx = parse_vn(t), tidx = parse_vt(t);
                    if (count == 0) { first = idx; nfirst = nidx; tfirst = tidx; }
                    else if (count >= 2) pc.tris.push_back(RawTri{{first, prev, idx}, nv_local, {nfirst, nprev, nidx}, nvn_local, {tfirst, tprev, tidx}, nvt_local});   // fan: (first, previous, this)
                    prev = idx;
                    nprev = nidx;
                    tprev = tidx;
                    ++count;
                    t += std::strcspn(t, " \t");
                    t += std::strspn(t, " \t");
                }
                if (count < 3) pc.ev.push_back(Event{kEvShortFace, pc.tris.size(), std::string()});
                continue;
            }
            const bool usemtl = 0 == std::strncmp(t, "usemtl", 6) && is_space(t[6]);
            if (usemtl || (0 == std::strncmp(t, "mtllib", 6) && is_space(t[6]))) {
                t += 7;
                t += std::strspn(t, " \t");
                pc.ev.push_back(Event{usemtl ? kEvUsemtl : kEvMtllib, pc.tris.size(), std::string(t, std::strcspn(t, " \t"))});
                continue;
            }
            if ((t[0] == 'g' || t[0] == 'o') && is_space(t[1])) pc.ev.push_back(Event{kEvShape, pc.tris.size(), std::string()});
            // s, t ...: nothing add_Obj reads
        }
    };
    {
        std::atomic<size_t> next(0);
        std::vector<std::thread> th;
        const size_t nt = std::min<size_t>(n_pieces, std::min<unsigned>(hw ? hw : 1u, 16u));
        auto worker = [&]() {
            for (;;) {
                const size_t k = next.fetch_add(1);
                if (k >= n_pieces) return;
                parse_piece(pieces[k]);
            }
        };
        for (size_t k = 1; k < nt; ++k) th.emplace_back(worker);
        worker();
        for (std::thread& t : th) t.join();
    }
    clk.lap("parse: pieces");

    // B: the state machine
    std::vector<MtlRec> mtls;
    std::map<std::string, int> mtl_index;
    struct Run { size_t piece, tri_begin, tri_end; int material; size_t shape; size_t dst; };
    std::vector<Run> runs;
    std::vector<size_t> shape_tris;      // triangles per provisional shape
    std::vector<char> shape_kept;
    shape_tris.push_back(0);
    shape_kept.push_back(0);
    bool group_open = false;
    int material = -1;
    std::vector<size_t> vbase(n_pieces + 1, 0), vnbase(n_pieces + 1, 0), vtbase(n_pieces + 1, 0);
    for (size_t k = 0; k < n_pieces; ++k) {
        const Piece& pc = pieces[k];
        vbase[k + 1] = vbase[k] + pc.v.size() / 3;
        vnbase[k + 1] = vnbase[k] + pc.vn.size() / 3;
        vtbase[k + 1] = vtbase[k] + pc.vt.size() / 2;
        size_t at = 0;
        auto close_run = [&](size_t upto) {
            if (upto > at) {
                runs.push_back(Run{k, at, upto, material, shape_tris.size() - 1, shape_tris.back()});
                shape_tris.back() += upto - at;
                group_open = true;
                at = upto;
            }
        };
        for (const Event& e : pc.ev) {
            close_run(e.tri_pos);
            if (e.kind == kEvShortFace) {
                group_open = true;
            } else if (e.kind == kEvUsemtl) {
                int id = -1;
                auto it = mtl_index.find(e.name);
                if (it != mtl_index.end()) id = it->second;
                if (id != material) { group_open = false; material = id; }
            } else if (e.kind == kEvMtllib) {
                if (!load_mtl(matpath + e.name, &mtls, &mtl_index)) return fail_ctx(ctx, PT_EIO, "cannot open MTL file: " + matpath + e.name);
            } else {      // g / o
                shape_kept.back() = group_open ? 1 : 0;
                shape_tris.push_back(0);
                shape_kept.push_back(0);
                group_open = false;
            }
        }
        close_run(pc.tris.size());
    }
    shape_kept.back() = (group_open || shape_tris.back() != 0) ? 1 : 0;     // end of file: tiny_obj_loader.h flushes the pending group

    // C: vertices in file order, triangles into their shapes
    std::vector<float> v(vbase[n_pieces] * 3), vn(vnbase[n_pieces] * 3), vt(vtbase[n_pieces] * 2);
    std::vector<Shape> shapes;
    std::vector<size_t> shape_slot(shape_tris.size(), (size_t)-1);
    for (size_t sidx = 0; sidx < shape_tris.size(); ++sidx)
        if (shape_kept[sidx]) {
            shape_slot[sidx] = shapes.size();
            shapes.emplace_back();
            shapes.back().faces.resize(shape_tris[sidx]);
        }
    parallel_ranges(n_pieces, 1, [&](size_t b, size_t e) {
        for (size_t k = b; k < e; ++k)
            if (!pieces[k].v.empty()) std::memcpy(&v[vbase[k] * 3], pieces[k].v.data(), sizeof(float) * pieces[k].v.size());
        for (size_t k = b; k < e; ++k)
            if (!pieces[k].vn.empty()) std::memcpy(&vn[vnbase[k] * 3], pieces[k].vn.data(), sizeof(float) * pieces[k].vn.size());
        for (size_t k = b; k < e; ++k)
            if (!pieces[k].vt.empty()) std::memcpy(&vt[vtbase[k] * 2], pieces[k].vt.data(), sizeof(float) * pieces[k].vt.size());
    });
    parallel_ranges(runs.size(), 1, [&](size_t b, size_t e) {
        for (size_t r = b; r < e; ++r) {
            const Run& run = runs[r];
            if (shape_slot[run.shape] == (size_t)-1) continue;
            Face3* out = shapes[shape_slot[run.shape]].faces.data() + run.dst;
            const Piece& pc = pieces[run.piece];
            const int vb = (int)vbase[run.piece];
            for (size_t i = run.tri_begin; i < run.tri_end; ++i, ++out) {
                const RawTri& rt = pc.tris[i];
                for (int c = 0; c < 3; ++c) out->v[c] = fix_index(rt.idx[c], vb + rt.nv_local);
                for (int c = 0; c < 3; ++c) out->vn[c] = rt.vn[c] == kNoVn || rt.vn[c] == 0 ? -1 : fix_index(rt.vn[c], (int)vnbase[run.piece] + rt.nvn_local);
                for (int c = 0; c < 3; ++c) out->vt[c] = rt.vt[c] == kNoVn || rt.vt[c] == 0 ? -1 : fix_index(rt.vt[c], (int)vtbase[run.piece] + rt.nvt_local);
                out->mat = run.material;
            }
        }
    });
    pieces.clear();
    clk.lap("parse");

    // ---- materials, main.cpp:562-581
    int base = -1;                                   // mat_offset, main.cpp:562
    std::map<std::string, int> maps;                 // map_Kd files of this call: texture index, or -1 for one that cannot be used
    ctx->obj_textures_loaded = ctx->obj_textures_skipped = 0;
    for (size_t i = 0; i < mtls.size(); ++i) {
        const MtlRec& m = mtls[i];
        auto kn = m.unknown.find("Kn"), kk = m.unknown.find("Kk"), tp = m.unknown.find("Tp");
        if (kn == m.unknown.end() || kk == m.unknown.end() || tp == m.unknown.end())
            return fail_ctx(ctx, PT_EIO, "material '" + m.name + "' lacks Kn/Kk/Tp (the reference's .at() would throw, main.cpp:568-571)");
        float N[3], K[3];
        if (!str_to_float3(kn->second, N) || !str_to_float3(kk->second, K))
            return fail_ctx(ctx, PT_EIO, "material '" + m.name + "': Kn/Kk need three blank-separated numbers");
        pt_material pm;
        pt_material_init(&pm, m.diffuse, m.specular, m.emission, N, K, m.shininess, (int32_t)std::atoi(tp->second.c_str()));
        int idx = pt_add_material(ctx, &pm);
        if (idx < 0) return idx;
        if (base < 0) base = idx;
        ctx->obj_textures_skipped += m.map_kd_skipped;
        if (!m.map_kd.empty()) {
            auto it = maps.find(m.map_kd);
            if (it == maps.end()) it = maps.insert(std::make_pair(m.map_kd, load_albedo_map(ctx, matpath + m.map_kd))).first;
            if (it->second >= 0 && pt_set_material_texture(ctx, idx, it->second) == PT_OK) ++ctx->obj_textures_loaded;
            else ++ctx->obj_textures_skipped;
        }
    }
    if (base < 0) base = 0;

    // ---- vertices, main.cpp:598-606: negate x, rotate_x(pitch), rotate_y(yaw), scale, translate -- once per VERTEX of
    // the file (the reference redoes it for every corner of every face, with the same arithmetic and so the same bits)
    const size_t nvert = v.size() / 3;
    std::vector<float> w(v.size());
    parallel_ranges(nvert, 1 << 14, [&](size_t b, size_t e) {
        for (size_t i = b; i < e; ++i) {
            float q[3] = {-v[3 * i + 0], v[3 * i + 1], v[3 * i + 2]};       // main.cpp:598
            rot_x(q, pitch);                                                // main.cpp:602-603
            rot_y(q, yaw);
            for (int a = 0; a < 3; ++a) w[3 * i + a] = q[a] * scale[a] + pos[a];   // main.cpp:604-606
        }
    });

    // ---- normals: the inverse transpose of that linear map -- negate x, rotate_x(pitch), rotate_y(yaw), divide by scale -- in double
    const size_t nnorm = vn.size() / 3;
    std::vector<float> wn(vn.size());
    {
        const double gx = (double)(pitch / 180.0f * 3.141593f), gy = (double)(yaw / 180.0f * 3.141593f);      // the angles rot_x / rot_y use
        const double cx = std::cos(gx), sx = std::sin(gx), cy = std::cos(gy), sy = std::sin(gy);
        for (size_t i = 0; i < nnorm; ++i) {
            const double x0 = -(double)vn[3 * i], y0 = vn[3 * i + 1], z0 = vn[3 * i + 2];
            const double y1 = y0 * cx - z0 * sx, z1 = y0 * sx + z0 * cx;
            const double q[3] = {(x0 * cy + z1 * sy) / (double)scale[0], y1 / (double)scale[1], (-x0 * sy + z1 * cy) / (double)scale[2]};
            const double l = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
            for (int a = 0; a < 3; ++a) wn[3 * i + a] = l > 0.0 && std::isfinite(l) ? (float)(q[a] / l) : 0.0f;
        }
    }
    clk.lap("transform vertices");
    // ---- shapes, main.cpp:587-616: one add_Triangle per face, one end_Obj per shape
    for (const Shape& sh : shapes) {
        if (sh.faces.empty()) return fail_ctx(ctx, PT_EIO, "OBJ shape without faces (the reference would call end_Obj on an empty object)");
        const size_t nf = sh.faces.size();
        int bad = 0;       // 1: face without material, 2: vertex out of range
        for (size_t i = 0; i < nf && !bad; ++i) {
            const Face3& f = sh.faces[i];
            if (f.mat < 0) bad = 1;
            for (int k = 0; k < 3 && !bad; ++k)
                if (f.v[k] < 0 || (size_t)f.v[k] >= nvert) bad = 2;
        }
        if (bad == 1) return fail_ctx(ctx, PT_EIO, "OBJ face without a known usemtl material (the reference would index materials[-1])");
        if (bad == 2) return fail_ctx(ctx, PT_EIO, "OBJ face references a vertex that does not exist");
        pt_triangle* tris = nullptr;                 // the records are built in place at the end of the scene's triangle list
        int rc = ptamd::append_triangles(ctx, (int64_t)nf, &tris);
        if (rc != PT_OK) return rc;
        parallel_ranges(nf, 1 << 14, [&](size_t b, size_t e) {
            for (size_t i = b; i < e; ++i) {
                const Face3& f = sh.faces[i];
                pt_triangle_init(&tris[i], &w[3 * (size_t)f.v[0]], &w[3 * (size_t)f.v[1]], &w[3 * (size_t)f.v[2]], (uint16_t)(base + f.mat));
            }
        });
        clk.lap("triangle records (add_Triangle)");
        bool any_vn = false;
        for (size_t i = 0; i < nf && !any_vn; ++i) any_vn = sh.faces[i].vn[0] >= 0;
        if (any_vn) {
            int64_t ntris = 0;
            pt_debug_scene_sizes(ctx, &ntris, nullptr, nullptr);
            std::vector<float> fn(nf * 9, 0.0f);
            for (size_t i = 0; i < nf; ++i) {
                const Face3& f = sh.faces[i];
                bool all = true;
                for (int k = 0; k < 3; ++k) all = all && f.vn[k] >= 0 && (size_t)f.vn[k] < nnorm;
                if (!all) continue;
                for (int k = 0; k < 3; ++k) std::memcpy(&fn[i * 9 + 3 * (size_t)k], &wn[3 * (size_t)f.vn[k]], sizeof(float) * 3);
            }
            rc = pt_set_vertex_normals(ctx, ntris - (int64_t)nf, (int64_t)nf, fn.data());
            if (rc != PT_OK) return rc;
        }
        bool any_vt = false;
        for (size_t i = 0; i < nf && !any_vt; ++i) any_vt = sh.faces[i].vt[0] >= 0;
        if (any_vt) {
            int64_t ntris = 0;
            pt_debug_scene_sizes(ctx, &ntris, nullptr, nullptr);
            const size_t nuv = vt.size() / 2;
            std::vector<float> fu(nf * 6, std::numeric_limits<float>::quiet_NaN());      // (NaN: the triangle has no uvs)
            for (size_t i = 0; i < nf; ++i) {
                const Face3& f = sh.faces[i];
                bool all = true;
                for (int k = 0; k < 3; ++k) all = all && f.vt[k] >= 0 && (size_t)f.vt[k] < nuv;
                if (!all) continue;
                for (int k = 0; k < 3; ++k) std::memcpy(&fu[i * 6 + 2 * (size_t)k], &vt[2 * (size_t)f.vt[k]], sizeof(float) * 2);
            }
            rc = pt_set_vertex_uvs(ctx, ntris - (int64_t)nf, (int64_t)nf, fu.data());
            if (rc != PT_OK) return rc;
        }
        rc = pt_end_obj(ctx);
        if (rc != PT_OK) return rc;
        clk.lap("pt_end_obj");
    }
    return PT_OK;
}
