"""Helpers of tests/test_obj_pieces_host.py: the OBJ fixtures under tests/golden/obj, what the reference parser's dump of a fixture
says pt_add_obj has to produce, and padded copies of a fixture that force the multi-piece parse.

pt_add_obj cuts a file into min(4 * min(cores, 16), bytes >> 16) pieces at line ends and parses them in parallel
(opencl_path_tracer_amd/csrc/pt_obj.cpp).  A `#` line means nothing to either parser, so a fixture with blocks of comment lines between
two of its lines must load exactly like the bare fixture, which the dump ties to the reference parser."""
import collections
import json
import os
import re

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "obj")
TRANSFORMS = [((0, 0, 0), (1, 1, 1), 0.0, 0.0), ((50, 330, -150), (190, 190, 190), -90.0, 50.0)]
EOLS = {"lf": b"\n", "crlf": b"\r\n", "cr": b"\r"}
PAD_SINGLE = 256 << 10          # bytes of padding in a gap: at least four pieces of at least 64 KiB, every cut inside the padding
PAD_EVEN = 96 << 10


def fixture(name):
    return os.path.join(GOLDEN, name + ".obj")


def dump_of(name):
    """The dump; a float the harness printed as `-0` keeps its sign (json alone would read the integer 0)."""
    with open(os.path.join(GOLDEN, name + ".tinyobj.json")) as f:
        return json.load(f, parse_int=lambda s: -0.0 if s == "-0" else int(s))


# ---------------------------------------------------------------------------- what the dump says
def expected_scene(oracle, dump, pos, scale, pitch, yaw, mat_offset=0):
    """(triangles, materials, object starts) by Scene::add_Obj's own steps (main.cpp:562-616) with the oracle's constructors."""
    mats = []
    for m in dump["materials"]:                                   # main.cpp:564-572
        def f3(s):
            parts = s.split(" ")
            return [np.float32(float(parts[i])) if parts[i] else np.float32(0) for i in range(3)]
        kn, kk, tp = m["unknown"]["Kn"], m["unknown"]["Kk"], int(m["unknown"]["Tp"])
        mats.append(oracle.make_material(m["diffuse"], m["specular"], m["emission"], f3(kn), f3(kk), m["shininess"], tp)[0])
    V = np.array(dump["vertices"], dtype=np.float32).reshape(-1, 3)
    W = [oracle.obj_vertex(v, pos, scale, pitch, yaw) for v in V]
    tris, obj_begin = [], []
    for sh in dump["shapes"]:                                     # main.cpp:587-616
        obj_begin.append(len(tris))
        assert set(sh["num_face_vertices"]) <= {3}
        for f in range(len(sh["num_face_vertices"])):
            a, b, c = sh["vertex_index"][3 * f:3 * f + 3]
            tris.append(oracle.make_triangle(W[a], W[b], W[c], mat_offset + sh["material_ids"][f])[0])
    return np.array(tris), np.array(mats), obj_begin


def normal_map(scale, pitch, yaw):
    """The inverse transpose of the positions' linear map (negate x, rotate_x(pitch), rotate_y(yaw), scale), in float64 -- the map
    pt_obj.cpp documents for vn, written as tests/test_smooth_host.py writes it."""
    g = float(np.float32(pitch) / np.float32(180.0) * np.float32(3.141593))
    b = float(np.float32(yaw) / np.float32(180.0) * np.float32(3.141593))
    F = np.diag([-1.0, 1.0, 1.0])
    Rx = np.array([[1, 0, 0], [0, np.cos(g), -np.sin(g)], [0, np.sin(g), np.cos(g)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    M = np.diag(np.asarray(scale, dtype=np.float64)) @ Ry @ Rx @ F
    return np.linalg.inv(M).T


def expected_attributes(dump, scale, pitch, yaw):
    """Per triangle of the dump, in order: (normals (n, 3, 3) float64, has_normals, uvs (n, 3, 2) float32, has_uvs).  Only a triangle
    whose three corners carry an index has the attribute (-1 is the reference's "no index")."""
    N = np.array(dump["normals"], dtype=np.float32).reshape(-1, 3).astype(np.float64)
    T = np.array(dump["texcoords"], dtype=np.float32).reshape(-1, 2)
    A = normal_map(scale, pitch, yaw)
    nrm, nhas, uvs, uhas = [], [], [], []
    for sh in dump["shapes"]:
        for f in range(len(sh["num_face_vertices"])):
            ni, ti = sh["normal_index"][3 * f:3 * f + 3], sh["texcoord_index"][3 * f:3 * f + 3]
            nhas.append(min(ni) >= 0)
            uhas.append(min(ti) >= 0)
            assert max(ni) < len(N) and max(ti) < len(T)
            n = (A @ N[ni].T).T if nhas[-1] else np.zeros((3, 3))
            nrm.append(n / np.linalg.norm(n, axis=1, keepdims=True) if nhas[-1] else n)
            uvs.append(T[ti] if uhas[-1] else np.zeros((3, 2), dtype=np.float32))
    return np.array(nrm).reshape(-1, 3, 3), np.array(nhas, dtype=bool), np.array(uvs, dtype=np.float32).reshape(-1, 3, 2), np.array(uhas, dtype=bool)


# ---------------------------------------------------------------------------- what pt_add_obj made
Loaded = collections.namedtuple("Loaded", "tris mats objs normals has_normals uvs has_uvs textures_loaded textures_skipped pieces")


def load(api, path, xf=TRANSFORMS[1]):
    """Everything a load leaves on a host-only context; `pieces` is not part of what two loads are compared by (same_load)."""
    sc = api.Scene(16, 16, device=None)
    sc.add_Obj(path, *xf)
    tris, mats, objs = sc.debug_scene()
    n, nh = sc.debug_vertex_normals()
    uv, uh = sc.debug_vertex_uvs()
    return Loaded(tris.tobytes(), mats.tobytes(), objs.tolist(), n.tobytes(), nh.tolist(), uv.tobytes(), uh.tolist(),
                  int(sc.stat("obj_textures_loaded")), int(sc.stat("obj_textures_skipped")), int(sc.stat("obj_pieces")))


def same_load(a, b):
    """The first field in which two loads differ (None: byte for byte the same scene)."""
    for name in Loaded._fields[:-1]:
        if getattr(a, name) != getattr(b, name):
            return name
    return None


def load_error(api, path, xf=TRANSFORMS[1]):
    """(code, message) of a load that has to fail."""
    sc = api.Scene(16, 16, device=None)
    try:
        sc.add_Obj(path, *xf)
    except api.PtError as e:
        return e.code, str(e)
    raise AssertionError("pt_add_obj accepted " + path)


# ---------------------------------------------------------------------------- padded copies
def units(data):
    """The file in units that each end with a meaningful line (not blank, not a comment) and its terminator; blank and comment lines
    travel with the meaningful line after them, those at the end of the file with the last one.  b"".join(units(d)) == d."""
    lines = re.findall(rb"[^\r\n]*(?:\r\n|\r|\n)|[^\r\n]+$", data)
    assert b"".join(lines) == data
    out, cur = [], b""
    for ln in lines:
        cur += ln
        body = ln.strip(b" \t\r\n")
        if body and not body.startswith(b"#"):
            out.append(cur)
            cur = b""
    if cur:
        out[-1] += cur
    return out


_CYCLE = {}


def padding(nbytes, eol, phase=0):
    """At least nbytes of `#` lines whose lengths cycle through 1..97 bytes (before the terminator), starting `phase` steps into the
    cycle: where a cut at a fixed fraction of the file lands -- a line's start, its middle, the \\r or the \\n -- varies with it."""
    if eol not in _CYCLE:
        _CYCLE[eol] = [b"#" + b"-" * k + eol for k in range(97)]
    c = _CYCLE[eol]
    c = c[phase % 97:] + c[:phase % 97]
    block = b"".join(c)
    return block * (nbytes // len(block)) + b"".join(_take(c, nbytes % len(block)))


def _take(lines, nbytes):
    got = 0
    for ln in lines:
        if got >= nbytes:
            return
        got += len(ln)
        yield ln


def padded(us, gaps, eol=b"\n", phase=0):
    """The units with padding(gaps[g]) between unit g - 1 and unit g, for g in 1..len(us) - 1."""
    out = [us[0]]
    for g in range(1, len(us)):
        if g in gaps:
            assert out[-1].endswith((b"\n", b"\r"))
            out.append(padding(gaps[g], eol, phase + 7 * g))
        out.append(us[g])
    return b"".join(out)


def cut_classes(data, pieces):
    """Where the nominal cuts of pt_add_obj (byte size * k / pieces) land: "start" (first byte of a line), "cr", "lf" (the terminators
    themselves), "crlf_lf" (the \\n of a \\r\\n) or "mid"."""
    out = []
    for k in range(1, pieces):
        p = len(data) * k // pieces
        c, before = data[p:p + 1], data[p - 1:p]
        if c == b"\r":
            out.append("cr")
        elif c == b"\n":
            out.append("crlf_lf" if before == b"\r" else "lf")
        elif before in (b"\n", b"\r"):
            out.append("start")
        else:
            out.append("mid")
    return out
