"""-m "not gpu": pt_add_obj against the reference's parser on fixtures built for its edges, and the same fixtures cut into pieces.

tests/golden/obj/*.tinyobj.json are dumps of the reference's vendored tinyobj v1.0.3 (tests/golden/make_obj_golden.py), now with normals,
texcoords and their per-corner indices.  Part 1 holds every fixture to its dump: triangles, materials and object starts byte for byte
by Scene::add_Obj's steps, vertex normals by pt_obj.cpp's documented inverse-transpose map in float64, uvs bit for bit.  Part 2 pads the
fixtures with comment lines (tests/obj_cases.py) so that pt_add_obj parses them in 4 to 64 pieces with every gap between two meaningful
lines on a piece boundary in turn, and requires the bare fixture's scene; the statistic "obj_pieces" proves the pieces.  Part 3 looks at
the numbers token by token, part 4 at the errors, bare and across pieces.

Part 2 as a whole (single gaps, slid cuts, two gaps, even padding; about 900 loads of 0.25 to 3.5 MiB) was measured at 1.5 s of wall
time and 2.1 s of CPU (user + system, pytest's start included) on eight cores; the whole module takes 2.1 s."""
import os
import random
import shutil

import numpy as np
import pytest

import obj_cases as oc

VALID = ["scene1", "relidx", "shapes", "shapes_noeol", "text_lf", "text_crlf", "text_cr", "mtl", "order", "zeroidx", "numbers"]
TEXT = ["text_lf", "text_crlf", "text_cr"]
# what has to fail, the words of pt_add_obj's message, and what the dump shows of the reference's undefined behaviour at that point
ERRORS = {"err_relidx": "vertex that does not exist", "err_relorder": "vertex that does not exist", "err_pastend": "vertex that does not exist",
          "err_nousemtl": "without a known usemtl", "err_nomtl": "cannot open MTL file", "err_empty": "shape without faces"}


@pytest.fixture()
def workdir(tmp_path):
    """The fixtures' libraries and map next to where the padded copies are written."""
    for f in os.listdir(oc.GOLDEN):
        if f.endswith((".mtl", ".ppm")):
            shutil.copy(os.path.join(oc.GOLDEN, f), str(tmp_path))
    return str(tmp_path)


def write(workdir, name, data):
    path = os.path.join(workdir, name)
    with open(path, "wb") as f:
        f.write(data)
    return path


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------- 1. the fixtures against the reference parser
@pytest.mark.parametrize("xf", oc.TRANSFORMS, ids=["identity", "placed"])
@pytest.mark.parametrize("name", VALID)
def test_fixture_matches_reference_parser(api, oracle, name, xf):
    dump = oc.dump_of(name)
    assert dump["ret"] is True
    got = oc.load(api, oc.fixture(name), xf)
    etris, emats, eobjs = oc.expected_scene(oracle, dump, *xf)
    assert got.objs == eobjs
    assert got.mats == emats.astype(api.MATERIAL).tobytes()
    assert len(got.tris) == len(etris) * api.TRIANGLE.itemsize
    assert got.tris == etris.astype(api.TRIANGLE).tobytes()
    assert got.pieces == 1                      # a file under 128 KiB is one piece


@pytest.mark.parametrize("xf", oc.TRANSFORMS, ids=["identity", "placed"])
@pytest.mark.parametrize("name", [n for n in VALID if n != "zeroidx"])
def test_fixture_normals_and_uvs_match_the_dump(api, name, xf):
    """Normals: within 1e-6 of the float64 map (the bound of tests/test_smooth_host.py for the same map); uvs: copied, so the same bits;
    a triangle has either only if all three of its corners carry the index."""
    dump = oc.dump_of(name)
    got = oc.load(api, oc.fixture(name), xf)
    n, nhas, uv, uhas = oc.expected_attributes(dump, xf[1], xf[2], xf[3])
    assert got.has_normals == nhas.tolist() and got.has_uvs == uhas.tolist()
    gn = np.frombuffer(got.normals, np.float32).reshape(-1, 3, 3)
    guv = np.frombuffer(got.uvs, np.float32).reshape(-1, 3, 2)
    if len(gn):
        assert np.abs(gn.astype(np.float64) - n).max() <= 1e-6
        assert not gn[~nhas].any() and not guv[~uhas].any()
    assert np.array_equal(bits(guv), bits(uv))
    if name in ("relidx", "mtl", "order") + tuple(TEXT):
        assert nhas.any() or name == "mtl"
        assert uhas.any() and not uhas.all()


def test_index_zero_means_absent_for_vt_and_vn(api):
    """The one place the reader leaves the reference on purpose: the reference's fixIndex maps a 0 to the FIRST element
    (tiny_obj_loader.h:410-414; the dump shows index 0); pt_add_obj reads a 0 in a vt or vn position as "no index", so that face
    carries no uvs / no normals.  The triangles themselves are the reference's (test_fixture_matches_reference_parser)."""
    dump = oc.dump_of("zeroidx")
    sh = dump["shapes"][0]
    assert sh["texcoord_index"] == [0, 0, 0, 0, 1, 2, 0, 2, 1] and sh["normal_index"] == [0] * 9
    got = oc.load(api, oc.fixture("zeroidx"))
    assert got.has_uvs == [False, True, True] and got.has_normals == [True, False, True]
    n, nhas, uv, uhas = oc.expected_attributes(dump, *oc.TRANSFORMS[1][1:])
    guv = np.frombuffer(got.uvs, np.float32).reshape(-1, 3, 2)
    assert np.array_equal(bits(guv[1:]), bits(uv[1:])) and not guv[0].any()


def test_the_three_line_endings_are_one_file(api):
    dumps = [oc.dump_of(n) for n in TEXT]
    assert dumps[0] == dumps[1] == dumps[2] and len(dumps[0]["shapes"]) == 2
    loads = [oc.load(api, oc.fixture(n)) for n in TEXT]
    assert oc.same_load(loads[0], loads[1]) is None and oc.same_load(loads[0], loads[2]) is None


def test_mtl_fixture_maps(api):
    """mtl.obj: `first` names a map that loads, the first `dup` one with an option token, `late` a file that does not exist."""
    got = oc.load(api, oc.fixture("mtl"))
    assert (got.textures_loaded, got.textures_skipped) == (1, 2)


def test_fixtures_hold_what_they_are_for():
    """The dumps show the cases the fixtures were written for (a fixture edited into something tamer fails here)."""
    sh = oc.dump_of("shapes")
    assert [s["name"] for s in sh["shapes"]] == ["", "", "dropped_tail", "last"]                      # obj_b is dropped at `g dropped_tail`
    assert [len(s["material_ids"]) for s in sh["shapes"]] == [2, 1, 3, 3]
    assert oc.dump_of("shapes_noeol")["shapes"][-1]["vertex_index"][-9:] == [0, 1, 2, 0, 2, 3, 0, 3, 4]   # the last line has no terminator
    rel = oc.dump_of("relidx")
    assert sum(len(s["material_ids"]) for s in rel["shapes"]) == 1 + 2 + 2 + 2 + 1 + 3 + 2 + 5 + 1 + 2
    m = oc.dump_of("mtl")
    assert [x["name"] for x in m["materials"]] == ["first", "dup", "tabbed", "dup", "late", "second_only"]
    assert m["shapes"][0]["material_ids"] == [0, 1, 2, 4, 1, 5, 0]                                     # `dup` stays the first library's
    assert m["materials"][2]["unknown"]["Kn"] == "0.5 0.25 0.125" and m["materials"][5]["shininess"] == 1
    for name in VALID:
        with open(oc.fixture(name), "rb") as f:
            assert len(oc.units(f.read())) < (64 if name != "numbers" else 512), name


# ---------------------------------------------------------------------------- 2. every piece boundary
def single_gap_sweep(api, workdir, name, eols):
    with open(oc.fixture(name), "rb") as f:
        us = oc.units(f.read())
    bare = oc.load(api, write(workdir, "bare.obj", b"".join(us)))
    assert bare.pieces == 1
    for g in range(1, len(us)):
        data = oc.padded(us, {g: oc.PAD_SINGLE}, eols[g % len(eols)])
        got = oc.load(api, write(workdir, "padded.obj", data))
        assert 4 <= got.pieces <= 64, (name, g, got.pieces)
        assert oc.same_load(bare, got) is None, (name, g, oc.same_load(bare, got))
    return len(us) - 1


@pytest.mark.parametrize("name", ["scene1", "relidx", "shapes", "shapes_noeol", "mtl", "order"])
def test_single_gap_padding(api, workdir, name):
    """At least 256 KiB of comments in ONE gap: piece 0 ends after line g, the last piece starts at line g + 1, the pieces between hold
    comments only.  Every gap of the fixture; the padding's line ends go through \\n, \\r\\n and \\r with g."""
    assert single_gap_sweep(api, workdir, name, [b"\n", b"\r\n", b"\r"]) >= 10


@pytest.mark.parametrize("pad", sorted(oc.EOLS))
@pytest.mark.parametrize("name", TEXT)
def test_single_gap_padding_text(api, workdir, name, pad):
    """The content in each line-ending style, padded in each style, independently."""
    assert single_gap_sweep(api, workdir, name, [oc.EOLS[pad]]) >= 10


@pytest.mark.parametrize("pad", ["crlf", "cr", "lf"])
def test_cut_slides_over_a_line_end(api, workdir, pad):
    """One gap of text_crlf, the padding grown four bytes at a time: the first of the four pieces' cuts moves one byte at a time over
    more than a whole padding line, so it lands on a line's first byte, inside it, on its \\r and on the \\n of its \\r\\n."""
    with open(oc.fixture("text_crlf"), "rb") as f:
        us = oc.units(f.read())
    bare = oc.load(api, write(workdir, "bare.obj", b"".join(us)))
    g, eol, seen = 9, oc.EOLS[pad], set()
    base = oc.padding(oc.PAD_SINGLE, eol)
    step = b"#" + b"-" * (3 - len(eol)) + eol
    for j in range(104):
        data = b"".join(us[:g]) + base + step * j + b"".join(us[g:])
        got = oc.load(api, write(workdir, "padded.obj", data))
        assert got.pieces == 4 and oc.same_load(bare, got) is None, (j, oc.same_load(bare, got))
        seen.add(oc.cut_classes(data, 4)[0])
    assert seen == {"start", "mid"} | {"crlf": {"cr", "crlf_lf"}, "cr": {"cr"}, "lf": {"lf"}}[pad]


def gap_pairs(us, count, seed):
    """`count` pairs g1 < g2, seeded; first those whose middle stretch changes state (usemtl, mtllib, g, o, a short face) without
    a triangle, up to a third of the sample."""
    def kind(u):
        body = [ln.strip() for ln in u.replace(b"\r", b"\n").split(b"\n")]
        body = [ln for ln in body if ln and not ln.startswith(b"#")][-1].split()
        if body[0] == b"f":
            return "tri" if len(body) > 3 else "event"
        return "event" if body[0] in (b"usemtl", b"mtllib", b"g", b"o") else "data"
    kinds = [kind(u) for u in us]
    pairs = [(a, b) for a in range(1, len(us)) for b in range(a + 1, len(us))]
    quiet = [p for p in pairs if "tri" not in kinds[p[0]:p[1]] and "event" in kinds[p[0]:p[1]]]
    rng = random.Random(seed)
    rng.shuffle(quiet)
    rng.shuffle(pairs)
    out = quiet[:count // 3]
    out += [p for p in pairs if p not in out][:count - len(out)]
    return out, len(quiet[:count // 3])


@pytest.mark.parametrize("name", ["scene1", "relidx", "shapes", "shapes_noeol", "mtl", "text_crlf"])
def test_two_gap_padding(api, workdir, name):
    """At least 256 KiB in each of two gaps: the parser's state crosses three stretches of content in different pieces (or four:
    with equal padding the middle cut can fall inside the middle stretch)."""
    with open(oc.fixture(name), "rb") as f:
        us = oc.units(f.read())
    bare = oc.load(api, write(workdir, "bare.obj", b"".join(us)))
    pairs, quiet = gap_pairs(us, 30, 1234)
    assert len(pairs) == 30 and quiet >= 3
    for k, (g1, g2) in enumerate(pairs):
        eol = [b"\n", b"\r\n", b"\r"][k % 3]
        got = oc.load(api, write(workdir, "padded.obj", oc.padded(us, {g1: oc.PAD_SINGLE, g2: oc.PAD_SINGLE}, eol, phase=k)))
        assert 4 <= got.pieces <= 64
        assert oc.same_load(bare, got) is None, (name, g1, g2, oc.same_load(bare, got))


@pytest.mark.parametrize("name", ["scene1", "relidx"])
def test_even_padding(api, workdir, name):
    """96 KiB in every gap: several MiB, as many pieces as the host's cores allow (64 from 16 cores)."""
    with open(oc.fixture(name), "rb") as f:
        us = oc.units(f.read())
    bare = oc.load(api, write(workdir, "bare.obj", b"".join(us)))
    data = oc.padded(us, {g: oc.PAD_EVEN for g in range(1, len(us))}, b"\r\n" if name == "relidx" else b"\n")
    assert len(data) > (2 << 20)
    got = oc.load(api, write(workdir, "padded.obj", data))
    assert 4 < got.pieces <= 64
    assert oc.same_load(bare, got) is None, oc.same_load(bare, got)


# ---------------------------------------------------------------------------- 3. the grammar of numbers
def numbers_tokens():
    toks = []
    with open(oc.fixture("numbers")) as f:
        for ln in f:
            if ln.startswith("v "):
                toks += ln.split()[1:4]
    return toks


def test_number_tokens_give_the_reference_bits(api):
    """Every coordinate of numbers.obj against the dump, bit for bit (identity transform: x is negated and nothing else happens), and
    the materials' float fields.  Well-formed tokens: strtod rounds correctly, the reference accumulates digits in double; both are
    then cast to float -- measured here: no token of the fixture differs.  Odd tokens (`.5`, `1e`, `nan`, `0x10` ...): the reference's
    grammar wants sign, digits, optional fraction, optional non-empty exponent and otherwise gives 0 (tiny_obj_loader.h:437-443)."""
    dump = oc.dump_of("numbers")
    sc = api.Scene(16, 16, device=None)
    sc.add_Obj(oc.fixture("numbers"), *oc.TRANSFORMS[0])
    tris, mats, _ = sc.debug_scene()
    got = np.stack([tris["r1"][:, :3], tris["r2"][:, :3], tris["r3"][:, :3]], axis=1).reshape(-1)
    want = np.array(dump["vertices"], dtype=np.float32).reshape(-1, 3) * np.array([-1, 1, 1], dtype=np.float32) + np.float32(0)
    toks = numbers_tokens()
    assert len(toks) == got.size == want.size and got.size > 900
    wrong = [(toks[i], float(got[i]), float(want.reshape(-1)[i])) for i in np.nonzero(bits(got) != bits(want.reshape(-1)))[0]]
    print("number tokens that differ from the reference:", len(wrong), wrong)
    assert wrong == []
    assert np.isfinite(got).all()
    by_token = dict(zip(toks, np.abs(want.reshape(-1)).tolist()))
    for t in (".5", "-.5", "1e", "1e+", "nan", "inf", "0x10", "+.5", "1.5e", "1ex", "infinity", "-0x10"):
        assert by_token[t] == 0.0, t                                # what the issue read from the reference's source, now seen in its dump
    assert by_token["1.5.3"] == 1.5 and by_token["12abc"] == 12.0 and by_token["2.e3"] == 2000.0 and by_token["1e5x"] == 100000.0
    for i, m in enumerate(dump["materials"]):
        for key, field in (("diffuse", "kd"), ("specular", "ks"), ("emission", "emission")):
            assert np.array_equal(bits(mats[field][i, :3]), bits(np.array(m[key], dtype=np.float32))), (m["name"], key)
        assert bits(mats["shininess"][i]) == bits(np.float32(m["shininess"])), m["name"]
    assert dump["materials"][1]["diffuse"] == [0, 0, 0] and dump["materials"][1]["specular"] == [0, 0, 12] and dump["materials"][1]["shininess"] == 0


# ---------------------------------------------------------------------------- 4. errors, bare and across pieces
def reference_is_undefined(name, dump):
    nv = len(dump["vertices"]) // 3
    if ERRORS[name] == "vertex that does not exist":
        return any(i < 0 or i >= nv for s in dump["shapes"] for i in s["vertex_index"])
    if ERRORS[name] == "without a known usemtl":
        return any(i < 0 for s in dump["shapes"] for i in s["material_ids"])
    if ERRORS[name] == "shape without faces":
        return any(not s["material_ids"] for s in dump["shapes"])
    return "not found" in dump["err"] and any("Kn" not in m["unknown"] for m in dump["materials"])      # a default material stands in


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_errors_across_pieces(api, workdir, name):
    """What the reference answers with undefined behaviour (the dump shows the index, the material id -1, the empty shape, the
    stand-in material) is PT_EIO with one message, wherever the pieces are cut."""
    assert reference_is_undefined(name, oc.dump_of(name))
    with open(oc.fixture(name), "rb") as f:
        us = oc.units(f.read())
    code, msg = oc.load_error(api, write(workdir, "e.obj", b"".join(us)))
    assert code == api.PT_EIO and ERRORS[name] in msg
    for g in range(1, len(us)):
        sc_code, sc_msg = oc.load_error(api, write(workdir, "e.obj", oc.padded(us, {g: oc.PAD_SINGLE}, [b"\n", b"\r\n", b"\r"][g % 3])))
        assert (sc_code, sc_msg) == (code, msg), (name, g)


def test_positive_indices_may_name_later_elements(api):
    """order.obj names v / vt / vn in front of their lines by positive index: legal for the reference as the elements exist at the
    end of the file (its dump holds plain indices), and loaded like any other file (test_fixture_matches_reference_parser); the same
    idea with relative indices counts the elements read so far and is err_relorder.obj."""
    d = oc.dump_of("order")
    assert d["shapes"][0]["vertex_index"] == [0, 1, 2, 0, 2, 3, 4, 0, 1] and d["shapes"][0]["normal_index"] == [0, 0, 0, -1, -1, -1, 1, 0, 0]
    assert min(oc.dump_of("err_relorder")["shapes"][0]["vertex_index"]) < 0
