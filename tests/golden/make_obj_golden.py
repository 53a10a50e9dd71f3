"""Regenerates tests/golden/obj/*.tinyobj.json by running the reference's own vendored parser
(/root/reference/tiny_obj_loader.h, compiled into oracle/_ref/tinyobj_dump by oracle/Makefile)
on the synthetic OBJ/MTL files next to them.  Only possible in the build container.

numbers.obj is written here first (seeded, so the same every time): a few hundred `v` lines in the forms exporters
write, then a short block of tokens outside the reference's number grammar (tiny_obj_loader.h:437-443)."""
import glob
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

ODD_V = [".5 -.5 1e", "1e+ nan inf", "0x10 1.5.3 12abc", "+.5 - +", "1.5e 1ex 2.e3", "-0x10 1e5x infinity", "1e-x -nan 1.e", "7 .e1 e1"]


def numbers_obj():
    rng = np.random.default_rng(20240607)
    forms = ["%.6f", "%.4f", "%g", "%r", "%s", "%.9g", "%e", "%.12f", "%.8f", "%.3f"]
    toks = []
    for k in range(864):
        x = np.float32(rng.standard_normal() * 10.0 ** rng.integers(-4, 5))
        f = forms[k % len(forms)]
        toks.append(repr(float(x)) if f == "%r" else str(x) if f == "%s" else f % float(x))       # %r: the float32 as Python prints the double
    toks += ["1e-3", "1E+2", "-0", "5.", "+1.5", "0", "7", "-12", "1000000", "0.123456789012", "3.14159265358979", "-0.000001",
             "1.e5", "2.5E-7", "1e10", "-1E-10", "16777217", "0.1", "0.30000001192092896", "123456.789", "+0", "00012.50", "9.999999e9", "1e0"]
    assert len(toks) % 3 == 0
    lines = ["mtllib numbers.mtl", "# number forms (written by tests/golden/make_obj_golden.py; own data)", "usemtl plain"]
    nv = 0
    for k in range(0, len(toks), 3):
        lines.append("v " + " ".join(toks[k:k + 3]))
        nv += 1
    lines.append("# tokens outside the reference's grammar")
    for t in ODD_V:
        lines.append("v " + t)
        nv += 1
    while nv % 3:
        lines.append("v 1 2 3")
        nv += 1
    lines.append("usemtl odd")
    for k in range(0, nv, 3):
        lines.append("f %d %d %d" % (k + 1, k + 2, k + 3))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    with open(os.path.join(HERE, "obj", "numbers.obj"), "w") as f:
        f.write(numbers_obj())
    exe = os.path.join(ROOT, "oracle", "_ref", "tinyobj_dump")
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "-s"], check=True)
    for obj in sorted(glob.glob(os.path.join(HERE, "obj", "*.obj"))):
        # (by its name alone, from its own directory: a warning in the dump then names no directory of the machine it was made on)
        out = subprocess.run([exe, os.path.basename(obj)], check=True, capture_output=True, text=True, cwd=os.path.join(HERE, "obj")).stdout
        open(obj[:-4] + ".tinyobj.json", "w").write(out)
        print("wrote", obj[:-4] + ".tinyobj.json")
