"""Ownership of a context's device arrays (csrc/pt_devbuf.hpp), checked on the CPU: tests/cpp/devbuf_test.cpp drives DevBuf with a
counting allocator through every sequence of up to four operations and every position of one failing allocation or free, under
AddressSanitizer and UBSan.  A plain executable: built here, run as a child process."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devbuf_ownership_sequences(tmp_path):
    exe = tmp_path / "devbuf_test"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "opencl_path_tracer_amd", "csrc"), "-o", str(exe),
                    os.path.join(ROOT, "tests", "cpp", "devbuf_test.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.startswith("devbuf_test: ok"), r.stdout[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
