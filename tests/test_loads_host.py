"""The wall loads' boundary-face list builder (navierstokessolver_amd/csrc/ns_loads_host.h) on the host:
tests/loads_host_test.cpp drives it -- the (edge, s) order, the CSR offsets, chunks of 256 that never span two edges,
one-face edges, a cell with two boundary faces, an edge without faces, a bad edge index -- as a stand-alone program
under the sanitizers.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "navierstokessolver_amd", "csrc")


def test_face_list_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "loads_host_test")
    # (the sanitizer runtimes linked statically, as tests/test_timing_host.py does)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "loads_host_test.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
