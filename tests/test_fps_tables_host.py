"""The direct Poisson solve's host tables (navierstokessolver_amd/csrc/ns_fps_tables.h) without a GPU:
tests/fps_tables_host_test.cpp builds them for the operators of tests/test_gpu_fps_setup_bits.py that need none -- every
square, lx and x-stretched shape, the outflow channel, the 2- and 3-rank splits -- as a stand-alone program under the
sanitizers, and checks the table sizes, a slab's rows against the one-rank table's, the block fixed points, what an
outflow side changes and the pivot-shortcut census.  And how the solver (ns_solver.h, ns_solver.cpp, ns_observe.cpp)
uses the header."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "navierstokessolver_amd", "csrc")


def test_fps_tables_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "fps_tables_host_test")
    # (the sanitizer runtimes linked statically, as tests/test_timing_host.py does)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "fps_tables_host_test.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_solver_takes_its_pivots_from_the_header_and_its_layout_from_one_list():
    cpp = open(os.path.join(CSRC, "ns_solver.cpp")).read()
    sh = open(os.path.join(CSRC, "ns_solver.h")).read()   # (the solver's struct and what ns_observe.cpp shares)
    src = sh + cpp + open(os.path.join(CSRC, "ns_observe.cpp")).read()
    hdr = open(os.path.join(CSRC, "ns_fps_tables.h")).read()
    # Thomas' pivot recurrence is written once, in the header.  (Stricter than it must be: the solver holds no fma at
    # all today; a later fma there that is no pivot may narrow this to fps_setup's region)
    assert "std::fma(" not in src
    assert hdr.count("std::fma(-g,") == 1 and hdr.count("double fps_piv_next(") == 1
    assert "fps_piv_next(w, false," in hdr   # the shortcut's rows end before nx - 1: said at the call
    # no hand-summed block size beside the arena's list
    for old in ("n_mr", "n_pt", "total +"):
        assert old not in src, old
    assert cpp.count("hipMalloc(&d.mem") == 1 and cpp.count("hipMemset(d.mem") == 1
    # host-only: the header includes no HIP header (nor anything of the project's that does)
    inc = re.findall(r'#include\s*[<"]([^>"]+)[>"]', hdr)
    assert inc and not any("hip" in i or i.startswith("ns_") or "roc" in i for i in inc), inc
    # the direct solve's device pointers: one member of ns_solver
    body = sh.split("struct ns_solver {", 1)[1].split("\n};\n", 1)[0]   # (the struct's own closing brace)
    assert "} lo;" in body and body.count("} fpd;") == 1
    for old in ("fps_mem", "fps_tw", "fps_tw8", "fps_wk", "fps_ragg", "fps_gath", "fps_n", "s->fps_og", "s->og_b", "s->og_x1",
                "s->m0[ebga]", "s->dF", "s->dG", "s->dense_mem"):
        assert not re.search(old + r"\b", src), old
