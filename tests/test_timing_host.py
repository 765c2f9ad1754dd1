"""The kernel-timing recorder (navierstokessolver_amd/csrc/ns_timing.h) on the host: tests/timing_host_test.cpp
drives it through a stub of the event calls -- open / close / drain by kind, the weight, event reuse across steps,
K5 kept across other kinds' drains, the empty interval, an abandoned interval leaving no dispatch stamp armed, growth
to 1000 live intervals without pre-sizing -- in both modes, as a stand-alone program under the sanitizers.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "navierstokessolver_amd", "csrc")


def test_recorder_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "timing_host_test")
    # (the sanitizer runtimes linked statically, as tests/test_knobs.py does)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "timing_host_test.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_solver_has_one_timing_member_and_no_event_pool_of_its_own():
    hdr = open(os.path.join(CSRC, "ns_solver.h")).read()
    src = hdr + "".join(open(os.path.join(CSRC, f)).read() for f in ("ns_solver.cpp", "ns_observe.cpp"))
    for old in ("hipEventCreate(", "evtag", "hev", "hcomp", "kev["):
        assert old not in src, old
    body = hdr.split("struct ns_solver {", 1)[1].split("\n};\n", 1)[0]   # (the struct's own closing brace)
    assert "} lo;" in body and body.count("Timing ") == 1
