"""The NSGPU_* environment knobs have one table, navierstokessolver_amd/csrc/ns_knobs.h: its parser (defaults,
clamps, string values) through a small C++ program, and that no other source file of the library reads the
environment for a knob.  No GPU."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "navierstokessolver_amd", "csrc")
NOT_KNOBS = {"NSGPU_LIB", "NSGPU_ABI_VERSION"}   # the Python loader's library path, the header's version macro

# every field of nsg::Knobs with its default (ns_knobs.h's initialisers, restated)
DEFAULTS = dict(
    rhs=0, k1s=0, k1_l=0, cell_grid=0, mask_cell=1, apply_grid=0, sd3=0, cv_blk=1, strip_rows=0, tiled=0, sweep3=1,
    sweep3_res=1, helm_uv=1, helm_band=1, band6=0, band_w=-1, band_sweeps=-1, ext_timing=1, speculate=1, k5_guess=0,
    k5_defer=1, fuse_restrict=1, fuse_prolong=1, tile_small=1, fuse4=1, gin=0, mg_predict=1, phi_extrap=-1,
    mg_omega=0.0, mg_omega_set=0, pair_min_cells=2048 * 2048, direct_cells=128 * 128, agg_cells=1024 * 1024, outflow_pc_wall=0,
    fps=1, fps_dense=1, fps_outflow=1, fps_check=16, fps_passes=0, fps_fuse=-1, fps_real=1, fps_grid=0, fps_ptab=2,
    fps_onegather=1, fps_defer=1, fps_pc=1, cap=1, cap_max=4096, cap_outflow=1, mask_rb=1, mask_rbt=1, mask_mt=1,
    mask_band=6, mask_band_w=-1, overlap=-1, comm_cus=0, bus=1, deep=1, loopback=0, virtual_iters="", virtual_iters_len=0,
    virtual_copy=0, time_pairs=0, verbose=0)


def _program(tmp_path, *flags):
    prints = "\n".join(
        f' std::printf("{f}=%s\\n", k.{f});' if isinstance(d, str) else
        f' std::printf("{f}=%.17g\\n", (double)k.{f});' for f, d in DEFAULTS.items())
    src = '#include <cstdio>\n#include "ns_knobs.h"\nint main() {\n const nsg::Knobs k = nsg::Knobs::from_env();\n' \
          + prints + "\n return 0;\n}\n"
    exe = str(tmp_path / ("ns_knobs_print" + "".join(flags).replace("=", "_").replace(",", "_")))
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, "-x", "c++", "-o", exe, "-"],
                   input=src, text=True, check=True)
    return exe


@pytest.fixture(scope="module")
def parse(tmp_path_factory):
    exe = _program(tmp_path_factory.mktemp("knobs"))

    def run(**env):
        clean = {k: v for k, v in os.environ.items() if not k.startswith("NSGPU_")}
        out = subprocess.run([exe], env={**clean, **env}, capture_output=True, text=True, check=True).stdout
        kv = dict(line.split("=", 1) for line in out.splitlines())
        return {f: kv[f] if isinstance(d, str) else float(kv[f]) for f, d in DEFAULTS.items()}
    return run


def test_struct_has_no_field_the_test_does_not_print():
    body = open(os.path.join(CSRC, "ns_knobs.h")).read().split("struct Knobs {", 1)[1].split("static Knobs from_env", 1)[0]
    fields = re.findall(r"^\s+(?:int|long|double|char)\s+(\w+)", body, re.M)
    assert sorted(fields) == sorted(DEFAULTS)


def test_defaults_in_a_clean_environment(parse):
    assert parse() == DEFAULTS


@pytest.mark.parametrize("var,val,field,want", [
    ("NSGPU_BAND_SWEEPS", "7", "band_sweeps", 6), ("NSGPU_BAND_SWEEPS", "1", "band_sweeps", 3),
    ("NSGPU_MASK_BAND", "9", "mask_band", 6), ("NSGPU_MASK_BAND", "-3", "mask_band", 0),
    ("NSGPU_PHI_EXTRAP", "9", "phi_extrap", 4), ("NSGPU_PHI_EXTRAP", "-2", "phi_extrap", 0),
    ("NSGPU_DIRECT_CELLS", "-5", "direct_cells", 0), ("NSGPU_BAND_W", "0", "band_w", 1),
    ("NSGPU_MASK_BAND_W", "-4", "mask_band_w", 1), ("NSGPU_FPS_CHECK", "-1", "fps_check", 0),
    ("NSGPU_STRIP_ROWS", "17", "strip_rows", 16), ("NSGPU_STRIP_ROWS", "200", "strip_rows", 64),
    ("NSGPU_STRIP_ROWS", "3", "strip_rows", 0), ("NSGPU_FPS_PASSES", "3", "fps_passes", 3),
    ("NSGPU_FPS_PASSES", "5", "fps_passes", 2), ("NSGPU_FPS_FUSE", "0", "fps_fuse", 0),
    ("NSGPU_OVERLAP", "0", "overlap", 0), ("NSGPU_OVERLAP", "1", "overlap", 1), ("NSGPU_COMM_CUS", "-8", "comm_cus", 0),
    ("NSGPU_FPS", "0", "fps", 0), ("NSGPU_FPS_REAL", "0", "fps_real", 0), ("NSGPU_MASK_CELL", "0", "mask_cell", 0),
    ("NSGPU_TIME_PAIRS", "1", "time_pairs", 1)])
def test_clamps_and_roundings(parse, var, val, field, want):
    got = parse(**{var: val})
    assert got[field] == want
    assert {f: v for f, v in got.items() if f != field} == {f: v for f, v in DEFAULTS.items() if f != field}


def test_knobs_with_a_companion_field(parse):
    """NSGPU_MG_OMEGA takes any number (a flag says it was set); NSGPU_VIRTUAL_ITERS keeps its length, so that
    ns_create can refuse a list that did not fit instead of replaying a cut one."""
    assert parse(NSGPU_MG_OMEGA="-0.5") == {**DEFAULTS, "mg_omega": -0.5, "mg_omega_set": 1}
    assert parse(NSGPU_VIRTUAL_ITERS="4:2,6:3") == {**DEFAULTS, "virtual_iters": "4:2,6:3", "virtual_iters_len": 7}


@pytest.mark.parametrize("var,good,field,want", [
    ("NSGPU_RHS", "global", "rhs", 2), ("NSGPU_RHS", "lds", "rhs", 1), ("NSGPU_SWEEP", "tiled", "tiled", 1),
    ("NSGPU_CELL", "grid", "cell_grid", 1), ("NSGPU_APPLY", "grid", "apply_grid", 1),
    ("NSGPU_MASK_HELM", "krylov", "mask_rb", 0), ("NSGPU_OUTFLOW_PC", "wall", "outflow_pc_wall", 1)])
def test_string_knobs(parse, var, good, field, want):
    assert parse(**{var: good})[field] == want != DEFAULTS[field]
    if var != "NSGPU_RHS":   # (any other value of NSGPU_RHS has always meant the LDS-tiled K1)
        assert parse(**{var: "bogus"}) == parse() == DEFAULTS


def test_an_overlong_replay_list_is_not_cut(parse):
    got = parse(NSGPU_VIRTUAL_ITERS=",".join(["4:2"] * 2000))
    assert got["virtual_iters"] == "" and got["virtual_iters_len"] == 7999   # (ns_create refuses it by its length)


def test_parser_is_clean_under_sanitizers(tmp_path):
    # (the sanitizer runtimes linked statically: a stand-alone program, whatever else the process loads)
    exe = _program(tmp_path, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                   "-static-libubsan")
    env = {k: v for k, v in os.environ.items() if not k.startswith("NSGPU_")}
    env.update(NSGPU_VIRTUAL_ITERS=",".join(["4:2"] * 2000), NSGPU_RHS="", NSGPU_BAND_SWEEPS="-2147483648",
               NSGPU_CELL="grid", NSGPU_MASK_BAND="-7")
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_only_the_table_reads_the_environment_for_a_knob():
    for path in glob.glob(os.path.join(CSRC, "*")):
        if os.path.isfile(path) and os.path.basename(path) != "ns_knobs.h":
            assert 'getenv("NSGPU_' not in open(path, errors="replace").read(), path


def test_every_knob_the_tests_set_is_in_the_table():
    table = set(re.findall(r'"(NSGPU_[A-Z0-9_]+)"', open(os.path.join(CSRC, "ns_knobs.h")).read()))
    used = set()
    for path in glob.glob(os.path.join(ROOT, "tests", "*.py")):
        txt = open(path).read()
        used |= set(re.findall(r'monkeypatch\.(?:setenv|delenv)\(\s*"(NSGPU_[A-Z0-9_]+)"', txt))
        used |= set(re.findall(r'"(NSGPU_[A-Z0-9_]+)"', txt))   # (names that reach setenv through a variable)
    used -= NOT_KNOBS
    assert len(used) > 30
    assert used <= table, sorted(used - table)
