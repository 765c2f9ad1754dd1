"""(r8) The direct solve's recurrences (k_fps_t1b / k_fps_t2b) run a constant-coefficient body on the FIXED chunks: past
a 128-mode block's fixed-point row every pivot is the constant pinf, so pw / p and -pe / p are formed once per mode
instead of once per row (FpsArgs::cfix, classified by fps_setup; NSGPU_VERBOSE prints the census this file reads).  The
fixed body applies the general body's operations to the same operands, so nothing may change by a bit.

References, all inside the same library:
  * NSGPU_FPS_PTAB=0 -- a division per row and mode, no fixed point, so every chunk takes the general body: u, v, phi,
    both monitors and it_u, it_phi, res_u, res_v of every step BYTE-EQUAL (mode 2's fixed point is exact, so the parent
    commit agrees with its own PTAB=0 bit for bit as well: bench planes of the parent and of this build are equal);
  * NSGPU_FPS_PASSES=3 -- the three-pass recurrences: phi modulo its mean to 1e-12 of max|phi|
    (test_two_pass_recurrences_equal_three_pass's bound);
  * one solve of a random right-hand side against the oracle's sequential direct solve: <= 1e-10 of max|phi|
    (test_direct_solve_matches_oracle's bound), on the first and the last shapes.

Every case is the cavity from rest at Re 100, 6 ns_step_async calls, a closing monitor() and one more step, as in
test_gpu_tails.py.  Shapes (nx x ny; square cells unless lx is given), the smallest at which each piece can go wrong
(the pivot shortcut needs ny > 128 and nx - 1 > 64):
  64 x 256          two blocks, too few rows for the pivot shortcut (nx - 1 = 63): the census reports 0 and nothing
                    changes.  (The issue lists 80 x 256 here; its census shows block 1 at its fixed point from row 16
                    on, chunks 1 to 3 fixed -- with ny = 256 no nx > 65 is without a fixed chunk);
  200 x 512         block 1 fixed from row 26, no multiple of 16: the chunk holding it is general, the next one fixed;
                    nx no multiple of 16 (a ragged last chunk) nor of 64 (a ragged last group).  (The issue lists
                    200 x 256, whose block 1 is fixed from row 16, a chunk's first row);
  520 x 1024        8 blocks with different first fixed chunks; 33 chunks in 9 groups, some mixing general and fixed;
  1040 x 1024       the segmented group scan, 65 chunks;
  2048 x 512, lx 4  as the issue lists it -- but lx = 4 = nx / ny makes these cells square too (pw = 1 / hy^2), so
  2048 x 512, lx 8  is added: hx = 2 hy, pw = pe = 1 / (4 hy^2), g and q are not the square case's values (and block 0,
                    with mode 0 and its shift, reaches its fixed point inside the grid).
Each case asserts the census it expects (0 fixed chunks on the first shape, > 0 on every other, and there a block
whose first fixed chunk lies inside the grid, not at its start) and fails -- never skips -- if its path was not taken."""
import os
import re

import numpy as np
import pytest

from oracle import OGrid

pytestmark = pytest.mark.gpu

STEPS = 6
RE = 100.0
# (nx, ny, lx or None for square cells)
SHAPES = [(64, 256, None), (200, 512, None), (520, 1024, None), (1040, 1024, None), (2048, 512, 4.0), (2048, 512, 8.0)]
IDS = [f"{nx}x{ny}" + (f"-lx{lx:g}" if lx else "") for nx, ny, lx in SHAPES]
KEYS = ("umin", "umax", "vmin", "vmax", "it_u", "it_phi", "res_u", "res_v")
CENSUS = re.compile(r"nsgpu fps: fixed chunks (\d+) of (\d+) \(block, chunk\) pairs([^\n]*)")

_runs = {}


def _lx(nx, ny, lx):
    return lx if lx else nx / ny


def _census(err):
    m = CENSUS.search(err)
    assert m, "no census line on stderr:\n" + err[-2000:]
    def ints(label):
        q = re.search(label + r":([^\n;]*)", m.group(3))
        return [None if t == "-" else int(t) for t in q.group(1).split()] if q else []

    return dict(fixed=int(m.group(1)), pairs=int(m.group(2)), rows=ints("fixed-point rows"), first=ints("first fixed chunks"))


def _run(gpu, capfd, nx, ny, lx, env):
    """One run (cached per shape and environment) under NSGPU_VERBOSE, with its census."""
    key = (nx, ny, lx, tuple(sorted(env.items())))
    if key in _runs:
        return _runs[key]
    env = {**env, "NSGPU_VERBOSE": "1"}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        L = _lx(nx, ny, lx)
        capfd.readouterr()
        gs = gpu.GpuSolver(gpu.rectangle(nx, ny, lx=L), min(L / nx, 1.0 / ny) / 8, RE)
        census = _census(capfd.readouterr().err)
        stats = [gs.step_async() for _ in range(STEPS)]
        mon = gs.monitor()
        after = gs.step_async()
        mon2 = gs.monitor()
        fields = [a.copy() for a in gs.fields()]
        gs.close()
        capfd.readouterr()   # (the verbose per-step lines)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    _runs[key] = dict(stats=stats, mon=mon, after=after, mon2=mon2, fields=fields, census=census)
    return _runs[key]


def _same(x, y):
    return (np.isnan(x) and np.isnan(y)) or x == y


def demean(x):
    x = np.asarray(x).ravel()
    return x - x.mean()


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _check_census(nx, ny, census):
    nch = (nx + 15) // 16
    assert census["pairs"] == ((ny + 127) // 128) * nch, census
    if nx == 64:
        assert census["fixed"] == 0, census
        return
    assert census["fixed"] > 0, census
    inside = [c for c in census["first"] if c is not None]
    # the general and the fixed body both run: every fixed block starts past its first chunk
    assert inside and all(0 < c < nch - 1 for c in inside), census
    if nx == 200:
        # block 1's fixed-point row is no multiple of 16: the chunk holding it is general, the next one fixed
        assert census["rows"][1] % 16 != 0 and census["first"][1] == census["rows"][1] // 16 + 1, census
    if (nx, ny) in ((520, 1024), (1040, 1024)):
        assert len(set(inside)) > 1, census                 # blocks with different first fixed chunks
        assert any(c % 4 != 0 for c in inside), census      # a group that mixes general and fixed chunks


@pytest.mark.parametrize("nx,ny,lx", SHAPES, ids=IDS)
def test_fixed_chunks_change_no_bit_against_divisions_everywhere(gpu, capfd, nx, ny, lx):
    a = _run(gpu, capfd, nx, ny, lx, {})
    b = _run(gpu, capfd, nx, ny, lx, {"NSGPU_FPS_PTAB": "0"})
    print(f"{nx}x{ny}: census {a['census']}")
    _check_census(nx, ny, a["census"])
    assert b["census"]["fixed"] == 0, b["census"]           # (the reference ran the general body everywhere)
    assert all(s["it_phi"] == 1 for s in a["stats"] + b["stats"])
    for x, y in zip(a["stats"] + [a["after"]], b["stats"] + [b["after"]]):
        assert all(_same(x[k], y[k]) for k in KEYS), (x, y)
    assert a["mon"] == b["mon"] and a["mon2"] == b["mon2"]
    assert all(np.isfinite(v) for v in a["mon2"])
    for x, y in zip(a["fields"], b["fields"]):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("nx,ny,lx", SHAPES, ids=IDS)
def test_fixed_chunks_against_three_pass_recurrences(gpu, capfd, nx, ny, lx):
    a = _run(gpu, capfd, nx, ny, lx, {})
    b = _run(gpu, capfd, nx, ny, lx, {"NSGPU_FPS_PASSES": "3"})
    _check_census(nx, ny, a["census"])
    dp = rel(demean(a["fields"][2]), demean(b["fields"][2]))
    print(f"{nx}x{ny}: two-pass with fixed chunks vs three-pass: phi {dp:.3e}")
    assert dp <= 1e-12, dp


@pytest.mark.parametrize("nx,ny,lx", [SHAPES[0], SHAPES[-2], SHAPES[-1]], ids=[IDS[0], IDS[-2], IDS[-1]])
def test_fixed_chunks_solve_matches_oracle(gpu, capfd, monkeypatch, nx, ny, lx):
    monkeypatch.setenv("NSGPU_VERBOSE", "1")
    L = _lx(nx, ny, lx)
    rng = np.random.default_rng(nx * 7 + ny)
    og = OGrid.rectangle(nx, ny, lx=L)
    assert og.fps_ok()
    capfd.readouterr()
    gs = gpu.GpuSolver(gpu.rectangle(nx, ny, lx=L), 1e-3, RE, rtol=1e-11)
    _check_census(nx, ny, _census(capfd.readouterr().err))
    b = rng.uniform(-100, 100, nx * ny)
    gs.set(gpu.NS_ARR_PHI, np.zeros(nx * ny))
    gs.set(gpu.NS_ARR_RPHI, b)
    its, res = gs.kernel(gpu.NS_K_POIS_SOLVE)[:2]
    g = demean(gs.get(gpu.NS_ARR_PHI))
    gs.close()
    d = rel(g, demean(og.fps_solve(b)))
    print(f"{nx}x{ny} lx {L:g}: direct solve residual {res:.3e}, against the oracle {d:.3e}")
    assert its == 1 and res <= 1e-11, (its, res)
    assert d <= 1e-10, d
