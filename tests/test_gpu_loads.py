"""GPU: the wall loads (ns_loads_*, k_load_faces / k_load_edges) against their NumPy statement (tests/loads_ref.py,
itself pinned to the oracle's budgets by tests/test_loads_ref.py).

Bars: the per-face arrays s, ds, tx, ty, un, tb, qn are the statement's own IEEE operations (helpers compiled with
contraction off) and must be array_equal; p agrees to 1e-12 of max |P| (ns_derive's bar); an edge sum lies within
nf 2^-52 sum |term| of the exactly rounded sum -- any order of adding nf terms stays inside that -- plus
1e-12 max |P| len for fpx / fpy."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from derived_ref import DGrid, cell_fields
from loads_ref import FACE_KEYS, SUMS, loads, sum_bounds
from navierstokessolver_amd.cavity import grid_file_text, sim_file_text
from oracle import OGrid
from polygons import ALL, NARROW, SPLITS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "navierstokessolver_amd", "host")

BC_CAVITY = [(2, 0.0), (2, 1.0), (2, 0.0), (2, 0.0)]
BC_CHANNEL = [(0, 1.0), (2, 0.0), (4, 0.0), (2, 0.0)]   # inlet W, walls N / S, NEUMANN outflow E
BC_FLOW = [(0, 1.0), (2, 0.0), (0, 1.0), (2, 0.5)]      # inlet both ends, moving wall S
BCSETS = {"cavity": BC_CAVITY, "channel": BC_CHANNEL, "flow": BC_FLOW}
# 4x3: one partly filled chunk per edge; 12x33 / 21x130: odd sizes, ld 128 / 256; 300x5 and 5x300: an edge of more than
# 256 faces -- two chunks -- in each orientation (y-normal: ld apart; x-normal: contiguous); 33x140 stretched
SHAPES = [(4, 3, -1, -1), (12, 33, -1, -1), (21, 130, -1, -1), (300, 5, -1, -1), (5, 300, -1, -1), (33, 140, 1.05, 0.95)]
SHAPE_IDS = [f"{a}x{b}{'s' if c > 0 else ''}" for a, b, c, _ in SHAPES]
S_MIXED = [("dirichlet", 1.0), ("zerograd",), ("dirichlet", -0.25), ("zerograd",)]   # edges W, N, E, S
S_CAVITY = [("zerograd",), ("dirichlet", 1.0), ("zerograd",), ("dirichlet", 0.0)]    # hot lid, cold floor
DT, RE, PE = 1e-3, 250.0, 71.0
Q = {k: n for n, k in enumerate(SUMS)}


def lid_profile(nx):
    x = (np.arange(nx) + 0.5) / nx
    return (1 - (2 * x - 1) ** 16) ** 2


def sums_array(rows):
    return np.array([[r[k] for k in SUMS] for r in rows])


def check_faces(got, ref, pmax, what):
    """One edge's per-face arrays against the statement's."""
    assert got["s"].shape == ref["s"].shape, (what, got["s"].shape, ref["s"].shape)
    for k in FACE_KEYS:
        if k == "p":
            err = np.max(np.abs(got[k] - ref[k]), initial=0.0)
            assert err <= 1e-12 * pmax, (what, k, err / pmax)
        else:
            assert np.array_equal(got[k], ref[k]), (what, k, float(np.max(np.abs(got[k] - ref[k]))))


def check_sums(got, ref, bound, what):
    err = np.abs(got - ref)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"{what}: the sums' worst error is {worst:.2e} of its bound")
    assert np.all(err <= bound), (what, np.argwhere(err > bound).tolist(), worst)


def statement(G, dt, re, u, v, phi, scalar=None):
    """(faces, sums, bounds, max |P|) of the statement."""
    faces, S = loads(G, dt, re, u, v, phi, scalar)
    pmax = float(np.max(np.abs(cell_fields(G, dt, re, u, v, phi)[2])))
    return faces, S, sum_bounds(faces, pmax), pmax


def everything(gs, scalar):
    out = list(gs.fields())
    if scalar:
        out += list(gs.scalar(cT0=True))
    return out


# ------------------------------------------------------------------ 1. the kernels against the statement: rectangles
CASES = [(s, n, None) for s in range(len(SHAPES)) for n in BCSETS] + [(2, "cavity", "profile"), (3, "cavity", "profile"),
                                                                      (1, "cavity", "scalar"), (3, "channel", "scalar"),
                                                                      (4, "flow", "scalar")]


@pytest.mark.parametrize("shape,name,extra", CASES, ids=[f"{SHAPE_IDS[s]}-{n}{'-' + x if x else ''}" for s, n, x in CASES])
def test_kernels_vs_statement(gpu, monkeypatch, shape, name, extra):
    nx, ny, xr, yr = SHAPES[shape]
    bc = BCSETS[name]
    rng = np.random.default_rng(61)
    u, v, phi, T = (rng.uniform(-1, 1, (nx, ny)) for _ in range(4))
    profile = lid_profile(nx) if extra == "profile" else None
    out = {}
    for mode in ("stream", "grid"):
        if mode == "grid":
            monkeypatch.setenv("NSGPU_CELL", "grid")
        else:
            monkeypatch.delenv("NSGPU_CELL", raising=False)
        gs = gpu.GpuSolver(gpu.rectangle(nx, ny, bc=bc, xratio=xr, yratio=yr), DT, RE)
        if profile is not None:
            gs.set_edge_profile(1, profile)
        if extra == "scalar":
            gs.enable_scalar(PE, S_MIXED)
            gs.set_scalar(T, rng.uniform(-1, 1, (nx, ny)))
        gs.set_fields_compact(u=u, v=v, phi=phi)
        gs.enable_loads()
        before = everything(gs, extra == "scalar")
        out[mode] = ([gs.wall_faces(e) for e in range(4)], sums_array(gs.loads()))
        after = everything(gs, extra == "scalar")
        hx, hy = gs.hx.copy(), gs.hy.copy()
        assert gs.load_stats()["total"] == 0        # (neither call writes a record)
        gs.close()
        for a, b in zip(before, after):
            assert np.array_equal(a, b), "a wall-load call changed a field"
    monkeypatch.delenv("NSGPU_CELL", raising=False)
    og = OGrid.rectangle(nx, ny, bc=bc, xratio=xr, yratio=yr)
    G = DGrid(hx, hy, og.id.reshape(nx, ny) >= 0, og.tag, bc, {1: profile} if profile is not None else None)
    faces, S, bound, pmax = statement(G, DT, RE, u, v, phi, (PE, T, S_MIXED) if extra == "scalar" else None)
    assert [len(F["s"]) for F in faces] == [ny, nx, ny, nx]
    for mode, (wf, got) in out.items():
        for e in range(4):
            check_faces(wf[e], faces[e], pmax, f"{mode} edge {e}")
        check_sums(got, S, bound, f"{nx}x{ny} {name} {mode}")
        if extra != "scalar":
            assert not np.any(got[:, Q["heat"]]) and not np.any(got[:, Q["heat_adv"]])
            assert all(not wf[e]["tb"].any() and not wf[e]["qn"].any() for e in range(4))
    for e in range(4):
        for k in FACE_KEYS:
            assert np.array_equal(out["stream"][0][e][k], out["grid"][0][e][k]), (e, k)
    assert np.array_equal(out["stream"][1], out["grid"][1])
    if extra == "scalar":
        # (a wall's normal face velocity is exactly 0: only a domain with an inlet or an outflow advects heat out)
        assert np.any(S[:, Q["heat"]] != 0.0) and np.any(S[:, Q["heat_adv"]] != 0.0) == (name != "cavity")
    if extra == "profile":      # the lid's shear follows the profile: not the uniform lid's
        G0 = DGrid(hx, hy, og.id.reshape(nx, ny) >= 0, og.tag, bc)
        assert np.max(np.abs(loads(G0, DT, RE, u, v, phi)[0][1]["tx"] - faces[1]["tx"])) > 1e-3


# ------------------------------------------------------------------ 2. polygons: one-face edges, cells with two
# boundary faces
MASKED = {**ALL, **{k: NARROW[k] for k in ("plus", "u_div1", "throat_out")},
          **{k: SPLITS[k] for k in ("split_2x2", "split_3x4")}}


@pytest.mark.parametrize("name", sorted(MASKED))
def test_masked_domains(gpu, name):
    P = MASKED[name]
    og = OGrid(P["vertices"], P["xspec"], P["yspec"], P["bc"])
    gs = gpu.GpuSolver(gpu.polygon(P["vertices"], og.hx, og.hy, P["bc"]), DT, RE)
    G = DGrid.from_oracle(og, P["bc"])
    rng = np.random.default_rng(62)
    u, v, phi = (rng.uniform(-1, 1, og.N) for _ in range(3))
    gs.set_fields_compact(u=u, v=v, phi=phi)
    gs.enable_loads()
    n_edges = len(P["bc"])
    before = gs.fields()
    wf = [gs.wall_faces(e) for e in range(n_edges)]
    got = sums_array(gs.loads())
    pd = gs.derived(vort=False, div=False, psi=False)["p"]
    after = gs.fields()
    gs.close()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    faces, S, bound, pmax = statement(G, DT, RE, G.plane(u), G.plane(v), G.plane(phi))
    for e in range(n_edges):
        check_faces(wf[e], faces[e], pmax, f"{name} edge {e}")
        at_cells = np.array([pd[i, j] for i, j, _ in faces[e]["cells"]])
        assert np.max(np.abs(wf[e]["p"] - at_cells), initial=0.0) <= 1e-12 * pmax
    check_sums(got, S, bound, name)
    assert sum(len(F["s"]) for F in faces) == int(np.sum(G.tag[G.mask] >= 0))


# ------------------------------------------------------------------ 3. in the step
def scalar_cavity(gpu, n=16, **kw):
    gs = gpu.GpuSolver(gpu.rectangle(n, n, bc=BC_CAVITY), 1.0 / (8 * n), 100.0, **kw)
    gs.enable_scalar(PE, S_CAVITY)
    gs.set_scalar(np.random.default_rng(63).uniform(0, 1, (n, n)))
    return gs


def cavity_grid(gs, n=16):
    og = OGrid.rectangle(n, n, bc=BC_CAVITY)
    return DGrid(gs.hx, gs.hy, np.ones((n, n), bool), og.tag, BC_CAVITY)


STAT_KEYS = ("umin", "umax", "vmin", "vmax", "it_u", "it_phi")


@pytest.mark.parametrize("every", [1, 3])
def test_in_step_sync(gpu, every):
    n, steps = 16, 7
    gs, tw = scalar_cavity(gpu), scalar_cavity(gpu)
    gs.enable_loads(every=every)
    G = cavity_grid(gs)
    want = []
    for k in range(steps):
        if k % every == 0:    # the statement applied to the twin's state before the step
            u, v, phi = tw.fields()
            want.append((k,) + statement(G, tw.dt, tw.re, u, v, phi, (PE, tw.scalar(), S_CAVITY))[1:3])
        a, b = gs.step(), tw.step()
        assert all(a[q] == b[q] for q in STAT_KEYS), (k, a, b)
        assert gs.scalar_stats()["it_t"] == tw.scalar_stats()["it_t"]
    hs, rec = gs.load_history()
    assert hs.tolist() == [w[0] for w in want] and rec.shape == (len(want), 4, 8)
    for r, (k, S, bound) in enumerate(want):
        check_sums(rec[r], S, bound, f"every {every} record {r} (step {k})")
    st = gs.load_stats()
    assert (st["total"], st["held"], st["steps"]) == (len(want), len(want), steps)
    for a, b, what in zip(gs.fields() + (gs.scalar(),), tw.fields() + (tw.scalar(),), ("u", "v", "phi", "T")):
        assert np.array_equal(a, b), what
    assert np.all(rec[:, :, Q["len"]] == 1.0)
    assert np.all(rec[1:, 1, Q["fvx"]] < 0.0) and np.any(rec[:, :, Q["heat"]] != 0.0)   # the fluid drags on the lid
    gs.close()
    tw.close()


def test_async_ring_sample_reset(gpu):
    steps = 7
    sync = scalar_cavity(gpu)
    sync.enable_loads()
    for _ in range(steps):
        sync.step()
    hs, hrec = sync.load_history()
    # ns_step_async: the same records, read while a deferred correction is pending
    asy = scalar_cavity(gpu)
    asy.enable_loads()
    sts = [asy.step_async() for _ in range(steps)]
    assert sum(s["k5_deferred"] for s in sts) >= steps - 1
    as_, arec = asy.load_history()
    assert np.array_equal(as_, hs) and np.array_equal(arec, hrec)
    # sample_loads settles the correction and writes a record with step -1: the current fields' sums
    asy.sample_loads()
    as_, arec = asy.load_history()
    assert as_.tolist() == list(range(steps)) + [-1]
    assert np.array_equal(arec[-1], sums_array(asy.loads()))
    for a, b in zip(asy.fields(), sync.fields()):
        assert np.array_equal(a, b)
    asy.close()
    # a ring of 4: the latest four, oldest first
    ring = scalar_cavity(gpu)
    ring.enable_loads(every=1, capacity=4)
    for _ in range(steps):
        ring.step()
    rs, rrec = ring.load_history()
    st = ring.load_stats()
    assert (st["total"], st["held"], st["steps"]) == (steps, 4, steps)
    assert rs.tolist() == [3, 4, 5, 6] and np.array_equal(rrec, hrec[3:])
    # reset: empty, and the steps count from it
    ring.reset_loads()
    st = ring.load_stats()
    assert (st["total"], st["held"], st["steps"]) == (0, 0, 0)
    rs, rrec = ring.load_history()
    assert rs.size == 0 and rrec.shape == (0, 4, 8)
    ring.step()
    sync.step()
    rs, rrec = ring.load_history()
    assert rs.tolist() == [0] and np.array_equal(rrec[0], sync.load_history()[1][steps])
    ring.close()
    sync.close()


# ------------------------------------------------------------------ 4. the conduction budget on the device
def test_conduction_budget(gpu):
    """Walls at rest, u = v = 0: one step is one Crank-Nicolson conduction step, solved to the residual it reports:
    |sum A dT + (dt / 2) (H1 + H0)| <= A_max sqrt(N) res_t ||rT||_2 + 1e-13 sum A |T| (Cauchy-Schwarz on the
    residual; the second term for the sums' round-off)."""
    nx, ny, dt, pe = 20, 24, 1.0 / 64, 40.0
    bc = [(2, 0.0)] * 4
    gs = gpu.GpuSolver(gpu.rectangle(nx, ny, bc=bc, xratio=1.05, yratio=0.95), dt, 100.0, rtol=1e-12)
    gs.enable_scalar(pe, S_MIXED)
    T0 = np.random.default_rng(64).uniform(-1, 1, (nx, ny))
    gs.set_scalar(T0)
    gs.enable_loads()
    H0 = math.fsum(r["heat"] for r in gs.loads())
    gs.step()
    H1 = math.fsum(r["heat"] for r in gs.loads())
    T1, res_t, rT = gs.scalar(), gs.scalar_stats()["res_t"], gs.scalar_rhs()
    u, v, _ = gs.fields()
    assert not u.any() and not v.any()
    A = np.outer(gs.hx, gs.hy)
    gs.close()
    lhs = math.fsum((A * (T1 - T0)).ravel())
    gap = abs(lhs + 0.5 * dt * (H0 + H1))
    bound = A.max() * math.sqrt(nx * ny) * res_t * float(np.linalg.norm(rT)) + 1e-13 * math.fsum((A * np.abs(T1)).ravel())
    print(f"conduction budget: gap {gap:.3e}, bound {bound:.3e} (res_t {res_t:.2e}, sum A dT {lhs:.3e})")
    assert res_t <= 1e-10 and abs(lhs) > 1e-6     # (the bound means something: the solve converged, heat moved)
    assert gap <= bound


# ------------------------------------------------------------------ 5. refusals
def test_refusals(gpu, monkeypatch):
    L = gpu._lib
    lib = L.lib()
    err = lambda: lib.ns_last_error().decode()
    desc, st, n = L.NsLoadDesc(1, 8), L.NsLoadStats(), ctypes.c_int64()
    buf = np.zeros(64)
    dp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    fs = L.NsLoadFaces()
    for call in (lambda: lib.ns_loads_enable(None, ctypes.byref(desc)), lambda: lib.ns_loads_sample(None),
                 lambda: lib.ns_loads_edges(None, dp), lambda: lib.ns_loads_face_count(None, 0, ctypes.byref(n)),
                 lambda: lib.ns_loads_faces(None, 0, ctypes.byref(fs)), lambda: lib.ns_loads_history(None, 0, 0, None, dp),
                 lambda: lib.ns_loads_reset(None), lambda: lib.ns_loads_last(None, ctypes.byref(st))):
        assert call() == L.NS_EINVAL and "null solver" in err()
    gs = gpu.GpuSolver(gpu.rectangle(12, 10), 1e-3, 100.0)
    assert lib.ns_loads_enable(gs._h, None) == L.NS_EINVAL and "descriptor is NULL" in err()
    for call in (gs.sample_loads, gs.loads, lambda: gs.wall_faces(0), gs.load_history, gs.reset_loads, gs.load_stats):
        with pytest.raises(gpu.NsError, match=r"wall loads are not enabled \(ns_loads_enable\)"):
            call()
    with pytest.raises(gpu.NsError, match="every = 0 is less than 1"):
        gs.enable_loads(every=0)
    with pytest.raises(gpu.NsError, match="capacity = 0 is less than 1"):
        gs.enable_loads(capacity=0)
    with pytest.raises(gpu.NsError, match="capacity = -3 is less than 1"):
        gs.enable_loads(capacity=-3)
    st0 = gs.step()     # (a refused enable leaves the solver as it was)
    gs.enable_loads(every=1, capacity=8)
    with pytest.raises(gpu.NsError, match="already enabled"):
        gs.enable_loads()
    for e in (-1, 4, 99):
        with pytest.raises(gpu.NsError, match=f"edge {e} of a grid with 4 edges"):
            gs.wall_faces(e)
    assert lib.ns_loads_face_count(gs._h, 1, ctypes.byref(n)) == 0 and n.value == 12
    for _ in range(3):
        gs.step()
    for first, cnt in ((-1, 1), (0, 4), (3, 1), (4, 0), (0, -1)):
        assert lib.ns_loads_history(gs._h, first, cnt, None, dp) == L.NS_EINVAL, (first, cnt)
        assert f"the range [{first}, {first + cnt}) is outside [0, 3)" in err()
    assert lib.ns_loads_history(gs._h, 1, 2, None, dp) == 0 and lib.ns_loads_history(gs._h, 3, 0, None, None) == 0
    assert lib.ns_loads_edges(gs._h, None) == L.NS_EINVAL and "out is NULL" in err()
    assert lib.ns_loads_last(gs._h, None) == L.NS_EINVAL and "out is NULL" in err()
    assert st0["it_phi"] >= 1
    gs.close()
    # nranks > 1 (a virtual slab: rank 2 of 4 with itself as every peer)
    monkeypatch.setenv("NSGPU_RCCL_LOOPBACK", "1")
    monkeypatch.setenv("NSGPU_VIRTUAL_ITERS", "4:1")
    gv = gpu.GpuSolver(gpu.cavity(128), 1.0 / 1024, 1000.0, device=0, rank=2, nranks=4)
    with pytest.raises(gpu.NsError, match="ns_loads_enable: nranks > 1 is not supported"):
        gv.enable_loads()
    gv.close()


# ------------------------------------------------------------------ 6. the driver's -loads
def test_driver_loads(gpu, tmp_path):
    n, steps, re = 16, 6, 100.0
    dt = 1.0 / (8 * n)
    (tmp_path / "grid").write_text(grid_file_text(n, n))
    (tmp_path / "sim").write_text(sim_file_text(dt, steps * dt, re, 1000, BC_CAVITY))
    exe = os.path.join(HOST, "ns_main")
    out = subprocess.run([exe, "-loads", "2", "grid", "sim"], capture_output=True, text=True, cwd=tmp_path,
                         timeout=120).stdout
    assert "Solution Complete!" in out, out
    assert [l for l in out.splitlines() if l.startswith("loads:")] == [f"loads: records={steps // 2} steps={steps}"], out
    rows = (tmp_path / "Loads.csv").read_text().splitlines()
    assert rows[0] == "Step,Edge,Len,Fpx,Fpy,Fvx,Fvy,Q,Heat,HeatAdv" and len(rows) == 1 + (steps // 2) * 4
    d = np.loadtxt(tmp_path / "Loads.csv", delimiter=",", skiprows=1)
    gs = gpu.GpuSolver(gpu.rectangle(n, n, bc=BC_CAVITY), dt, re)
    gs.enable_loads(every=2)
    for _ in range(steps):
        gs.step()
    hs, rec = gs.load_history()
    gs.close()
    assert d[:, 0].tolist() == np.repeat(hs, 4).tolist() and d[:, 1].tolist() == [0, 1, 2, 3] * (steps // 2)
    # (%.17g round-trips a double; the driver's run and this one agree like test_gpu_averages' driver test: 1e-12 of
    # the column's largest entry, a column that is identically 0 exactly)
    for col in range(8):
        a, b = d[:, 2 + col], rec.reshape(-1, 8)[:, col]
        assert np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b)), (col, float(np.max(np.abs(a - b))))
    assert np.all(d[:, 2] == 1.0) and np.any(d[:, 2 + Q["fvx"]] != 0.0) and np.any(d[:, 2 + Q["fpy"]] != 0.0)
    # without the option: no file, no line
    (tmp_path / "plain").mkdir()
    out0 = subprocess.run([exe, "../grid", "../sim"], capture_output=True, text=True, cwd=tmp_path / "plain",
                          timeout=120).stdout
    assert "Solution Complete!" in out0 and "loads:" not in out0
    assert not (tmp_path / "plain" / "Loads.csv").exists()
    assert [l for l in out.splitlines() if not l.startswith("loads:")] == out0.splitlines()


# ------------------------------------------------------------------ 7. timing
def test_timing(gpu):
    steps, every = 4, 2
    runs = {}
    for mode in ("loads", "twin"):
        gs = scalar_cavity(gpu, timing=True)
        if mode == "loads":
            gs.enable_loads(every=every)
        runs[mode] = [gs.step() for _ in range(steps)]
        if mode == "loads":
            st = gs.load_stats()
            assert st["total"] == 2 and st["steps"] == steps and st["n_kernels"] == 2 * 2, st   # two launches a sample
            assert np.isfinite(st["t_kernel_ms"]) and st["t_kernel_ms"] > 0
            again = gs.load_stats()      # handed out once
            assert again["n_kernels"] == 0 and again["t_kernel_ms"] == 0.0 and again["total"] == 2
            gs.sample_loads()
            assert gs.load_stats()["n_kernels"] == 2
            gs.loads()                   # (no record: not a sample)
            assert gs.load_stats()["n_kernels"] == 0
        gs.close()
    counts = [k for k in runs["loads"][0] if k.startswith("n_") or k in ("it_u", "it_phi", "k5_deferred")]
    assert len(counts) >= 10
    for a, b in zip(runs["loads"], runs["twin"]):
        assert [a[k] for k in counts] == [b[k] for k in counts]
