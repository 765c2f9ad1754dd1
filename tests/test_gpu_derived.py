"""GPU: ns_derive -- pressure, vorticity, divergence, stream function and the run's integrals on the device --
against its NumPy statement (tests/derived_ref.py, itself pinned to the oracle by tests/test_derived_ref.py).

Tolerances: a single kernel against the restatement 1e-12 of the plane's max (the arithmetic alone gives ~1e-14:
test_derived_ref.py), psi 1e-12 of max |psi|, every integral 1e-12 relative (sums of <= 5000 terms of one sign, the
CFL number's reciprocal spacings: ~1e-15 each); min / max are those of the very arrays the call returned; the strips
and the thread-per-cell form agree bit for bit."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from derived_ref import STATS, DGrid, derived
from oracle import OGrid, OSolver
from polygons import ALL, NARROW

pytestmark = pytest.mark.gpu
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "navierstokessolver_amd", "host")

BC_CAVITY = [(2, 0.0), (2, 1.0), (2, 0.0), (2, 0.0)]
BC_CHANNEL = [(0, 1.0), (2, 0.0), (4, 0.0), (2, 0.0)]   # inlet W, walls N / S, NEUMANN outflow E
BC_FLOW = [(0, 1.0), (2, 0.0), (0, 1.0), (2, 0.5)]      # inlet both ends, moving wall S
BCSETS = {"cavity": BC_CAVITY, "channel": BC_CHANNEL, "flow": BC_FLOW}
# test_gpu_scalar's shapes -- 4x3: below one strip; 12x33: odd ny; 40x70: ny no multiple of 64 / 128; 21x130: a second
# column strip with two live columns (across the 124-column strip edge); 130x16: several strip-rows; 33x140 stretched
SHAPES = [(4, 3, -1, -1), (12, 33, -1, -1), (40, 70, -1, -1), (21, 130, -1, -1), (130, 16, -1, -1),
          (33, 140, 1.05, 0.95)]
SHAPE_IDS = [f"{a}x{b}{'s' if c > 0 else ''}" for a, b, c, _ in SHAPES]
DT, RE = 1e-3, 250.0
SUMS = ("ke", "enstrophy", "div_l2", "div_max", "cfl")


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


def lid_profile(nx):
    x = (np.arange(nx) + 0.5) / nx
    return (1 - (2 * x - 1) ** 16) ** 2


def rect_run(nsa, nx, ny, xr, yr, bc, u, v, phi, profile=None, **kw):
    gs = nsa.GpuSolver(nsa.rectangle(nx, ny, bc=bc, xratio=xr, yratio=yr), DT, RE)
    if profile is not None:
        gs.set_edge_profile(1, profile)
    gs.set_fields_compact(u=u, v=v, phi=phi)
    before = gs.fields()
    out = gs.derived(**kw)
    after = gs.fields()
    hx, hy = gs.hx.copy(), gs.hy.copy()
    gs.close()
    for a, b in zip(before, after):
        assert np.array_equal(a, b), "ns_derive changed a field"
    return out, hx, hy


def check(got, ref, mask=None):
    """The planes, psi and every integral against the restatement; min / max against the call's own arrays."""
    m = np.ones(ref["p"].shape, bool) if mask is None else mask
    for k in ("p", "vort", "div"):
        e = rel(got[k], ref[k])
        assert e <= 1e-12, (k, e)
        assert not np.any(got[k][~m]), f"{k}: a cell outside the domain is not exactly 0"
    e = rel(got["psi"], ref["psi"])
    assert e <= 1e-12, ("psi", e)
    for k in SUMS:
        assert abs(got[k] - ref[k]) <= 1e-12 * abs(ref[k]), (k, got[k], ref[k])
    assert got["vort_min"] == got["vort"][m].min() and got["vort_max"] == got["vort"][m].max()
    assert got["p_min"] == got["p"][m].min() and got["p_max"] == got["p"][m].max()
    assert got["psi_min"] == got["psi"].min() and got["psi_max"] == got["psi"].max()


# ------------------------------------------------------------------ 1 / 2. the kernels against the restatement, and
# the strips against the thread-per-cell form
CASES = [(s, n, False) for s in range(len(SHAPES)) for n in BCSETS] + [(2, "cavity", True), (3, "cavity", True)]


@pytest.mark.parametrize("shape,name,prof", CASES,
                         ids=[f"{SHAPE_IDS[s]}-{n}{'-profile' if p else ''}" for s, n, p in CASES])
def test_kernels_vs_restatement_and_each_other(gpu, monkeypatch, shape, name, prof):
    nx, ny, xr, yr = SHAPES[shape]
    bc = BCSETS[name]
    rng = np.random.default_rng(41)
    u, v, phi = (rng.uniform(-1, 1, (nx, ny)) for _ in range(3))
    profile = lid_profile(nx) if prof else None
    out = {}
    for mode in ("stream", "grid"):
        if mode == "grid":
            monkeypatch.setenv("NSGPU_CELL", "grid")
        else:
            monkeypatch.delenv("NSGPU_CELL", raising=False)
        out[mode], hx, hy = rect_run(gpu, nx, ny, xr, yr, bc, u, v, phi, profile)
    monkeypatch.delenv("NSGPU_CELL", raising=False)
    og = OGrid.rectangle(nx, ny, bc=bc, xratio=xr, yratio=yr)
    G = DGrid(hx, hy, og.id.reshape(nx, ny) >= 0, og.tag, bc, {1: profile} if prof else None)
    ref = derived(G, DT, RE, u, v, phi)
    print(f"{nx}x{ny} {name}: " + " ".join(f"{k} {rel(out['stream'][k], ref[k]):.1e}" for k in ("p", "vort", "div", "psi")))
    for mode in out:
        check(out[mode], ref)
    for k in ("p", "vort", "div", "psi"):
        assert np.array_equal(out["stream"][k], out["grid"][k]), f"{k}: strips and thread-per-cell differ"


# ------------------------------------------------------------------ 3. masked domains
MASKED = {**ALL, **{k: NARROW[k] for k in ("plus", "u_div1", "throat_out")}}


@pytest.mark.parametrize("name", sorted(MASKED))
def test_masked_domains(gpu, name):
    P = MASKED[name]
    og = OGrid(P["vertices"], P["xspec"], P["yspec"], P["bc"])
    gs = gpu.GpuSolver(gpu.polygon(P["vertices"], og.hx, og.hy, P["bc"]), DT, RE)
    G = DGrid.from_oracle(og, P["bc"])
    rng = np.random.default_rng(42)
    u, v, phi = (rng.uniform(-1, 1, og.N) for _ in range(3))
    gs.set_fields_compact(u=u, v=v, phi=phi)
    got = gs.derived()
    gs.close()
    ref = derived(G, DT, RE, G.plane(u), G.plane(v), G.plane(phi))
    print(f"{name}: " + " ".join(f"{k} {rel(got[k], ref[k]):.1e}" for k in ("p", "vort", "div", "psi")))
    check(got, ref, G.mask)
    assert rel(got["p"][G.mask], og.pressure(DT / (2 * RE), phi)) <= 1e-12
    assert rel(got["div"][G.mask], DT * og.divergence(DT, u, v)) <= 1e-12


# ------------------------------------------------------------------ 4. mid-run
def same(a, b):
    for k in ("p", "vort", "div", "psi"):
        assert np.array_equal(a[k], b[k]), k
    for k in STATS:
        assert a[k] == b[k], (k, a[k], b[k])


def test_mid_run(gpu):
    n, dt, re = 32, 1.0 / (8 * 32), 100.0   # (the power-of-two cavity: ns_step_async defers K5 into the next K1)
    mk = lambda: gpu.GpuSolver(gpu.cavity(n), dt, re)
    a, b = mk(), mk()
    sts = [a.step_async() for _ in range(6)]
    assert sum(s["k5_deferred"] for s in sts) >= 5
    da = a.derived()
    for _ in range(6):
        b.step()
    db = b.derived()
    same(da, db)
    a.close()
    # a solver that calls derived() after every step against a twin that never does
    twin = mk()
    for _ in range(6):
        twin.step()
    for _ in range(6):
        sb, st = b.step(), twin.step()
        b.derived()
        assert all(sb[q] == st[q] for q in ("umin", "umax", "vmin", "vmax", "it_u", "it_phi"))
    for x, y in zip(b.fields(), twin.fields()):
        assert np.array_equal(x, y), "derived() disturbed the run"
    # the approximate projection's divergence is visible, and it is the oracle's / the restatement's
    u, v, phi = b.fields()
    got = b.derived()
    b.close(); twin.close()
    og = OGrid.rectangle(n, n)
    ref = derived(DGrid.from_oracle(og, BC_CAVITY), dt, re, u, v, phi)
    dmax_oracle = np.max(np.abs(dt * og.divergence(dt, u.ravel(), v.ravel())))
    print(f"32^2 cavity after 12 steps: div_max {got['div_max']:.4e} (restatement {ref['div_max']:.4e}, oracle {dmax_oracle:.4e})")
    assert got["div_max"] > 1e-3
    assert abs(got["div_max"] - ref["div_max"]) <= 1e-12 * ref["div_max"]
    assert abs(ref["div_max"] - dmax_oracle) <= 1e-12 * dmax_oracle
    check(got, ref)


# ------------------------------------------------------------------ 5. selective output
def test_selective_output(gpu):
    nx, ny = 40, 70
    rng = np.random.default_rng(43)
    gs = gpu.GpuSolver(gpu.rectangle(nx, ny, bc=BC_CHANNEL), DT, RE)
    gs.set_fields_compact(*(rng.uniform(-1, 1, (nx, ny)) for _ in range(3)))
    part = gs.derived(p=False, psi=False)        # (first: only these two planes exist on the device)
    only = gs.derived(p=False, vort=False, div=False, psi=False)
    full = gs.derived()
    gs.close()
    assert "p" not in part and "psi" not in part and part["vort"].shape == (nx, ny)
    assert not any(k in only for k in ("p", "vort", "div", "psi"))
    assert np.array_equal(part["vort"], full["vort"]) and np.array_equal(part["div"], full["div"])
    for k in STATS:
        if k.startswith("psi"):
            assert math.isnan(part[k]) and math.isnan(only[k]) and not math.isnan(full[k])
        else:
            assert part[k] == full[k] == only[k], k
    assert full["psi"].shape == (nx + 1, ny + 1)


# ------------------------------------------------------------------ 6. refusals
def test_refusals(gpu, monkeypatch):
    L = gpu._lib
    gs = gpu.GpuSolver(gpu.rectangle(12, 10), DT, RE)
    assert L.lib().ns_derive(gs._h, None, None) == L.NS_EINVAL
    assert b"both NULL" in L.lib().ns_last_error()
    assert L.lib().ns_derive(None, None, ctypes.byref(L.NsDerivedStats())) == L.NS_EINVAL
    st = L.NsDerivedStats()
    assert L.lib().ns_derive(gs._h, None, ctypes.byref(st)) == 0 and st.ke == 0.0 and math.isnan(st.psi_min)
    gs.close()
    # nranks > 1 (a virtual slab: rank 2 of 4 with itself as every peer)
    monkeypatch.setenv("NSGPU_RCCL_LOOPBACK", "1")
    monkeypatch.setenv("NSGPU_VIRTUAL_ITERS", "4:1")
    gv = gpu.GpuSolver(gpu.cavity(128), 1.0 / 1024, 1000.0, device=0, rank=2, nranks=4)
    with pytest.raises(gpu.NsError, match="ns_derive: nranks > 1 is not supported"):
        gv.derived()
    gv.close()


# ------------------------------------------------------------------ 7. the driver's -derived
def test_driver_derived(tmp_path):
    n, steps, save = 16, 6, 6
    dt = 1.0 / (8 * n)
    (tmp_path / "grid").write_text(f"Vertices {{\n0 0\n0 1\n1 1\n1 0\n}}\nNx {{\n0 1 {n} -1\n}}\nNy {{\n0 1 {n} -1\n}}\n")
    (tmp_path / "sim").write_text(f"BC {{\n2 0\n2 1\n2 0\n2 0\n}}\ndt {dt!r}\nfinal_time {steps * dt!r}\nre 100.0\nsaveIter {save}\n")
    exe = os.path.join(HOST, "ns_main")
    run = lambda d, *opt: subprocess.run([exe, *opt, "../grid", "../sim"], capture_output=True, text=True, cwd=d,
                                         timeout=120).stdout
    (tmp_path / "with").mkdir(); (tmp_path / "without").mkdir()
    out1 = run(tmp_path / "with", "-derived")
    out0 = run(tmp_path / "without")
    assert "Solution Complete!" in out1 and "Solution Complete!" in out0
    # without the option: no Derived_* file, and stdout is the other run's minus its one extra line
    assert not list((tmp_path / "without").glob("Derived_*"))
    extra = [l for l in out1.splitlines() if l.startswith("derived:")]
    assert len(extra) == 1 and not any(l.startswith("derived:") for l in out0.splitlines())
    assert [l for l in out1.splitlines() if not l.startswith("derived:")] == out0.splitlines()
    f = extra[0].split()
    assert f[1::2] == ["ke", "enstrophy", "div_max", "cfl"] and all(float(x) > 0 for x in f[2::2])
    assert out1.splitlines()[-2] == extra[0]     # after the last step, before "Solution Complete!"
    d = np.loadtxt(tmp_path / "with" / f"Derived_{save}.csv", delimiter=",", skiprows=1)
    assert (tmp_path / "with" / f"Derived_{save}.csv").read_text().splitlines()[0] == "Point_X,Point_Y,Vorticity,Divergence,Pr"
    assert d.shape == (n * n, 5)
    flow = np.loadtxt(tmp_path / "with" / f"FlowData_{save}.csv", delimiter=",", skiprows=1)
    rows, r = [], 0                              # FlowData: each cell's row, then one per boundary face
    for i in range(n):
        for j in range(n):
            rows.append(r)
            r += 1 + (i == 0) + (i == n - 1) + (j == 0) + (j == n - 1)
    cells = flow[rows]
    assert np.array_equal(d[:, :2], cells[:, :2])
    # both columns are printed with 6 significant digits from values that agree to ~1e-14: equal but for a flip of
    # the last printed digit (1e-5 relative)
    assert np.all(np.abs(d[:, 4] - cells[:, 5]) <= 1e-5 * np.abs(cells[:, 5]) + 1e-300)
    assert np.mean(d[:, 4] == cells[:, 5]) > 0.9
    assert np.array_equal(np.loadtxt(tmp_path / "without" / f"FlowData_{save}.csv", delimiter=",", skiprows=1), flow)
