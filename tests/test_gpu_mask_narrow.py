"""Masked domains with narrow features and split box complements (polygons.NARROW, SPLITS, NARROW_TALL) on the GPU,
against the oracle -- test_gpu_mask.py's comparisons and tolerances at the shapes that suite never reaches:
  * 2-cell arms and throats and a divider one cell thick: the MUSCL reach guards (TopoMask::in(+-2) lands in the
    domain again across the divider), outside cells referenced by 2 to 3 interface faces, domains with no FC_DEEP
    cell (the streaming k_cell_s has nothing to do), wall bands that cover the whole domain, Helmholtz tiles larger
    than the domain;
  * bounding boxes whose outside falls into 2 to 4 connected components: the capacitance matrix has one null vector
    per component (ns_solver.cpp cap_setup; tests/test_capacitance_method.py restates it on the CPU), so the exact
    solve must hold there too, and deterministically -- not by the luck of a rounding-level pivot;
  * tiny five-vertex rectangles (every cell in the domain, no interface face);
  * 1024 columns: the masked inverse transform (launch_fps_idct_masked), the capacitance solve's direct_x branch;
  * x-slabs cut through the dumbbell's throat and along the divider.
Tolerances: single kernels 1e-12 relative; converged solves 1e-8 against the oracle (phi modulo its mean), 1e-9
between the two GPU paths; full steps 1e-9 / 1e-7 at rtol 1e-11 and 1e-6 / 1e-4 at the reference's 1e-8."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import OGrid, OSolver
from polygons import NARROW, NARROW_COMPONENTS, NARROW_TALL, SPLITS

POLY = {**NARROW, **SPLITS, **NARROW_TALL}
SMALL = sorted(NARROW) + sorted(SPLITS)
HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu


def pair(gpu, name, dt, re, **kw):
    P = POLY[name]
    og = OGrid(P["vertices"], P["xspec"], P["yspec"], P["bc"])
    gs = gpu.GpuSolver(gpu.polygon(P["vertices"], og.hx, og.hy, P["bc"]), dt, re, **kw)
    return og, gs, gs.grid.mask.ravel()


def plane(m, x):
    p = np.zeros(m.size)
    p[m] = x
    return p


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a).ravel() - np.asarray(b).ravel())) / max(np.max(np.abs(b)), 1e-300))


def demean(x):
    return x - x.mean()


def fill(rng, name, og, m, k):
    """k random compact fields.  u_div1: the two arms (left of the divider's column 9 and under it / right of it)
    differ in sign and scale, +1 +- 0.1 and -100 +- 10, so a stencil that reaches across the one-cell divider
    misses by orders of magnitude; arms: per arm, the compact cells in it."""
    if name != "u_div1":
        return [rng.uniform(-1, 1, og.N) for _ in range(k)], [np.ones(og.N, bool)]
    left = (np.flatnonzero(m) // og.ny) <= 9
    return ([np.where(left, rng.uniform(0.9, 1.1, og.N), rng.uniform(-110, -90, og.N)) for _ in range(k)],
            [left, ~left])


@pytest.mark.parametrize("name", SMALL)
def test_narrow_k1_rhs_velocity(gpu, name):
    rng = np.random.default_rng(21)
    dt, re = 1e-3, 250.0
    og, gs, m = pair(gpu, name, dt, re)
    (u, v, phi, cu, cv), arms = fill(rng, name, og, m, 5)
    for a, x in ((gpu.NS_ARR_U, u), (gpu.NS_ARR_V, v), (gpu.NS_ARR_PHI, phi), (gpu.NS_ARR_CU, cu),
                 (gpu.NS_ARR_CV, cv)):
        gs.set(a, plane(m, x))
    sums = gs.kernel(gpu.NS_K_RHS)
    gx, gy = og.grad_phi(phi)
    ru, rv, cu1, cv1 = og.rhs_velocity(dt, re, u, v, gx, gy, cu, cv)
    for a, ref in ((gpu.NS_ARR_RU, ru), (gpu.NS_ARR_RV, rv), (gpu.NS_ARR_CU, cu1), (gpu.NS_ARR_CV, cv1)):
        got = gs.get(a).ravel()
        for arm in arms:
            err = rel(got[m][arm], ref[arm])
            assert err <= 1e-12, (a, err)
        assert not np.any(got[~m]), "cells outside the domain must stay 0"
    assert abs(sums[0] - np.sum(ru * ru)) <= 1e-11 * np.sum(ru * ru)


@pytest.mark.parametrize("cells", ["1", "0"])
@pytest.mark.parametrize("name", SMALL)
def test_narrow_k3_k5(gpu, monkeypatch, name, cells):
    """K3 / K5 (cells=1: the streaming k_cell_s on the FC_DEEP cells -- none in `plus` and the tiny splits -- and
    k_div_cells / k_correct_cells on the rest; 0: the thread-per-cell kernels)."""
    monkeypatch.setenv("NSGPU_MASK_CELL", cells)
    rng = np.random.default_rng(22)
    dt = 1.0 / 512
    og, gs, m = pair(gpu, name, dt, 100.0)
    (us, vs, phi), arms = fill(rng, name, og, m, 3)
    gs.set(gpu.NS_ARR_U, plane(m, us)); gs.set(gpu.NS_ARR_V, plane(m, vs))
    sums = gs.kernel(gpu.NS_K_DIV)
    ref = og.divergence(dt, us, vs)
    got = gs.get(gpu.NS_ARR_RPHI).ravel()[m]
    for arm in arms:
        err = rel(got[arm], ref[arm])
        assert err <= 1e-12, err
    assert abs(sums[0] - ref.sum()) <= 1e-9 * np.abs(ref).sum()
    gs.set(gpu.NS_ARR_PHI, plane(m, phi))
    mm = gs.kernel(gpu.NS_K_CORRECT)
    u, v, _, _ = og.correct(dt, us, vs, phi)
    gu, gv = gs.get(gpu.NS_ARR_U).ravel()[m], gs.get(gpu.NS_ARR_V).ravel()[m]
    for arm in arms:
        eu, ev = rel(gu[arm], u[arm]), rel(gv[arm], v[arm])
        assert eu <= 1e-12 and ev <= 1e-12, (eu, ev)
    np.testing.assert_allclose(mm[:4], [u.min(), u.max(), v.min(), v.max()], rtol=1e-12, atol=1e-15)
    assert not np.any(gs.get(gpu.NS_ARR_U).ravel()[~m]) and not np.any(gs.get(gpu.NS_ARR_RPHI).ravel()[~m])
    assert not np.any(gs.get(gpu.NS_ARR_V).ravel()[~m])


def poisson_solves(gpu, monkeypatch, name, b, rtol, phi0=None):
    """NS_K_POIS_SOLVE of the compact right-hand side b under the default (the capacitance solve) and NSGPU_CAP=0
    (BiCGStab preconditioned by the box's solve), twice each in fresh solvers: {cap: (its, res, phi plane)}, after
    the checks that hold per path -- res <= rtol, cells outside 0, the oracle's projected residual <= 1e-11, and
    the second run bit-identical (the path taken must not hang on rounding noise)."""
    out = {}
    for cap in ("1", "0"):
        monkeypatch.setenv("NSGPU_CAP", cap)
        runs = []
        for _ in range(2):
            og, gs, m = pair(gpu, name, 1e-3, 100.0, rtol=rtol)
            gs.set(gpu.NS_ARR_PHI, np.zeros(m.size) if phi0 is None else plane(m, phi0))
            gs.set(gpu.NS_ARR_RPHI, plane(m, b))
            its, res = gs.kernel(gpu.NS_K_POIS_SOLVE)[:2]
            runs.append((int(its), float(res), gs.get(gpu.NS_ARR_PHI).ravel().copy()))
            gs.close()
        its, res, phi = runs[0]
        print(f"{name}: NSGPU_CAP={cap}: its {its}, res {res:.3e}")
        assert res <= rtol, (cap, its, res)
        assert not np.any(phi[~m]), "cells outside the domain must stay 0"
        bm = demean(b)
        r = demean(bm - og.apply_poisson(phi[m]))
        rr = float(np.linalg.norm(r) / np.linalg.norm(bm))
        print(f"{name}: NSGPU_CAP={cap}: oracle-operator projected residual {rr:.3e}")
        assert rr <= 1e-11, (cap, rr)
        assert runs[1][0] == its and np.array_equal(runs[1][2], phi), (cap, its, runs[1][0])
        out[cap] = (its, res, phi)
    return og, m, out


@pytest.mark.parametrize("name", sorted(NARROW))
def test_narrow_converged_solves(gpu, monkeypatch, name):
    """Converged Helmholtz and Poisson solves at rtol 1e-12.  The Poisson solve's default is the capacitance solve on
    every NARROW shape, the multi-component ones and the bordered throat_out included: at most 2 refinements, never
    more iterations than BiCGStab with the box preconditioner (a polluted start would cost extra ones), and fewer
    where that path needs more than 2 (`plus`: 60 cells)."""
    rng = np.random.default_rng(23)
    dt, re = 1.0 / 128, 50.0
    alpha = dt / (2 * re)
    for cap in ("1", "0"):
        monkeypatch.setenv("NSGPU_CAP", cap)
        og, gs, m = pair(gpu, name, dt, re, rtol=1e-12)
        ru, rv = rng.uniform(-1, 1, og.N), rng.uniform(-1, 1, og.N)
        gs.set(gpu.NS_ARR_U, np.zeros(m.size)); gs.set(gpu.NS_ARR_V, np.zeros(m.size))
        gs.set(gpu.NS_ARR_RU, plane(m, ru)); gs.set(gpu.NS_ARR_RV, plane(m, rv))
        its, res = gs.kernel(gpu.NS_K_HELM_SOLVE)[:2]
        assert res <= 1e-12 and its > 0, (cap, its, res)
        xu, _ = og.solve_helmholtz(alpha, ru)
        u = gs.get(gpu.NS_ARR_U).ravel()
        err = rel(u[m], xu)
        assert err <= 1e-9, err
        assert not np.any(u[~m])
        gs.close()
    b = rng.uniform(-100, 100, og.N)
    og, m, out = poisson_solves(gpu, monkeypatch, name, b, 1e-12)
    xp, _ = og.solve_poisson(b)
    for cap in ("1", "0"):
        err = rel(demean(out[cap][2][m]), demean(xp))
        assert err <= 1e-8, (cap, err, out[cap][0])
    assert rel(demean(out["1"][2][m]), demean(out["0"][2][m])) <= 1e-9
    its1, its0 = out["1"][0], out["0"][0]
    assert its1 <= its0, (its1, its0)
    assert its1 <= 2, (its1, its0)                  # the capacitance solve is kept on every shape
    if NARROW_COMPONENTS[name] == 1:
        assert its1 <= 2 < its0, (its1, its0)


@pytest.mark.parametrize("rtol", [1e-11, 1e-8])
@pytest.mark.parametrize("name", SMALL)
def test_narrow_full_steps_vs_oracle(gpu, name, rtol):
    """8 steps from rest against the oracle (rtol 1e-13), test_mask_full_steps_vs_oracle's bounds."""
    P = POLY[name]
    n = max(P["xspec"][-1][2], P["yspec"][-1][2])
    steps_vs_oracle(gpu, name, 8, 1.0 / (16 * n), 200.0, rtol)


def steps_vs_oracle(gpu, name, steps, dt, re, rtol):
    og, gs, m = pair(gpu, name, dt, re, rtol=rtol)
    osv = OSolver(og, dt, re, rtol=1e-13)
    tu, tp = (1e-6, 1e-4) if rtol >= 1e-8 else (1e-9, 1e-7)
    its = []
    for _ in range(steps):
        st = gs.step()
        its.append(int(st["it_phi"]))
        assert st["it_phi"] > 0, st
        if st["phi_checked"] == 1:
            assert st["res_phi"] <= rtol, st
        mm, _ = osv.step()
        np.testing.assert_allclose([st["umin"], st["umax"], st["vmin"], st["vmax"]], mm, atol=tu)
    if rtol >= 1e-8 and all(k == 1 for k in its):
        tp = 1e-5   # (the capacitance solve, one exact iteration per step: test_mask_full_steps_vs_oracle)
    ref = osv.get()
    u, v, phi = (a.ravel() for a in gs.fields())
    du, dv = float(np.max(np.abs(u[m] - ref["u"]))), float(np.max(np.abs(v[m] - ref["v"])))
    assert du <= tu and dv <= tu, (du, dv)
    assert not np.any(u[~m]) and not np.any(v[~m]) and not np.any(phi[~m])
    p, q = demean(phi[m]), demean(ref["phi"])
    ep = float(np.linalg.norm(p - q) / np.linalg.norm(q))
    assert ep <= tp, (ep, its)
    # the last step's Poisson solve re-evaluated by the oracle's operator: P A phi = P (b - mean b) to rtol
    b = gs.get(gpu.NS_ARR_RPHI).ravel()[m]
    bm = demean(b)
    r = demean(bm - og.apply_poisson(phi[m]))
    rr = float(np.linalg.norm(r) / np.linalg.norm(bm))
    assert rr <= 1.01 * rtol + 1e-14, rr
    gs.close()


@pytest.mark.parametrize("name", ["plus", "dumbbell", "u_div1"])
def test_narrow_helmholtz_tiled_sweeps_bit_identical(gpu, monkeypatch, name):
    """test_mask_helmholtz_tiled_sweeps_bit_identical's three settings where the 32 x 64 tiles of k_helm_mt_mask are
    larger than the domain: the same fields and sweep counts bit for bit."""
    P = POLY[name]
    n = max(P["xspec"][-1][2], P["yspec"][-1][2])
    out = {}
    monkeypatch.setenv("NSGPU_MASK_BAND", "0")
    for mt, rbt in (("1", "1"), ("0", "1"), ("0", "0")):
        monkeypatch.setenv("NSGPU_MASK_MT", mt)
        monkeypatch.setenv("NSGPU_MASK_RBT", rbt)
        og, gs, m = pair(gpu, name, 1.0 / (16 * n), 200.0, rtol=1e-10)
        st = [gs.step() for _ in range(6)]
        out[mt + rbt] = ([x["it_u"] for x in st], [a.copy() for a in gs.fields()])
        gs.close()
    for k in ("11", "01"):
        assert out[k][0] == out["00"][0], (k, out[k][0], out["00"][0])
        for a, b in zip(out[k][1], out["00"][1]):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name", ["dumbbell", "throat_out"])
def test_narrow_wall_bands(gpu, monkeypatch, name):
    """test_mask_wall_bands' comparison where the bands (6 cells from a wall) cover whole lobes and throats."""
    P = POLY[name]
    n = max(P["xspec"][-1][2], P["yspec"][-1][2])
    out = {}
    for band in ("6", "0"):
        monkeypatch.setenv("NSGPU_MASK_BAND", band)
        og, gs, m = pair(gpu, name, 1.0 / (16 * n), 200.0, rtol=1e-10)
        st = [gs.step() for _ in range(6)]
        out[band] = ([x["it_u"] for x in st], [a.copy() for a in gs.fields()], st)
        gs.close()
    assert sum(out["6"][0]) <= sum(out["0"][0]), (out["6"][0], out["0"][0])
    for a, b in zip(out["6"][2], out["0"][2]):
        np.testing.assert_allclose([a[k] for k in ("umin", "umax", "vmin", "vmax")],
                                   [b[k] for k in ("umin", "umax", "vmin", "vmax")], atol=1e-9)
    u6, v6 = out["6"][1][0], out["6"][1][1]
    u0, v0 = out["0"][1][0], out["0"][1][1]
    assert float(np.max(np.abs(u6 - u0))) <= 1e-8 and float(np.max(np.abs(v6 - v0))) <= 1e-8


def _has_masked_idct(gpu, monkeypatch, capfd, name):
    """Whether this build's capacitance solve writes its solution through the masked inverse transform at this
    shape's ny: cap_setup's success line says so under NSGPU_VERBOSE (from the predicate bicgstab's direct_x uses).
    The capacitance matrix itself must have been built -- a pivot that failed k_gj_prep's test, the fall-back to
    BiCGStab, is a failure here, never a reason to skip."""
    monkeypatch.setenv("NSGPU_VERBOSE", "1")
    capfd.readouterr()
    og, gs, m = pair(gpu, name, 1e-3, 100.0)
    gs.close()
    err = capfd.readouterr().err
    monkeypatch.delenv("NSGPU_VERBOSE")
    assert "pivot failed" not in err and "BiCGStab" not in err, err
    assert "masked Poisson by the capacitance matrix" in err, err
    return "masked inverse transform" in err


@pytest.mark.parametrize("name", sorted(NARROW_TALL))
def test_narrow_masked_inverse_transform(gpu, monkeypatch, capfd, name):
    """ny = 1024: the capacitance solve's first pass writes the solution's domain cells straight into phi by the
    masked inverse transform (bicgstab's direct_x), one and two outside components.  phi's plane is pre-filled:
    ns_set_array copies the caller's plane as it is, cells outside the domain included (no masking).  Keeping those
    0 is the caller's contract -- the solves never write them, so a non-zero value put there would stay; the fill here
    covers the domain's cells only (plane()), and "outside cells are 0 after the solve" is asserted under that
    contract, for both paths.  The capacitance solve starts from zero whatever phi holds, so a domain cell
    the masked transform failed to store would keep its pre-filled value instead of the solution.  The fill is
    +- 0.05: BiCGStab (NSGPU_CAP=0) starts from it, and the residual it can reach, re-evaluated, has the floor
    eps |A| |x0| / |b| = 1.1e-16 * 4 * 1024^2 * 0.05 / 58 = 4e-13 -- under the 1e-11 asked here (a fill of 1e3 would
    put that floor at 8e-9).  Then converged_solves' assertions at rtol 1e-11 under both paths, and 3 full steps
    against the oracle."""
    if not _has_masked_idct(gpu, monkeypatch, capfd, name):
        pytest.skip("this build has no masked inverse transform for ny = 1024 (fps_idct_mask_ok)")
    rng = np.random.default_rng(24)
    P = POLY[name]
    og = OGrid(P["vertices"], P["xspec"], P["yspec"], P["bc"])
    b = rng.uniform(-100, 100, og.N)
    og, m, out = poisson_solves(gpu, monkeypatch, name, b, 1e-11, phi0=rng.uniform(-0.05, 0.05, og.N))
    xp, _ = og.solve_poisson(b)
    for cap in ("1", "0"):
        err = rel(demean(out[cap][2][m]), demean(xp))
        assert err <= 1e-8, (cap, err, out[cap][0])
    assert rel(demean(out["1"][2][m]), demean(out["0"][2][m])) <= 1e-9
    its1, its0 = out["1"][0], out["0"][0]
    assert its1 <= 2 and its1 <= its0, (its1, its0)
    if name == "lshape_1024":                       # (one outside component: test_masked_poisson_capacitance_solve's)
        assert its1 <= 2 < its0, (its1, its0)
    monkeypatch.delenv("NSGPU_CAP")
    for rtol in (1e-11, 1e-8):
        steps_vs_oracle(gpu, name, 3, 1.0 / (16 * 1024), 200.0, rtol)


def launch(tmp_path, *args, port, nproc=2):
    out = tmp_path / "r.npz"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(HERE, "mr_worker.py"),
           "--output", str(out), *args]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=150, env=dict(os.environ))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return dict(np.load(out, allow_pickle=False))


@pytest.mark.parametrize("poly,rows,port", [("dumbbell", [(0, 12), (12, 24)], 29961),
                                            ("u_div1", [(0, 10), (10, 20)], 29963)])
def test_narrow_slabs_match_single_rank(gpu, tmp_path, poly, rows, port):
    """test_masked_domain_slabs_match_single_rank's comparison with the cut through the dumbbell's 2-cell throat
    (rows 8 ... 15) and with rank 1's first row facing u_div1's divider (row 9)."""
    assert [gpu.slab_range(rows[-1][1], 2, q) for q in range(2)] == rows
    P = POLY[poly]
    og = OGrid(P["vertices"], P["xspec"], P["yspec"], P["bc"])
    steps, rtol = 5, 1e-11
    r = launch(tmp_path, "--xport", "host", "--poly", poly, "--nsteps", str(steps), "--tol", str(rtol), port=port)
    assert str(r["status"]) == "ok", r["status"]
    gs = gpu.GpuSolver(gpu.polygon(P["vertices"], og.hx, og.hy, P["bc"]), 1.0 / (8 * og.nx), 100.0, rtol=rtol,
                       device=0)
    mm = np.array([list(gs.step().values())[:7] for _ in range(steps)])
    u, v, _ = gs.fields()
    du, dv = float(np.max(np.abs(r["u"] - u))), float(np.max(np.abs(r["v"] - v)))
    assert du <= 1e-8 and dv <= 1e-8, (du, dv)
    np.testing.assert_allclose(r["mm"][:, :4], mm[:, :4], atol=1e-8)
