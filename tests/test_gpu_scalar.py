"""GPU: the passive scalar carried by the time step (ns_scalar_*, k_rhs_t) against its NumPy
restatement (tests/scalar_ref.py) and the oracle's Helmholtz solve.

Tolerances are test_gpu_parity.py's: 1e-12 relative (to max |reference|) for a single kernel,
1e-9 for a solve converged to rtol 1e-11, 1e-6 absolute for full steps at rtol 1e-8.  The
streaming kernel and its thread-per-cell form (NSGPU_CELL=grid) must agree bit for bit."""
import numpy as np
import pytest

from oracle import OGrid
from polygons import LSHAPE
from scalar_ref import (IDENTITY_CASES, identity_inputs, identity_oracle, oracle_bc_of, sbc_of_ghosts, scalar_ghosts,
                        scalar_rhs, velocity_ghosts)

pytestmark = pytest.mark.gpu

WALLS = [(2, 0.0), (2, 0.0), (2, 0.0), (2, 0.0)]
BC_CAVITY = [(2, 0.0), (2, 1.0), (2, 0.0), (2, 0.0)]
BC_FLOW = [(0, 1.0), (2, 0.0), (0, 1.0), (2, 0.5)]      # inlet W, inlet-as-outlet E, moving wall S (no NEUMANN side)
BC_CHANNEL = [(0, 1.0), (2, 0.0), (4, 0.0), (2, 0.0)]   # inlet W, walls N / S, NEUMANN outflow E
# the scalar's conditions per edge (W, N, E, S)
S_CAVITY = [("zerograd",), ("dirichlet", 1.0), ("zerograd",), ("dirichlet", 0.0)]   # hot lid, cold floor
S_CHANNEL = [("dirichlet", 1.0), ("zerograd",), ("zerograd",), ("zerograd",)]       # hot inlet, outflow E
S_ADIABATIC = [("zerograd",)] * 4
S_MIXED = [("dirichlet", -0.5), ("zerograd",), ("dirichlet", 0.75), ("dirichlet", 0.25)]


def rel(a, b):
    return np.max(np.abs(np.asarray(a).ravel() - np.asarray(b).ravel())) / max(np.max(np.abs(b)), 1e-300)


def solver(nsa, nx, ny, bc, sbc, dt, re, pe, xr=-1, yr=-1, **kw):
    gs = nsa.GpuSolver(nsa.rectangle(nx, ny, bc=bc, xratio=xr, yratio=yr), dt, re, **kw)
    gs.enable_scalar(pe, sbc)
    return gs


def load(nsa, gs, u, v, T, c0):
    gs.set(nsa.NS_ARR_U, u)
    gs.set(nsa.NS_ARR_V, v)
    gs.set_scalar(T, c0)


# ------------------------------------------------------------------ 2. the RHS kernel against the restatement
# 4x3: all ring; 12x33: odd ny; 40x70: ny no multiple of 64 / 128; 21x130: ld 256, a second column strip with two
# live columns; 130x16: more than one row strip; 40x70 stretched
SHAPES = [(4, 3, -1, -1), (12, 33, -1, -1), (40, 70, -1, -1), (21, 130, -1, -1), (130, 16, -1, -1),
          (40, 70, 1.05, 0.95)]
BCSETS = {"cavity": (BC_CAVITY, S_CAVITY), "channel": (BC_CHANNEL, S_CHANNEL), "adiabatic": (WALLS, S_ADIABATIC)}


@pytest.mark.parametrize("name", list(BCSETS))
@pytest.mark.parametrize("nx,ny,xr,yr", SHAPES, ids=[f"{a}x{b}{'s' if c > 0 else ''}" for a, b, c, _ in SHAPES])
def test_rhs_kernel_vs_restatement(gpu, monkeypatch, nx, ny, xr, yr, name):
    bc, sbc = BCSETS[name]
    if name == "channel" and min(nx, ny) < 12:
        bc = BC_FLOW   # (the 4 x 3 grid: the channel's scalar sides over velocity sides without a NEUMANN one)
    rng = np.random.default_rng(21)
    dt, re, pe = 1e-3, 250.0, 71.0
    u, v, T, c0 = (rng.uniform(-1, 1, (nx, ny)) for _ in range(4))
    out = {}
    for mode in ("stream", "grid"):
        if mode == "grid":
            monkeypatch.setenv("NSGPU_CELL", "grid")
        else:
            monkeypatch.delenv("NSGPU_CELL", raising=False)
        gs = solver(gpu, nx, ny, bc, sbc, dt, re, pe, xr, yr)
        load(gpu, gs, u, v, T, c0)
        b2 = gs.scalar_kernel(1)[0]
        out[mode] = (gs.scalar_rhs(), gs.scalar(cT0=True)[1], b2, gs.scalar())
        hx, hy = gs.hx.copy(), gs.hy.copy()
        gs.close()
    monkeypatch.delenv("NSGPU_CELL", raising=False)
    ugh, vgh = velocity_ghosts(bc)
    rT, cT = scalar_rhs(hx, hy, dt, pe, u, v, T, c0, ugh, vgh, scalar_ghosts(sbc))
    er, ec = rel(out["stream"][0], rT), rel(out["stream"][1], cT)
    print(f"{nx}x{ny} {name}: rT {er:.2e} cT {ec:.2e}")
    assert er <= 1e-12 and ec <= 1e-12, (er, ec)
    assert rel(out["grid"][0], rT) <= 1e-12 and rel(out["grid"][1], cT) <= 1e-12
    assert np.array_equal(out["stream"][0], out["grid"][0]), "rT: strips and thread-per-cell differ"
    assert np.array_equal(out["stream"][1], out["grid"][1]), "cT: strips and thread-per-cell differ"
    assert np.array_equal(out["stream"][3], T), "the right-hand side alone must leave T untouched"
    for mode in out:
        assert abs(out[mode][2] - np.sum(rT * rT)) <= 1e-11 * np.sum(rT * rT)


# ------------------------------------------------------------------ 3. the oracle identity through the library
@pytest.mark.parametrize("nx,ny,xr,yr,bc,comp", IDENTITY_CASES)
def test_rhs_kernel_is_the_oracles_velocity_rhs(gpu, nx, ny, xr, yr, bc, comp):
    og, dt, re, u, v, cu, cv = identity_inputs(nx, ny, xr, yr, bc, comp)
    ugh, vgh = velocity_ghosts(bc)
    gs = solver(gpu, nx, ny, bc, sbc_of_ghosts(ugh if comp == "u" else vgh), dt, re, re, xr, yr)
    load(gpu, gs, u, v, u if comp == "u" else v, cu if comp == "u" else cv)
    gs.scalar_kernel(1)
    rT, cT = gs.scalar_rhs(), gs.scalar(cT0=True)[1]
    gs.close()
    r_ref, c_ref = identity_oracle(og, dt, re, u, v, cu, cv, comp)
    print(f"{nx}x{ny} {comp}: rT {rel(rT, r_ref):.2e} cT {rel(cT, c_ref):.2e}")
    assert rel(rT, r_ref) <= 1e-12
    assert rel(cT, c_ref) <= 1e-12


# ------------------------------------------------------------------ 4. the converged solve
@pytest.mark.parametrize("nx,ny,xr,yr,sbc", [(24, 20, -1, -1, S_MIXED), (20, 24, 1.05, 0.95, S_ADIABATIC)],
                         ids=["mixed-24x20", "adiabatic-20x24s"])
def test_converged_solve_vs_oracle(gpu, nx, ny, xr, yr, sbc):
    rng = np.random.default_rng(22)
    dt, re, pe = 0.02, 100.0, 10.0   # dt / (2 pe h^2) ~ 0.5: a solve of tens of sweeps, not two
    gs = solver(gpu, nx, ny, WALLS, sbc, dt, re, pe, xr, yr, rtol=1e-11)
    u, v, T, c0 = (rng.uniform(-1, 1, (nx, ny)) for _ in range(4))
    load(gpu, gs, u, v, T, c0)
    gs.scalar_kernel(1)
    rT = gs.scalar_rhs()
    its, res = gs.scalar_kernel(2)
    Tn = gs.scalar()
    st = gs.scalar_stats()
    gs.close()
    og = OGrid.rectangle(nx, ny, bc=oracle_bc_of(sbc), xratio=xr, yratio=yr)
    ref, _ = og.solve_helmholtz(dt / (2 * pe), rT.ravel())
    e = rel(Tn, ref)
    print(f"{nx}x{ny}: {int(its)} sweeps, residual {res:.2e}, vs oracle {e:.2e}")
    assert res <= 1e-11 and its >= 2
    assert e <= 1e-9, e
    assert st["tmin"] == Tn.min() and st["tmax"] == Tn.max() and st["it_t"] == int(its)


# ------------------------------------------------------------------ 5. full steps
STEPS = {"cavity": (24, 20, BC_CAVITY, S_CAVITY), "channel": (32, 16, BC_CHANNEL, S_CHANNEL)}


@pytest.mark.parametrize("name", list(STEPS))
def test_full_steps(gpu, name):
    nx, ny, bc, sbc = STEPS[name]
    rng = np.random.default_rng(23)
    dt, re, pe = 1.0 / (8 * max(nx, ny)), 100.0, 71.0
    gs = solver(gpu, nx, ny, bc, sbc, dt, re, pe)
    twin = gpu.GpuSolver(gpu.rectangle(nx, ny, bc=bc), dt, re)   # the same grid without a scalar
    gs.set_scalar(rng.uniform(0, 1, (nx, ny)))
    og = OGrid.rectangle(nx, ny, bc=oracle_bc_of(sbc))
    ugh, vgh = velocity_ghosts(bc)
    worst = 0.0
    for k in range(5):
        u, v, _ = gs.fields()
        T, c0 = gs.scalar(cT0=True)
        st, st0 = gs.step(), twin.step()
        rT, cT = scalar_rhs(gs.hx, gs.hy, dt, pe, u, v, T, c0, ugh, vgh, scalar_ghosts(sbc))
        ref, _ = og.solve_helmholtz(dt / (2 * pe), rT.ravel(), x0=T.ravel(), rtol=1e-13)
        Tn, c1 = gs.scalar(cT0=True)
        d = float(np.max(np.abs(Tn.ravel() - ref)))
        worst = max(worst, d)
        assert d <= 1e-6, (k, d)
        assert rel(c1, cT) <= 1e-12
        assert st["tmin"] == Tn.min() and st["tmax"] == Tn.max()
        assert "tmin" not in st0 and "tmax" not in st0
        for a, b in zip(gs.fields(), twin.fields()):
            assert np.array_equal(a, b), "the scalar changed the velocities or phi"
        assert all(st[q] == st0[q] for q in ("umin", "umax", "vmin", "vmax", "it_u", "it_phi"))
    ss = gs.scalar_stats()
    gs.close(); twin.close()
    print(f"{name}: max|dT| {worst:.2e}, last solve {ss['it_t']} sweeps, residual {ss['res_t']:.2e}")
    assert ss["res_t"] <= 1e-8 and ss["it_t"] >= 2


# ------------------------------------------------------------------ 6. ns_step_async
def test_async_steps_match_sync(gpu):
    n = 32   # (a uniform power-of-two cavity: the async steps defer K5 into the next K1)
    rng = np.random.default_rng(24)
    T0 = rng.uniform(0, 1, (n, n))
    runs = {}
    for mode in ("sync", "async"):
        gs = solver(gpu, n, n, BC_CAVITY, S_CAVITY, 1.0 / (8 * n), 100.0, 71.0)
        gs.set_scalar(T0)
        if mode == "sync":
            sts = [gs.step() for _ in range(10)]
            last = gs.scalar_stats()
        else:
            sts = [gs.step_async() for _ in range(10)]
            gs.monitor()
            last = gs.scalar_stats()
        u, v, _ = gs.fields()
        runs[mode] = (gs.scalar(), u, v, last, sts)
        gs.close()
    assert sum(s["k5_deferred"] for s in runs["async"][4]) == 9
    for a, b, what in zip(runs["sync"][:3], runs["async"][:3], "Tuv"):
        assert np.array_equal(a, b), what
    T = runs["async"][0]
    assert runs["async"][3]["tmin"] == T.min() and runs["async"][3]["tmax"] == T.max()
    assert all(runs["async"][3][q] == runs["sync"][3][q] for q in ("tmin", "tmax", "it_t", "res_t"))


# ------------------------------------------------------------------ 7. conservation
def test_adiabatic_box_conserves_the_scalar(gpu):
    """All walls still and adiabatic: sum A (rT - T) = 0 (with cT0 = 0; the velocities zero in the cells touching a
    wall, whose face states otherwise carry a normal velocity into the wall), and the solve keeps sum A T."""
    nx, ny, dt, pe = 20, 24, 1e-3, 71.0
    rng = np.random.default_rng(25)
    gs = solver(gpu, nx, ny, WALLS, S_ADIABATIC, dt, 250.0, pe, 1.05, 0.95, rtol=1e-11)
    u, v, T = (rng.uniform(-1, 1, (nx, ny)) for _ in range(3))
    for q in (u, v):
        q[0, :] = q[-1, :] = 0.0
        q[:, 0] = q[:, -1] = 0.0
    load(gpu, gs, u, v, T, np.zeros((nx, ny)))
    A = np.outer(gs.hx, gs.hy)
    gs.scalar_kernel(1)
    rT = gs.scalar_rhs()
    gs.scalar_kernel(2)
    Tn = gs.scalar()
    gs.close()
    d1, d2 = abs(np.sum(A * (rT - T))), abs(np.sum(A * (Tn - rT)))
    print(f"conservation: RHS {d1:.2e} of {np.sum(A * np.abs(T)):.2e}, solve {d2:.2e}")
    assert d1 <= 1e-12 * np.sum(A * np.abs(T))
    assert d2 <= 1e-9 * np.sum(A * np.abs(rT))


# ------------------------------------------------------------------ 8. rejections
def test_enable_rejections(gpu, monkeypatch):
    L = gpu._lib
    gs = gpu.GpuSolver(gpu.rectangle(12, 10), 1e-3, 100.0)
    with pytest.raises(gpu.NsError, match="no scalar enabled"):
        gs.scalar()
    with pytest.raises(gpu.NsError, match="no scalar enabled"):
        gs.scalar_stats()
    with pytest.raises(gpu.NsError, match="Peclet number should be positive"):
        gs.enable_scalar(0.0, S_CAVITY)
    with pytest.raises(gpu.NsError, match="Peclet number should be positive"):
        gs.enable_scalar(-3.0, S_CAVITY)
    with pytest.raises(gpu.NsError, match="3 boundary conditions for a grid of 4 edges"):
        gs.enable_scalar(10.0, S_CAVITY[:3])
    import ctypes
    arr = (L.NsScalarBc * 4)(*[L.NsScalarBc(t, 0.0) for t in (0, 1, 7, 0)])
    desc = L.NsScalarDesc(10.0, 4, arr)
    assert L.lib().ns_scalar_enable(gs._h, ctypes.byref(desc)) == L.NS_EINVAL
    assert b"edge 2: unknown scalar boundary type 7" in L.lib().ns_last_error()
    with pytest.raises(ValueError):
        gs.enable_scalar(10.0, [("robin", 1.0)] * 4)
    assert "tmin" not in gs.step()
    gs.enable_scalar(10.0, S_CAVITY)
    with pytest.raises(gpu.NsError, match="already carries a scalar"):
        gs.enable_scalar(10.0, S_CAVITY)
    assert "tmin" in gs.step()
    gs.close()
    # a masked polygon
    h = np.full(32, 1.0 / 32)
    gm = gpu.GpuSolver(gpu.polygon(LSHAPE["vertices"], h, h, LSHAPE["bc"]), 1e-3, 100.0)
    with pytest.raises(gpu.NsError, match="masked polygon"):
        gm.enable_scalar(10.0, [("zerograd",)] * len(LSHAPE["bc"]))
    gm.close()
    # nranks > 1 (a virtual slab: rank 2 of 4 with itself as every peer)
    monkeypatch.setenv("NSGPU_RCCL_LOOPBACK", "1")
    monkeypatch.setenv("NSGPU_VIRTUAL_ITERS", "4:1")
    gv = gpu.GpuSolver(gpu.cavity(128), 1.0 / 1024, 1000.0, device=0, rank=2, nranks=4)
    with pytest.raises(gpu.NsError, match="nranks > 1"):
        gv.enable_scalar(10.0, S_CAVITY)
    gv.close()
