"""GPU: Boussinesq buoyancy (ns_scalar_buoyancy, k_rhs_t's buoyant variant) against its formulas, the composed
reference step of tests/buoyancy_ref.py and the de Vahl Davis side-heated cavity.

Tolerances are test_gpu_scalar.py's: 1e-12 relative (to max |reference|) for a single kernel, 1e-6 absolute for
full steps at rtol 1e-8, bit identity between the strips and the thread-per-cell form (NSGPU_CELL=grid)."""
import ctypes

import numpy as np
import pytest

from buoyancy_ref import BuoyantRef

pytestmark = pytest.mark.gpu

WALLS = [(2, 0.0), (2, 0.0), (2, 0.0), (2, 0.0)]
BC_CAVITY = [(2, 0.0), (2, 1.0), (2, 0.0), (2, 0.0)]
# the scalar's conditions per edge (W, N, E, S)
S_CAVITY = [("zerograd",), ("dirichlet", 1.0), ("zerograd",), ("dirichlet", 0.0)]   # hot lid, cold floor
S_SIDE = [("dirichlet", 1.0), ("zerograd",), ("dirichlet", 0.0), ("zerograd",)]     # hot W, cold E, adiabatic N / S
MON = ("umin", "umax", "vmin", "vmax")


def rel(a, b):
    return np.max(np.abs(np.asarray(a).ravel() - np.asarray(b).ravel())) / max(np.max(np.abs(b)), 1e-300)


def solver(nsa, nx, ny, bc, sbc, dt, re, pe, xr=-1, yr=-1, buoy=None, **kw):
    gs = nsa.GpuSolver(nsa.rectangle(nx, ny, bc=bc, xratio=xr, yratio=yr), dt, re, **kw)
    gs.enable_scalar(pe, sbc)
    if buoy is not None:
        gs.set_buoyancy(**buoy)
    return gs


def state(nsa, gs):
    """u, v, phi, cu, cv, T, cT0 of a solver between steps."""
    u, v, phi = gs.fields()
    T, c0 = gs.scalar(cT0=True)
    return u, v, phi, gs.get(nsa.NS_ARR_CU), gs.get(nsa.NS_ARR_CV), T, c0


# ------------------------------------------------------------------ 1. the kernel against its formulas
# test_gpu_scalar.py's SHAPES -- 4x3: all ring; 12x33: odd ny; 40x70: ny no multiple of 64 / 128; 21x130: a second
# column strip with two live columns; 130x16: more than one row strip; 40x70 stretched
SHAPES = [(4, 3, -1, -1), (12, 33, -1, -1), (40, 70, -1, -1), (21, 130, -1, -1), (130, 16, -1, -1),
          (40, 70, 1.05, 0.95)]
FORCED = {"y": dict(by=3.25, bx=0.0, tref=0.4), "x": dict(by=0.0, bx=-1.75, tref=0.4),
          "xy": dict(by=3.25, bx=-1.75, tref=0.4)}


@pytest.mark.parametrize("forced", list(FORCED))
@pytest.mark.parametrize("nx,ny,xr,yr", SHAPES, ids=[f"{a}x{b}{'s' if c > 0 else ''}" for a, b, c, _ in SHAPES])
def test_buoyant_kernel_vs_formulas(gpu, monkeypatch, nx, ny, xr, yr, forced):
    B = FORCED[forced]
    rng = np.random.default_rng(41)
    dt, re, pe = 1e-3, 250.0, 71.0
    u, v, T, c0, ru, rv, cu, cv = (rng.uniform(-1, 1, (nx, ny)) for _ in range(8))
    planes = (gpu.NS_ARR_RU, gpu.NS_ARR_RV, gpu.NS_ARR_CU, gpu.NS_ARR_CV)
    out = {}
    for mode in ("stream", "grid"):
        if mode == "grid":
            monkeypatch.setenv("NSGPU_CELL", "grid")
        else:
            monkeypatch.delenv("NSGPU_CELL", raising=False)
        gs = solver(gpu, nx, ny, BC_CAVITY, S_CAVITY, dt, re, pe, xr, yr)
        gs.set(gpu.NS_ARR_U, u)
        gs.set(gpu.NS_ARR_V, v)
        for a, x in zip(planes, (ru, rv, cu, cv)):
            gs.set(a, x)
        # the plain right-hand side first (which = 1: no plane of the velocities' touched) ...
        gs.set_scalar(T, c0)
        gs.scalar_kernel(1)
        plain = (gs.scalar_rhs(), gs.scalar(cT0=True)[1])
        assert all(np.array_equal(gs.get(a), x) for a, x in zip(planes, (ru, rv, cu, cv)))
        # ... then the buoyant one on the same inputs
        gs.set_scalar(T, c0)
        gs.set_buoyancy(**B)
        sums = gs.scalar_kernel(3)
        out[mode] = dict(plain=plain, sums=sums, rT=gs.scalar_rhs(), cT=gs.scalar(cT0=True)[1], T=gs.scalar(),
                         u=gs.get(gpu.NS_ARR_U), v=gs.get(gpu.NS_ARR_V), f=[gs.get(a) for a in planes])
        gs.close()
    monkeypatch.delenv("NSGPU_CELL", raising=False)
    fx, fy = B["bx"] * (T - B["tref"]), B["by"] * (T - B["tref"])
    ref = [ru + (1.5 * dt) * fx, rv + (1.5 * dt) * fy, cu - fx, cv - fy]
    for mode, o in out.items():
        e = [rel(a, b) for a, b in zip(o["f"], ref)]
        print(f"{nx}x{ny} {forced} {mode}: ru {e[0]:.2e} rv {e[1]:.2e} cu {e[2]:.2e} cv {e[3]:.2e}")
        assert max(e) <= 1e-12, (mode, e)
        if B["bx"] == 0.0:
            assert np.array_equal(o["f"][0], ru) and np.array_equal(o["f"][2], cu), "x is not forced"
        if B["by"] == 0.0:
            assert np.array_equal(o["f"][1], rv) and np.array_equal(o["f"][3], cv), "y is not forced"
        assert np.array_equal(o["rT"], o["plain"][0]), "rT differs from the plain kernel's"
        assert np.array_equal(o["cT"], o["plain"][1]), "cT differs from the plain kernel's"
        assert np.array_equal(o["u"], u) and np.array_equal(o["v"], v) and np.array_equal(o["T"], T)
        for got, plane in zip(o["sums"], (o["rT"], o["f"][0], o["f"][1])):
            want = np.sum(plane * plane)
            assert abs(got - want) <= 1e-11 * want, (mode, got, want)
    for k, what in enumerate(("ru", "rv", "cu", "cv")):
        assert np.array_equal(out["stream"]["f"][k], out["grid"]["f"][k]), f"{what}: strips and thread-per-cell differ"
    assert np.array_equal(out["stream"]["rT"], out["grid"]["rT"]), "rT: strips and thread-per-cell differ"
    assert np.array_equal(out["stream"]["cT"], out["grid"]["cT"]), "cT: strips and thread-per-cell differ"


# ------------------------------------------------------------------ 2. off means off
@pytest.mark.parametrize("case", ["zero", "never", "at_tref"])
def test_off_means_off(gpu, case):
    nx, ny = 24, 20
    dt, re, pe = 1.0 / (8 * max(nx, ny)), 100.0, 71.0
    rng = np.random.default_rng(42)
    tref = 0.5
    T0 = np.full((nx, ny), tref) if case == "at_tref" else rng.uniform(0, 1, (nx, ny))
    gs = solver(gpu, nx, ny, BC_CAVITY, S_CAVITY, dt, re, pe)
    twin = solver(gpu, nx, ny, BC_CAVITY, S_CAVITY, dt, re, pe)   # the scalar alone
    if case == "zero":
        gs.set_buoyancy(0.0, 0.0, tref)
    elif case == "at_tref":
        gs.set_buoyancy(7.5, tref=tref)
    gs.set_scalar(T0)
    twin.set_scalar(T0)
    for k in range(1 if case == "at_tref" else 5):   # (T leaves tref with the first step: only that one is force-free)
        st, st0 = gs.step(), twin.step()
        for a, b, what in zip(gs.fields() + (gs.scalar(),), twin.fields() + (twin.scalar(),), ("u", "v", "phi", "T")):
            assert np.array_equal(a, b), (k, what)
        assert all(st[q] == st0[q] for q in MON + ("it_u", "tmin", "tmax")), (k, st, st0)
    gs.close(); twin.close()


# ------------------------------------------------------------------ 3. full steps against the composed reference
STEPS = {"cavity": (24, 20, -1, -1, BC_CAVITY, S_CAVITY, dict(by=4.0, bx=-1.5, tref=0.5)),
         "box-stretched": (20, 24, 1.05, 0.95, WALLS, S_SIDE, dict(by=25.0, bx=0.0, tref=0.5))}


@pytest.mark.parametrize("name", list(STEPS))
def test_full_steps_vs_composed_reference(gpu, name):
    nx, ny, xr, yr, bc, sbc, B = STEPS[name]
    rng = np.random.default_rng(43)
    dt, re, pe = 1.0 / (8 * max(nx, ny)), 100.0, 71.0
    gs = solver(gpu, nx, ny, bc, sbc, dt, re, pe, xr, yr, buoy=B)
    gs.set_scalar(rng.uniform(0, 1, (nx, ny)))
    ref = BuoyantRef(nx, ny, bc, sbc, dt, re, pe, xr=xr, yr=yr, **B)
    worst = 0.0
    for k in range(5):
        ref.load(*state(gpu, gs))   # (the reference from the GPU's own state: errors do not add up over the steps)
        st = gs.step()
        ref.step()
        u, v, _, cu, cv, T, _ = state(gpu, gs)
        d = [float(np.max(np.abs(a - b))) for a, b in ((u, ref.field("u")), (v, ref.field("v")), (T, ref.T))]
        ec = [rel(cu, ref.field("cu")), rel(cv, ref.field("cv"))]
        print(f"{name} step {k}: |du| {d[0]:.2e} |dv| {d[1]:.2e} |dT| {d[2]:.2e} cu {ec[0]:.2e} cv {ec[1]:.2e} "
              f"it_u {st['it_u']}")
        worst = max(worst, *d)
        assert max(d) <= 1e-6, (k, d)
        assert max(ec) <= 1e-12, (k, ec)
    gs.close()
    assert np.max(np.abs(ref.field("v"))) > 1e-3


# ------------------------------------------------------------------ 4. from rest
def side_heated(nsa, n=16, **kw):
    """The de Vahl Davis box in diffusive units, Ra 1e3, Pr 0.71: still walls, hot W (T = 1), cold E (T = 0)."""
    return solver(nsa, n, n, WALLS, S_SIDE, 2e-3, 1 / 0.71, 1.0, buoy=dict(by=710.0, tref=0.5), **kw)


def test_first_step_from_rest(gpu):
    """A fluid at rest: K1's ||RHS_v||^2 is exactly 0, and a Helmholtz check against it never passes -- the
    tolerance has to see the forced plane's own norm (max_iters = 200 turns the failure into an assertion)."""
    n = 16
    gs = side_heated(gpu, n, max_iters=200)
    T0 = np.repeat(1.0 - (np.arange(n) + 0.5) / n, n).reshape(n, n)   # linear in x between the Dirichlet sides
    gs.set_scalar(T0)
    ref = BuoyantRef(n, n, WALLS, S_SIDE, 2e-3, 1 / 0.71, 1.0, by=710.0, tref=0.5)
    ref.load(*state(gpu, gs))
    st = gs.step()
    ref.step()
    u, v, _ = gs.fields()
    T = gs.scalar()
    gs.close()
    d = [float(np.max(np.abs(a - b))) for a, b in ((u, ref.field("u")), (v, ref.field("v")), (T, ref.T))]
    print(f"from rest: it_u {st['it_u']} res_u {st['res_u']:.2e} res_v {st['res_v']:.2e} max|v| {np.abs(v).max():.4f} "
          f"|du| {d[0]:.2e} |dv| {d[1]:.2e} |dT| {d[2]:.2e}")
    assert st["it_u"] < 200, st["it_u"]
    assert st["res_v"] <= 1e-8, st["res_v"]
    assert np.abs(v).max() > 0.1
    assert max(d) <= 1e-6, d


# ------------------------------------------------------------------ 5. ns_step_async
def test_async_steps_match_sync(gpu):
    n = 32   # (a uniform power-of-two cavity: the async steps defer K5 into the next K1)
    rng = np.random.default_rng(44)
    T0 = rng.uniform(0, 1, (n, n))
    runs = {}
    for mode in ("sync", "async"):
        gs = solver(gpu, n, n, BC_CAVITY, S_CAVITY, 1.0 / (8 * n), 100.0, 71.0, buoy=dict(by=4.0, bx=-1.5, tref=0.5))
        gs.set_scalar(T0)
        if mode == "sync":
            sts = [gs.step() for _ in range(10)]
        else:
            sts = [gs.step_async() for _ in range(10)]
            gs.monitor()
        u, v, _ = gs.fields()
        runs[mode] = (gs.scalar(), u, v, sts)
        gs.close()
    assert sum(s["k5_deferred"] for s in runs["async"][3]) == 9
    for a, b, what in zip(runs["sync"][:3], runs["async"][:3], "Tuv"):
        assert np.array_equal(a, b), what


# ------------------------------------------------------------------ 6. restart
def test_restart_carries_the_force_history(gpu):
    nx, ny, xr, yr, bc, sbc, B = STEPS["cavity"]
    rng = np.random.default_rng(45)
    dt, re, pe = 1.0 / (8 * max(nx, ny)), 100.0, 71.0
    T0 = rng.uniform(0, 1, (nx, ny))
    straight = solver(gpu, nx, ny, bc, sbc, dt, re, pe, buoy=B)
    straight.set_scalar(T0)
    for _ in range(3):
        straight.step()
    u, v, phi, cu, cv, T, c0 = state(gpu, straight)
    fresh = solver(gpu, nx, ny, bc, sbc, dt, re, pe, buoy=B)
    fresh.set_fields_compact(u, v, phi, cu, cv)
    fresh.set_scalar(T, c0)
    for _ in range(2):
        straight.step()
        fresh.step()
    d = [float(np.max(np.abs(a - b))) for a, b in zip(state(gpu, straight), state(gpu, fresh))]
    straight.close(); fresh.close()
    print(f"restart: |du| {d[0]:.2e} |dv| {d[1]:.2e} |dT| {d[5]:.2e}")
    assert max(d[0], d[1], d[5]) <= 1e-6, d


# ------------------------------------------------------------------ 7. the side-heated cavity
def test_side_heated_cavity_de_vahl_davis(gpu):
    """Ra 1e3, Pr 0.71 on 16 x 16, 300 steps of dt 2e-3 from rest (settled by step 150): de Vahl Davis' benchmark
    gives max|u| 3.649 and max|v| 3.697 in diffusive units; the composed CPU reference on this grid ends at 3.592
    and 3.685 (1.6 % and 0.3 %).  A band of 3 %: far above any rtol-1e-8 effect, it catches a wrong sign, a wrong
    weight or a missing fold."""
    gs = side_heated(gpu, 16)
    gs.set_scalar(np.full((16, 16), 0.5))
    for _ in range(300):
        st = gs.step()
    u, v, _ = gs.fields()
    gs.close()
    mu, mv = float(np.abs(u).max()), float(np.abs(v).max())
    print(f"side-heated cavity 16x16, Ra 1e3: max|u| {mu:.4f} (3.649) max|v| {mv:.4f} (3.697), last it_u {st['it_u']}")
    assert abs(mu - 3.649) <= 0.03 * 3.649, mu
    assert abs(mv - 3.697) <= 0.03 * 3.697, mv


# ------------------------------------------------------------------ 8. rejections
def test_buoyancy_rejections(gpu):
    L = gpu._lib
    gs = gpu.GpuSolver(gpu.rectangle(12, 10), 1e-3, 100.0)
    with pytest.raises(gpu.NsError, match="no scalar enabled"):
        gs.set_buoyancy(1.0)
    gs.enable_scalar(10.0, S_CAVITY)
    assert L.lib().ns_scalar_buoyancy(gs._h, None) == L.NS_EINVAL
    assert b"null descriptor" in L.lib().ns_last_error()
    for bad in (dict(by=float("nan")), dict(by=1.0, bx=float("inf")), dict(by=1.0, tref=float("-inf"))):
        with pytest.raises(gpu.NsError, match="should be finite"):
            gs.set_buoyancy(**bad)
    desc = L.NsBuoyancyDesc(0.0, 2.0, 0.5)
    assert L.lib().ns_scalar_buoyancy(gs._h, ctypes.byref(desc)) == L.NS_OK
    with pytest.raises(gpu.NsError, match="unknown kernel 4"):
        gs.scalar_kernel(4)
    assert "tmin" in gs.step()
    gs.close()
