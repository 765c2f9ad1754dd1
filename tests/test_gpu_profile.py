"""GPU: boundary values that vary along an edge (ns_edge_profile) against the oracle stitched per column / row /
cell (tests/profile_ref.py).

Profiles are random (uniform in [0.5, 1.5], seeded), so an index slip of one cell is an O(1) error.  Tolerances
are test_gpu_parity.py's: 1e-12 relative (to max |reference|) for a kernel, 1e-6 absolute for full steps at rtol
1e-8, 1e-9 for full steps at rtol 1e-11.  A rectangle's edges are W, N, E, S = 0, 1, 2, 3."""
import numpy as np
import pytest

from oracle import OGrid
from polygons import ALL, BIG
from profile_ref import ProfiledGrid, rect_spec, velocity_step, zero_state
from scalar_ref import scalar_ghosts

pytestmark = pytest.mark.gpu

INLET, WALL, NEUMANN = 0, 2, 4
W, N, E, S = 0, 1, 2, 3
POLY = {**ALL, **BIG}


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a).ravel() - np.asarray(b).ravel())) / max(np.max(np.abs(b)), 1e-300))


def rnd(seed, n):
    return np.random.default_rng(seed).uniform(0.5, 1.5, n)


def bcset(name, nx, ny):
    """(bc, {edge: profile}) of a rectangle's boundary set."""
    if name == "x":      # W inlet profiled, E NEUMANN (4 x 3: an inlet of the same values), N and S plain walls
        p = rnd(101, ny)
        if min(nx, ny) < 12:
            return [(INLET, 1.0), (WALL, 0.0), (INLET, 1.0), (WALL, 0.0)], {W: p, E: p}
        return [(INLET, 1.0), (WALL, 0.0), (NEUMANN, 0.0), (WALL, 0.0)], {W: p}
    if name == "y":      # S and N inlets profiled, W and E still walls
        return [(WALL, 0.0), (INLET, 1.0), (WALL, 0.0), (INLET, 1.0)], {N: rnd(102, nx), S: rnd(103, nx)}
    if name == "lid":    # N wall's tangential speed profiled, the others still
        return [(WALL, 0.0), (WALL, 1.0), (WALL, 0.0), (WALL, 0.0)], {N: rnd(104, nx)}
    if name == "both":   # W inlet and N lid
        return [(INLET, 1.0), (WALL, 1.0), (INLET, 1.0), (WALL, 0.0)], {W: rnd(105, ny), N: rnd(106, nx)}
    raise KeyError(name)


class Case:
    """A grid with profiles: the GPU grid spec, the stitched reference, the domain mask."""

    def __init__(self, gpu, spec, profiles, rect=None):
        self.pg = ProfiledGrid(spec, profiles)
        self.profiles = profiles
        if rect is not None:
            nx, ny, bc, xr, yr, *lx = rect
            self.grid = gpu.rectangle(nx, ny, lx=lx[0] if lx else 1.0, bc=bc, xratio=xr, yratio=yr)
        else:
            self.grid = gpu.polygon(spec["vertices"], self.pg.base.hx, self.pg.base.hy, spec["bc"])
        self.m = self.grid.mask.ravel()

    def solver(self, gpu, dt, re, profiles=None, **kw):
        gs = gpu.GpuSolver(self.grid, dt, re, **kw)
        for e, p in (self.profiles if profiles is None else profiles).items():
            gs.set_edge_profile(e, p)
        return gs

    def plane(self, x):
        return self.pg.to_box(x).ravel()


def rect_case(gpu, nx, ny, xr, yr, name):
    bc, prof = bcset(name, nx, ny)
    return Case(gpu, rect_spec(nx, ny, bc, xr=xr, yr=yr), prof, rect=(nx, ny, bc, xr, yr))


def poly_case(gpu, name):
    P = POLY[name]
    og = OGrid(P["vertices"], P["xspec"], P["yspec"], P["bc"])
    if name in ("step", "step_big", "step_p2"):
        # edge 0: the inlet (x-normal, the upper half's columns); edge 4: the step's vertical wall, a tangential
        # profile -- two x-normal edges that share rows
        prof = {0: rnd(111, og.ny), 4: rnd(112, og.ny)}
    elif name == "lshape":
        prof = {1: rnd(113, og.nx)}          # the lid
    elif name == "uchannel":
        prof = {7: rnd(114, og.nx)}          # the y-normal inlet, on a stretched grid
    else:
        raise KeyError(name)
    return Case(gpu, P, prof)


# 4x3: all ring; 12x33: odd ny; 40x70: ny no multiple of 64 / 128; 21x130: a second column strip; 130x16: several row
# strips; 40x70 stretched (test_gpu_scalar.py's shapes)
SHAPES = [(4, 3, -1, -1), (12, 33, -1, -1), (40, 70, -1, -1), (21, 130, -1, -1), (130, 16, -1, -1),
          (40, 70, 1.05, 0.95)]
SHAPE_IDS = [f"{a}x{b}{'s' if c > 0 else ''}" for a, b, c, _ in SHAPES]
RECT_CASES = [(s, i, n) for s, i in zip(SHAPES, SHAPE_IDS) for n in ("x", "y", "lid", "both")
              if n != "both" or s[0] * s[1] <= 12 * 33]   # ("both": the reference is per cell)


def k1_check(gpu, monkeypatch, case, knobs, seed):
    rng = np.random.default_rng(seed)
    dt, re = 1e-3, 250.0
    pg = case.pg
    u, v, phi, cu, cv = (rng.uniform(-1, 1, pg.N) for _ in range(5))
    gx, gy = pg.base.grad_phi(phi)
    ref = pg.rhs_velocity(dt, re, u, v, gx, gy, cu, cv)
    plain = pg.base.rhs_velocity(dt, re, u, v, gx, gy, cu, cv)
    assert rel(plain[0], ref[0]) + rel(plain[1], ref[1]) > 1e-6   # (the profile is seen: not the edges' own values)
    for knob in knobs:
        for k, val in knob.items():
            monkeypatch.setenv(k, val)
        gs = case.solver(gpu, dt, re)
        for k in knob:
            monkeypatch.delenv(k)
        for a, x in ((gpu.NS_ARR_U, u), (gpu.NS_ARR_V, v), (gpu.NS_ARR_PHI, phi), (gpu.NS_ARR_CU, cu),
                     (gpu.NS_ARR_CV, cv)):
            gs.set(a, case.plane(x))
        sums = gs.kernel(gpu.NS_K_RHS)
        for a, r, tag in ((gpu.NS_ARR_RU, ref[0], "ru"), (gpu.NS_ARR_RV, ref[1], "rv"), (gpu.NS_ARR_CU, ref[2], "cu"),
                          (gpu.NS_ARR_CV, ref[3], "cv")):
            got = gs.get(a).ravel()
            err = rel(got[case.m], r)
            print(f"K1 {knob} {tag}: {err:.2e}")
            assert err <= 1e-12, (knob, tag, err)
            assert not np.any(got[~case.m]), "cells outside the domain must stay 0"
        s2 = float(np.sum(ref[0] * ref[0]))
        assert abs(sums[0] - s2) <= 1e-11 * s2, (knob, sums[0], s2)
        gs.close()


def k3_check(gpu, monkeypatch, case, knobs, seed):
    rng = np.random.default_rng(seed)
    dt = 1.0 / 512
    pg = case.pg
    us, vs = (rng.uniform(-1, 1, pg.N) for _ in range(2))
    ref = pg.divergence(dt, us, vs)
    # (the divergence reads a face's normal velocity: an inlet's profile is seen, a wall's tangential one must not be
    # -- the table belongs to one component)
    seen = rel(pg.base.divergence(dt, us, vs), ref)
    if any(case.pg.spec["bc"][e][0] == INLET for e in case.profiles):
        assert seen > 1e-6
    else:
        assert seen == 0.0
    for knob in knobs:
        for k, val in knob.items():
            monkeypatch.setenv(k, val)
        gs = case.solver(gpu, dt, 100.0)
        for k in knob:
            monkeypatch.delenv(k)
        gs.set(gpu.NS_ARR_U, case.plane(us))
        gs.set(gpu.NS_ARR_V, case.plane(vs))
        sums = gs.kernel(gpu.NS_K_DIV)
        got = gs.get(gpu.NS_ARR_RPHI).ravel()
        err = rel(got[case.m], ref)
        print(f"K3 {knob}: {err:.2e}")
        assert err <= 1e-12, (knob, err)
        assert not np.any(got[~case.m])
        assert abs(sums[0] - ref.sum()) <= 1e-9 * np.abs(ref).sum()
        gs.close()


# ------------------------------------------------------------------ 1. / 2. K1 and K3 on rectangles
@pytest.mark.parametrize("shape,sid,name", RECT_CASES, ids=[f"{i}-{n}" for _, i, n in RECT_CASES])
def test_k1_rectangles(gpu, monkeypatch, shape, sid, name):
    case = rect_case(gpu, *shape, name)
    k1_check(gpu, monkeypatch, case, [{}, {"NSGPU_RHS": "lds"}, {"NSGPU_RHS": "global"}], 51)


@pytest.mark.parametrize("shape,sid,name", RECT_CASES, ids=[f"{i}-{n}" for _, i, n in RECT_CASES])
def test_k3_rectangles(gpu, monkeypatch, shape, sid, name):
    case = rect_case(gpu, *shape, name)
    k3_check(gpu, monkeypatch, case, [{}, {"NSGPU_CELL": "grid"}], 52)


# ------------------------------------------------------------------ 3. the scalar's right-hand side
@pytest.mark.parametrize("nx,ny", [(12, 33), (40, 70)])
def test_scalar_rhs_sees_the_profile(gpu, monkeypatch, nx, ny):
    case = rect_case(gpu, nx, ny, -1, -1, "x")
    sbc = [("dirichlet", 1.0), ("zerograd",), ("zerograd",), ("zerograd",)]
    rng = np.random.default_rng(53)
    dt, re, pe = 1e-3, 250.0, 71.0
    u, v, T, c0 = (rng.uniform(-1, 1, (nx, ny)) for _ in range(4))
    rT, cT = case.pg.scalar_rhs(dt, pe, u, v, T, c0, scalar_ghosts(sbc))
    out = {}
    for mode in ("stream", "grid"):
        if mode == "grid":
            monkeypatch.setenv("NSGPU_CELL", "grid")
        gs = case.solver(gpu, dt, re)
        monkeypatch.delenv("NSGPU_CELL", raising=False)
        gs.enable_scalar(pe, sbc)
        gs.set(gpu.NS_ARR_U, u)
        gs.set(gpu.NS_ARR_V, v)
        gs.set_scalar(T, c0)
        gs.scalar_kernel(1)
        out[mode] = (gs.scalar_rhs(), gs.scalar(cT0=True)[1])
        gs.close()
    er, ec = rel(out["stream"][0], rT), rel(out["stream"][1], cT)
    print(f"{nx}x{ny}: rT {er:.2e} cT {ec:.2e}")
    assert er <= 1e-12 and ec <= 1e-12, (er, ec)
    assert np.array_equal(out["stream"][0], out["grid"][0]), "rT: strips and thread-per-cell differ"
    assert np.array_equal(out["stream"][1], out["grid"][1]), "cT: strips and thread-per-cell differ"


# ------------------------------------------------------------------ 4. polygons
@pytest.mark.parametrize("name", ["step", "lshape", "uchannel", "step_big"])
def test_k1_polygons(gpu, monkeypatch, name):
    k1_check(gpu, monkeypatch, poly_case(gpu, name), [{}], 54)


@pytest.mark.parametrize("name", ["step", "lshape", "uchannel"])
def test_k3_polygons(gpu, monkeypatch, name):
    k3_check(gpu, monkeypatch, poly_case(gpu, name), [{"NSGPU_MASK_CELL": "1"}, {"NSGPU_MASK_CELL": "0"}], 55)


# ------------------------------------------------------------------ 5. full steps against the composed reference
def run_steps(gpu, case, dt, re, steps, rtol, scale=None):
    gs = case.solver(gpu, dt, re, rtol=rtol)
    for k in range(steps):
        if scale is not None:
            for e, p in case.profiles.items():
                gs.set_edge_profile(e, scale(k) * p)
        gs.step()
    u, v, phi = (a.ravel() for a in gs.fields())
    gs.close()
    return u, v, phi


def ref_steps(case, dt, re, steps, scale=None):
    pg = case.pg
    st = zero_state(pg)
    for k in range(steps):
        if scale is not None:
            pg.set_profiles({e: scale(k) * p for e, p in case.profiles.items()})
        st = velocity_step(pg, dt, re, st, rtol=1e-13)
    return st


@pytest.fixture(scope="module")
def rect_refs():
    return {}


def rect_ref(cache, gpu, name):
    if name not in cache:
        case = rect_case(gpu, 32, 16, -1, -1, name)
        cache[name] = (case, ref_steps(case, 1.0 / 256, 100.0, 10))
    return cache[name]


@pytest.mark.parametrize("rtol", [1e-8, 1e-11])
@pytest.mark.parametrize("name,knob", [("y", {}), ("y", {"NSGPU_FPS_FUSE": "0"}), ("y", {"NSGPU_FPS": "0"}), ("x", {})],
                         ids=["y", "y-unfused", "y-multigrid", "x"])
def test_full_steps_rectangle(gpu, monkeypatch, rect_refs, name, knob, rtol):
    """32 x 16: "y" takes the direct solve with the divergence fused into its DCT (unfused / multigrid under the
    knobs), "x" the outflow elimination."""
    case, ref = rect_ref(rect_refs, gpu, name)
    for k, val in knob.items():
        monkeypatch.setenv(k, val)
    u, v, _ = run_steps(gpu, case, 1.0 / 256, 100.0, 10, rtol)
    tol = 1e-6 if rtol >= 1e-8 else 1e-9
    du, dv = float(np.max(np.abs(u - ref["u"]))), float(np.max(np.abs(v - ref["v"])))
    print(f"{name} {knob} rtol {rtol:g}: du {du:.2e} dv {dv:.2e}")
    assert du <= tol and dv <= tol, (du, dv)
    assert np.max(np.abs(ref["u"])) > 0.1


def test_fused_and_unfused_divergence_agree(gpu, monkeypatch, rect_refs):
    case, _ = rect_ref(rect_refs, gpu, "y")
    a = run_steps(gpu, case, 1.0 / 256, 100.0, 10, 1e-11)
    monkeypatch.setenv("NSGPU_FPS_FUSE", "0")
    b = run_steps(gpu, case, 1.0 / 256, 100.0, 10, 1e-11)
    for x, y in zip(a[:2], b[:2]):
        assert np.max(np.abs(x - y)) <= 1e-9


@pytest.mark.parametrize("rtol", [1e-8, 1e-11])
@pytest.mark.parametrize("name,re", [("step", 100.0), ("lshape", 400.0)])
def test_full_steps_polygons(gpu, name, re, rtol):
    case = poly_case(gpu, name)
    P = POLY[name]
    dt = 1.0 / (16 * max(P["xspec"][-1][2], P["yspec"][-1][2]))
    ref = ref_steps(case, dt, re, 10)
    u, v, _ = run_steps(gpu, case, dt, re, 10, rtol)
    tol = 1e-6 if rtol >= 1e-8 else 1e-9
    du, dv = float(np.max(np.abs(u[case.m] - ref["u"]))), float(np.max(np.abs(v[case.m] - ref["v"])))
    print(f"{name} rtol {rtol:g}: du {du:.2e} dv {dv:.2e}")
    assert du <= tol and dv <= tol, (du, dv)
    assert not np.any(u[~case.m]) and not np.any(v[~case.m])


# ------------------------------------------------------------------ 6. time dependence
def test_profile_rescaled_every_step(gpu):
    """The 32 x 16 "x" inlet profile times 1 + 0.1 sin(k) before step k."""
    case = rect_case(gpu, 32, 16, -1, -1, "x")
    scale = lambda k: 1.0 + 0.1 * np.sin(k)
    ref = ref_steps(case, 1.0 / 256, 100.0, 10, scale)
    u, v, _ = run_steps(gpu, case, 1.0 / 256, 100.0, 10, 1e-8, scale)
    du, dv = float(np.max(np.abs(u - ref["u"]))), float(np.max(np.abs(v - ref["v"])))
    print(f"du {du:.2e} dv {dv:.2e}")
    assert du <= 1e-6 and dv <= 1e-6, (du, dv)


def test_regularised_cavity_async_steps_match_sync(gpu):
    """The 32^2 regularised cavity (lid 16 x^2 (1 - x)^2 at the cell centres), the lid rescaled every step: a
    profile change between ns_step_async calls gives what it gives between ns_steps -- the deferred correction
    needs only phi."""
    n, steps = 32, 10
    x = (np.arange(n) + 0.5) / n
    lid = 16 * x ** 2 * (1 - x) ** 2
    out = {}
    for mode in ("sync", "async"):
        gs = gpu.GpuSolver(gpu.cavity(n), 1.0 / (8 * n), 100.0)
        sts = []
        for k in range(steps):
            gs.set_edge_profile(N, (1.0 + 0.1 * np.sin(k)) * lid)
            sts.append(gs.step() if mode == "sync" else gs.step_async())
        mm = gs.monitor() if mode == "async" else (sts[-1]["umin"], sts[-1]["umax"], sts[-1]["vmin"], sts[-1]["vmax"])
        out[mode] = (gs.fields(), tuple(mm), sum(int(s["k5_deferred"]) for s in sts))
        gs.close()
    for a, b, tag in zip(out["sync"][0], out["async"][0], "uvp"):
        assert np.array_equal(a, b), tag
    assert out["sync"][1] == out["async"][1]
    assert out["async"][2] == steps - 1 and out["sync"][2] == 0
    u = out["sync"][0][0]
    assert np.max(np.abs(u)) > 0.1
    # the lid's shape is seen: no corner singularity, the first column under the lid moves far less than the middle
    assert abs(u[0, -1]) < 0.1 * abs(u[n // 2, -1])


# ------------------------------------------------------------------ 7. off means off
def own_profiles(grid):
    return {e: np.full(grid.ny if ed.nx != 0 else grid.nx, ed.info) for e, ed in enumerate(grid.edges)
            if ed.type != NEUMANN}


@pytest.mark.parametrize("name", ["cavity", "lshape"])
def test_a_profile_of_the_edges_own_value_changes_nothing(gpu, name):
    if name == "cavity":
        grid, dt = gpu.rectangle(24, 20), 1.0 / 192
    else:
        P = ALL["lshape"]
        og = OGrid(P["vertices"], P["xspec"], P["yspec"], P["bc"])
        grid, dt = gpu.polygon(P["vertices"], og.hx, og.hy, P["bc"]), 1.0 / 512
    res = []
    for prof in (False, True):
        gs = gpu.GpuSolver(grid, dt, 100.0)
        if prof:
            for e, p in own_profiles(grid).items():
                gs.set_edge_profile(e, p)
        sts = [gs.step() for _ in range(5)]
        res.append((gs.fields(), [(s["umin"], s["umax"], s["vmin"], s["vmax"], s["it_u"], s["it_v"]) for s in sts]))
        gs.close()
    for a, b, tag in zip(res[0][0], res[1][0], "uvp"):
        assert np.array_equal(a, b), tag
    assert res[0][1] == res[1][1]
    assert np.max(np.abs(res[0][0][0])) > 1e-2


def test_cleared_profile_continues_as_a_restart_without_one(gpu):
    nx, ny, dt, re = 32, 16, 1.0 / 256, 100.0
    grid = gpu.rectangle(nx, ny)
    a = gpu.GpuSolver(grid, dt, re, check_every=2)   # (fixed batches: no adaptive state carried across the restart)
    a.set_edge_profile(N, rnd(121, nx))
    for _ in range(3):
        a.step()
    a.clear_edge_profile(N)
    u, v, phi = a.fields()
    cu, cv = a.get(gpu.NS_ARR_CU), a.get(gpu.NS_ARR_CV)
    b = gpu.GpuSolver(grid, dt, re, check_every=2)
    for gs in (a, b):   # both restart from the same fields
        gs.set_fields_compact(u, v, phi, cu, cv)
    for _ in range(3):
        sa, sb = a.step(), b.step()
    for x, y, tag in zip(a.fields(), b.fields(), "uvp"):
        assert np.array_equal(x, y), tag
    assert (sa["umin"], sa["umax"], sa["it_u"]) == (sb["umin"], sb["umax"], sb["it_u"])
    # (and the profile had been seen: the plain cavity from rest is elsewhere after 6 steps)
    c = gpu.GpuSolver(grid, dt, re, check_every=2)
    for _ in range(6):
        c.step()
    assert np.max(np.abs(c.fields()[0] - a.fields()[0])) > 1e-3
    for gs in (a, b, c):
        gs.close()


# ------------------------------------------------------------------ 9. the Poiseuille channel
def test_poiseuille_channel(gpu):
    """48 x 16, lx = 3: W an inlet carrying parabolic_profile's values (mean 1), E NEUMANN, Re 100, started from the
    inlet profile in every column, 100 steps.  GPU within 1e-6 of the composed reference; the outflow column
    carries the inflow as closely as the reference's does (+ 1e-6); the mid-channel column stays as close to the
    face-averaged parabola as the reference's (+ 1e-6).
    Measured: see DESIGN.md 4, "Edge profiles"."""
    nx, ny, lx, steps = 48, 16, 3.0, 100
    dt, re = 1.0 / (8 * nx), 100.0
    bc = [(INLET, 1.0), (WALL, 0.0), (NEUMANN, 0.0), (WALL, 0.0)]
    par = gpu.parabolic_profile(np.full(ny, 1.0 / ny), 0, ny, 1.0)
    case = Case(gpu, rect_spec(nx, ny, bc, lx=lx), {W: par}, rect=(nx, ny, bc, -1, -1, lx))
    grid = case.grid
    u0 = np.tile(par, (nx, 1))
    pg = case.pg
    st = zero_state(pg)
    st["u"] = u0.ravel().copy()
    for _ in range(steps):
        st = velocity_step(pg, dt, re, st, rtol=1e-13)
    gs = case.solver(gpu, dt, re)
    gs.set(gpu.NS_ARR_U, u0)
    for _ in range(steps):
        gs.step()
    u, v, _ = gs.fields()
    gs.close()
    ru, rv = st["u"].reshape(nx, ny), st["v"].reshape(nx, ny)
    du, dv = float(np.max(np.abs(u - ru))), float(np.max(np.abs(v - rv)))
    hy = grid.hy
    fg, fr = float(np.sum(u[-1] * hy)), float(np.sum(ru[-1] * hy))
    mg, mr = float(np.max(np.abs(u[nx // 2] - par))), float(np.max(np.abs(ru[nx // 2] - par)))
    print(f"du {du:.2e} dv {dv:.2e}; outflow flux gpu {fg!r} ref {fr!r} (inflow 1); mid-channel deviation from the "
          f"parabola gpu {mg:.3e} ref {mr:.3e}")
    assert du <= 1e-6 and dv <= 1e-6, (du, dv)
    assert abs(fg - 1.0) <= abs(fr - 1.0) + 1e-6
    assert mg <= mr + 1e-6


# ------------------------------------------------------------------ 10. refusals
def test_refusals(gpu):
    bc = [(INLET, 1.0), (WALL, 0.0), (NEUMANN, 0.0), (WALL, 0.0)]
    gs = gpu.GpuSolver(gpu.rectangle(16, 12, bc=bc), 1e-3, 100.0)
    with pytest.raises(gpu.NsError, match="edge 2 is a NEUMANN edge"):
        gs.set_edge_profile(E, np.ones(12))
    for e in (-1, 4):
        with pytest.raises(gpu.NsError, match=f"edge {e} of a grid with 4 edges"):
            gs.set_edge_profile(e, np.ones(12))
    with pytest.raises(gpu.NsError, match="edge 0: 16 values for an extent of 12"):
        gs.set_edge_profile(W, np.ones(16))
    with pytest.raises(gpu.NsError, match="edge 1: 12 values for an extent of 16"):
        gs.set_edge_profile(N, np.ones(12))
    bad = np.ones(12)
    bad[7] = np.nan
    with pytest.raises(gpu.NsError, match=r"edge 0: info\[7\] is not finite"):
        gs.set_edge_profile(W, bad)
    with pytest.raises(gpu.NsError, match="edge 9"):
        gs.clear_edge_profile(9)
    gs.set_edge_profile(W, np.ones(12))
    gs.clear_edge_profile(W)
    gs.clear_edge_profile(W)   # (clearing twice is fine)
    gs.step()
    gs.close()
    with pytest.raises(gpu.NsError, match="type 3"):   # NS_BC_PRESSURE stays refused
        gpu.GpuSolver(gpu.rectangle(8, 8, bc=[(3, 1.0), (2, 0.0), (2, 0.0), (2, 0.0)]), 1e-3, 100.0)
