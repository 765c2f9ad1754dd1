"""GPU: Lagrangian tracer particles (ns_tracers_*, k_tracer) against their NumPy statement (tests/tracer_ref.py,
pinned by tests/test_tracer_ref.py).

Tolerances count arithmetic, they are not measurements: a sample is about 12 flops on values bounded by M = max|q|,
so 64 eps M; an advance adds x + dt (...), so 1e-14 (box diagonal) per step, summed over the steps.  Where two device
paths must agree (TopoRect / TopoMask, ns_step / ns_step_async, frozen particles) they agree bit for bit."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from derived_ref import DGrid
from oracle import OGrid
from polygons import ALL, NARROW, SPLITS, _cells
from tracer_ref import EXITED, LIVE, STUCK, TGrid, Tracers

pytestmark = pytest.mark.gpu
HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "navierstokessolver_amd", "host")
EPS = np.finfo(np.float64).eps
DT, RE = 1e-3, 250.0

BC_CAVITY = [(2, 0.0), (2, 1.0), (2, 0.0), (2, 0.0)]
BC_CHANNEL = [(0, 1.0), (2, 0.0), (4, 0.0), (2, 0.0)]   # inlet W, walls N / S, NEUMANN outflow E
BC_FLOW = [(0, 1.0), (2, 0.0), (0, 1.0), (2, 0.5)]      # test_gpu_derived.py's: inlet both ends, moving wall S


def lid_profile(nx):
    x = (np.arange(nx) + 0.5) / nx
    return (1 - (2 * x - 1) ** 16) ** 2


def quadrant_seeds(T):
    """Four particles per domain cell, one per quadrant, at 0.2 and 0.8 of the cell: every wall half-cell, every
    corner."""
    xs, ys = [], []
    for i, j in zip(*np.nonzero(T.G.mask)):
        for fx in (0.2, 0.8):
            for fy in (0.2, 0.8):
                xs.append(T.xf[i] + fx * (T.xf[i + 1] - T.xf[i]))
                ys.append(T.yf[j] + fy * (T.yf[j + 1] - T.yf[j]))
    return np.array(xs), np.array(ys)


def deep_seeds(T, n, rng, margin=2):
    """n random points in cells whose neighbours up to `margin` away (the whole block) are in the domain."""
    m = T.G.mask
    ok = [(i, j) for i in range(margin, T.nx - margin) for j in range(margin, T.ny - margin)
          if m[i - margin:i + margin + 1, j - margin:j + margin + 1].all()]
    pick = rng.integers(0, len(ok), n)
    fx, fy = rng.uniform(0.0, 1.0, n), rng.uniform(0.0, 1.0, n)
    xs = [T.xf[ok[k][0]] + f * (T.xf[ok[k][0] + 1] - T.xf[ok[k][0]]) for k, f in zip(pick, fx)]
    ys = [T.yf[ok[k][1]] + f * (T.yf[ok[k][1] + 1] - T.yf[ok[k][1]]) for k, f in zip(pick, fy)]
    return np.array(xs), np.array(ys)


def rect_case(gpu, nx, ny, bc, xr=-1, yr=-1, profile=None, dt=DT, re=RE, **kw):
    gs = gpu.GpuSolver(gpu.rectangle(nx, ny, bc=bc, xratio=xr, yratio=yr), dt, re, **kw)
    if profile is not None:
        gs.set_edge_profile(1, profile)
    og = OGrid.rectangle(nx, ny, bc=bc, xratio=xr, yratio=yr)
    T = TGrid(DGrid(gs.hx, gs.hy, og.id.reshape(nx, ny) >= 0, og.tag, bc, {1: profile} if profile is not None else None))
    return gs, T


def poly_case(gpu, P, dt=DT, re=RE):
    og = OGrid(P["vertices"], P["xspec"], P["yspec"], P["bc"])
    gs = gpu.GpuSolver(gpu.polygon(P["vertices"], og.hx, og.hy, P["bc"]), dt, re)
    return gs, TGrid(DGrid.from_oracle(og, P["bc"])), og


def check_sample(gs, T, u, v, xs, ys, what):
    """u, v: (nx, ny) planes.  The device's sample of every seed against the statement's, 64 eps max|q|."""
    gs.enable_tracers(xs.size)
    gs.add_tracers(xs, ys)
    su, sv = gs.sample_tracers()
    P = Tracers(T)
    P.add(xs, ys)
    ru, rv = P.sample(u, v)
    eu = np.max(np.abs(su - ru)) / np.max(np.abs(u))
    ev = np.max(np.abs(sv - rv)) / np.max(np.abs(v))
    print(f"{what}: {xs.size} seeds, sample error u {eu / EPS:.2f} v {ev / EPS:.2f} eps max|q|")
    assert eu <= 64 * EPS and ev <= 64 * EPS, (what, eu / EPS, ev / EPS)
    return P


# ------------------------------------------------------------------ 1. the sample on rectangles
RECTS = {"4x3-cavity": (4, 3, BC_CAVITY, -1, -1, False), "12x33-channel": (12, 33, BC_CHANNEL, -1, -1, False),
         "33x40s-flow": (33, 40, BC_FLOW, 1.05, 0.95, False), "40x70-cavity-profile": (40, 70, BC_CAVITY, -1, -1, True)}


@pytest.mark.parametrize("name", list(RECTS))
def test_sample_on_rectangles(gpu, name):
    nx, ny, bc, xr, yr, prof = RECTS[name]
    gs, T = rect_case(gpu, nx, ny, bc, xr, yr, lid_profile(nx) if prof else None)
    rng = np.random.default_rng(51)
    u, v = rng.uniform(-1, 1, (nx, ny)), rng.uniform(-1, 1, (nx, ny))
    gs.set_fields_compact(u=u, v=v)
    check_sample(gs, T, u, v, *quadrant_seeds(T), name)
    gs.close()


# ------------------------------------------------------------------ 2. ... and on masked polygons
MASKED = {**{k: ALL[k] for k in ("lshape", "step", "uchannel")}, **{k: NARROW[k] for k in ("plus", "u_div1", "throat_out")}}


@pytest.mark.parametrize("name", list(MASKED))
def test_sample_on_masked_polygons(gpu, name):
    gs, T, og = poly_case(gpu, MASKED[name])
    rng = np.random.default_rng(52)
    u, v = rng.uniform(-1, 1, og.N), rng.uniform(-1, 1, og.N)
    gs.set_fields_compact(u=u, v=v)
    check_sample(gs, T, T.G.plane(u), T.G.plane(v), *quadrant_seeds(T), name)
    gs.close()


# ------------------------------------------------------------------ 3. TopoRect and TopoMask agree bit for bit
FULL = {"split_5x5": SPLITS["split_5x5"],
        "split_24x20": _cells([(0, 0), (0, 10), (0, 20), (24, 20), (24, 0)], 24, 20, {2: (2, 1.0)})}


@pytest.mark.parametrize("name", list(FULL))
def test_rectangle_and_full_mask_agree_bitwise(gpu, name):
    P = FULL[name]
    gm, T, og = poly_case(gpu, P)
    assert gm.grid.cell_id is not None and T.G.mask.all()
    lx, ly = og.hx.sum(), og.hy.sum()
    gr = gpu.GpuSolver(gpu.polygon([(0, 0), (0, ly), (lx, ly), (lx, 0)], og.hx, og.hy, BC_CAVITY), DT, RE)
    assert gr.grid.cell_id is None
    rng = np.random.default_rng(53)
    u, v = rng.uniform(-1, 1, (T.nx, T.ny)), rng.uniform(-1, 1, (T.nx, T.ny))
    xs, ys = quadrant_seeds(T)
    out = []
    for gs in (gr, gm):
        gs.set_fields_compact(u=u, v=v)
        gs.enable_tracers(xs.size)
        gs.add_tracers(xs, ys)
        s0 = gs.sample_tracers()
        gs.advance_tracers(0.9 * og.hy[0], 5)   # (CFL up to 0.9: some wall half-cell seeds overshoot and stick)
        out.append((s0, gs.tracers(), gs.sample_tracers()))
        gs.close()
    (ra, rt, rb), (ma, mt, mb) = out
    assert np.array_equal(ra[0], ma[0]) and np.array_equal(ra[1], ma[1])
    for k in ("x", "y", "age", "state"):
        assert np.array_equal(rt[k], mt[k]), k
    assert all(rt[k] == mt[k] for k in ("n", "live", "exited", "stuck", "age_max"))
    assert np.array_equal(rb[0], mb[0], equal_nan=True) and np.array_equal(rb[1], mb[1], equal_nan=True)
    assert 0 < rt["stuck"] < rt["n"] and rt["live"] > 0   # (both fates took part)


# ------------------------------------------------------------------ 4. a frozen rotation field, 200 AB2 steps
def test_frozen_field_rotation(gpu):
    n, steps = 16, 200
    gs, T = rect_case(gpu, n, n, BC_CAVITY)
    X, Y = np.meshgrid(T.xc, T.yc, indexing="ij")
    u, v = -(Y - 0.5), X - 0.5
    gs.set_fields_compact(u=u, v=v)
    th = 2 * math.pi * np.arange(64) / 64
    xs, ys = 0.5 + 0.3 * np.cos(th), 0.5 + 0.3 * np.sin(th)
    gs.enable_tracers(64)
    gs.add_tracers(xs, ys)
    dt = 2 * math.pi / steps
    gs.advance_tracers(dt, steps)
    got = gs.tracers()
    gs.close()
    P = Tracers(T)
    P.add(xs, ys)
    P.advance(u, v, dt, steps)
    tol = steps * 1e-14 * math.sqrt(2.0)
    err = max(np.max(np.abs(got["x"] - P.x)), np.max(np.abs(got["y"] - P.y)))
    ce_gpu, ce_ref = np.hypot(got["x"] - xs, got["y"] - ys), np.hypot(P.x - xs, P.y - ys)
    print(f"rotation: position error {err:.2e} (allowed {tol:.2e}); closing error {ce_gpu.max():.6e} (statement {ce_ref.max():.6e})")
    assert np.all(got["state"] == LIVE) and got["live"] == 64
    assert err <= tol
    assert np.max(np.abs(ce_gpu - ce_ref)) <= tol
    assert abs(got["age_max"] - P.age.max()) <= steps * EPS * 2 * math.pi and got["age_max"] == got["age"].max()


# ------------------------------------------------------------------ 5. fates on the device
def test_fates_on_the_device(gpu):
    nx, ny = 24, 16
    hx, hy = 1.0 / nx, 1.0 / ny
    gs, T = rect_case(gpu, nx, ny, BC_CHANNEL)
    gs.enable_tracers(4 * nx * ny)
    xs, ys = quadrant_seeds(T)

    def run(u, v, dt):
        gs.reset_tracers()
        gs.set_fields_compact(u=u, v=v)
        gs.add_tracers(xs, ys)
        gs.advance_tracers(dt, 1)
        got = gs.tracers()
        P = Tracers(T)
        P.add(xs, ys)
        P.advance(u, v, dt, 1)
        assert np.array_equal(got["state"], P.state)
        # the counts are a count of the states
        for k, s in (("live", LIVE), ("exited", EXITED), ("stuck", STUCK)):
            assert got[k] == int(np.sum(got["state"] == s)), k
        assert got["n"] == xs.size and got["live"] + got["exited"] + got["stuck"] == xs.size
        dead = got["state"] != LIVE
        # a particle that is not live stayed at x^n with age 0
        assert np.array_equal(got["x"][dead], xs[dead]) and np.array_equal(got["y"][dead], ys[dead])
        assert not np.any(got["age"][dead]) and np.all(got["age"][~dead] == dt)
        # twenty more advances change nothing in it, bit for bit
        gs.advance_tracers(dt, 20)
        more = gs.tracers()
        for k in ("x", "y", "age", "state"):
            assert np.array_equal(more[k][dead], got[k][dead]), k
        assert more["exited"] >= got["exited"] and more["stuck"] >= got["stuck"]
        return got

    one, zero = np.ones((nx, ny)), np.zeros((nx, ny))
    # u = 1 (0.4 in the wall half-cells), dt = 0.7 hx: the last column's seeds at 0.8 of the cell leave through the
    # NEUMANN side, every other seed stays
    got = run(one, zero, 0.7 * hx)
    last = xs > 1.0 - 0.5 * hx
    assert np.all(got["state"][last] == EXITED) and got["exited"] == int(last.sum()) == 2 * ny and got["stuck"] == 0
    # v = -1 (-0.4 at 0.2 of the bottom cells), dt = 0.7 hy: the bottom half-cells' seeds overshoot the wall
    got = run(zero, -one, 0.7 * hy)
    # (but for the one in the inlet's corner half-cell, where the inlet's v = 0 slows it to -0.16)
    low = (ys < 0.5 * hy) & (xs > 0.5 * hx)
    assert np.all(got["state"][low] == STUCK) and got["exited"] == 0 and got["stuck"] == int(low.sum()) == 2 * nx - 1
    gs.close()


# ------------------------------------------------------------------ 6. carried by the step
def carried(gpu, mk, T, xs, ys, steps, dt):
    """ns_step with the statement advanced in the very u^n, v^n read before each step; ns_step_async bit for bit."""
    a = mk()
    a.enable_tracers(xs.size)
    a.add_tracers(xs, ys)
    P = Tracers(T)
    P.add(xs, ys)
    for _ in range(steps):
        u, v, _phi = a.fields()
        a.step()
        P.advance(u, v, dt, 1)
    got = a.tracers()
    a.close()
    tol = steps * 1e-14 * math.hypot(T.xf[-1], T.yf[-1])
    err = max(np.max(np.abs(got["x"] - P.x)), np.max(np.abs(got["y"] - P.y)))
    moved = np.max(np.hypot(got["x"] - xs, got["y"] - ys))
    print(f"carried {T.nx}x{T.ny}: {steps} steps, error {err:.2e} (allowed {tol:.2e}), largest displacement {moved:.3e}")
    assert np.array_equal(got["state"], P.state) and np.all(got["state"] == LIVE)
    assert err <= tol and moved > 0.0
    assert np.all(got["age"] == P.age) and got["live"] == xs.size and got["age_max"] == got["age"].max()
    return got


@pytest.mark.parametrize("nx,ny", [(64, 48), (96, 96), (64, 64)])
def test_carried_by_the_step(gpu, nx, ny):
    steps, dt, re = 20, 1.0 / (8 * max(nx, ny)), 400.0
    mk = lambda: gpu.GpuSolver(gpu.rectangle(nx, ny, bc=BC_CAVITY), dt, re)
    og = OGrid.rectangle(nx, ny, bc=BC_CAVITY)
    probe = mk()
    T = TGrid(DGrid(probe.hx, probe.hy, og.id.reshape(nx, ny) >= 0, og.tag, BC_CAVITY))
    probe.close()
    xs, ys = deep_seeds(T, 300, np.random.default_rng(56))
    got = carried(gpu, mk, T, xs, ys, steps, dt)
    # the deferred path's fields are bit-identical (test_deferred_correction_is_bit_identical): so are the particles
    b = mk()
    b.enable_tracers(300)
    b.add_tracers(xs, ys)
    sts = [b.step_async() for _ in range(steps)]
    gb = b.tracers()
    b.close()
    print(f"  ns_step_async: {sum(s['k5_deferred'] for s in sts)} of {steps} steps applied a deferred correction")
    if (nx, ny) == (64, 64):   # (the power-of-two cavity: the direct solve, K5 folded into the next K1)
        assert sum(s["k5_deferred"] for s in sts) >= steps - 1
    for k in ("x", "y", "age", "state"):
        assert np.array_equal(gb[k], got[k]), k


def test_carried_by_the_step_masked(gpu):
    P = ALL["lshape"]
    dt, re, steps = 1.0 / (8 * 32), 400.0, 10
    og = OGrid(P["vertices"], P["xspec"], P["yspec"], P["bc"])
    mk = lambda: gpu.GpuSolver(gpu.polygon(P["vertices"], og.hx, og.hy, P["bc"]), dt, re)
    T = TGrid(DGrid.from_oracle(og, P["bc"]))
    xs, ys = deep_seeds(T, 300, np.random.default_rng(57))
    carried(gpu, mk, T, xs, ys, steps, dt)


# ------------------------------------------------------------------ 7. tracers do not perturb the flow
COUNTS = ("n_poisson_kernels", "n_restrict_kernels", "n_helm_kernels", "n_cycle_kernels", "n_guess_kernels",
          "n_rhs_kernels", "n_fps_solves", "n_k5_kernels", "n_band_kernels")


@pytest.mark.parametrize("mode", ["step", "step_async"])
def test_tracers_do_not_perturb_the_flow(gpu, mode):
    n, dt, re, steps = 32, 1.0 / 256, 400.0, 8
    mk = lambda: gpu.GpuSolver(gpu.cavity(n), dt, re, timing=True)
    plain, empty, full = mk(), mk(), mk()
    empty.enable_tracers(100)
    full.enable_tracers(100)
    og = OGrid.rectangle(n, n, bc=BC_CAVITY)
    T = TGrid(DGrid(full.hx, full.hy, og.id.reshape(n, n) >= 0, og.tag, BC_CAVITY))
    full.add_tracers(*deep_seeds(T, 100, np.random.default_rng(58)))
    for k in range(steps):
        sts = [getattr(g, mode)() for g in (plain, empty, full)]
        for st in sts[1:]:
            assert st["n_checks"] == sts[0]["n_checks"]
            assert all(st[q] == sts[0][q] for q in ("it_u", "it_phi", "k5_deferred") + COUNTS), (k, st, sts[0])
            if mode == "step" or k > 0:
                assert all(st[q] == sts[0][q] for q in ("umin", "umax", "vmin", "vmax"))
        # the interval recorder: nothing for an empty set, exactly one particle kernel per step otherwise
        te, tf = empty.tracer_stats(), full.tracer_stats()
        assert te["n_kernels"] == 0 and te["t_kernel_ms"] == 0.0 and te["n"] == 0
        assert tf["n_kernels"] == 1 and tf["t_kernel_ms"] > 0.0 and tf["live"] == 100
    if mode == "step_async":   # (ns_step returned its own monitor, compared above; the deferred one waits here)
        mon = [g.monitor() for g in (plain, empty, full)]
        assert mon[0] == mon[1] == mon[2]
    fa = plain.fields()
    for g in (empty, full):
        for x, y in zip(fa, g.fields()):
            assert np.array_equal(x, y), "tracers changed a field"
    for g in (plain, empty, full):
        g.close()


# ------------------------------------------------------------------ 8. streaklines: adding between steps
def test_streaklines(gpu):
    n, dt, re = 32, 1.0 / 256, 400.0
    gs, T = rect_case(gpu, n, n, BC_CAVITY, dt=dt, re=re)
    for _ in range(3):
        gs.step()   # (a flow to be carried by)
    gs.enable_tracers(50)
    x0 = np.full(10, 0.5)
    y0 = 0.975 + 0.002 * np.arange(10)   # in the top row of cells, which the lid drags along
    for k in range(5):
        gs.add_tracers(x0, y0)
        if k == 4:
            wu, wv = gs.sample_tracers()
        gs.step()
    got = gs.tracers()
    gs.close()
    assert got["n"] == 50 and np.all(got["state"] == LIVE)
    # stable indices: group k sits at [10 k, 10 k + 10) and is 5 - k steps old (dt = 2^-8: the sums are exact)
    assert np.array_equal(got["age"], np.repeat(dt * np.arange(5, 0, -1), 10))
    # the particles added last took one Euler step in the field they were sampled in
    assert np.array_equal(got["x"][40:], x0 + dt * wu[40:]) and np.array_equal(got["y"][40:], y0 + dt * wv[40:])
    assert np.all(wu[40:] > 0.0)
    # the older groups are further along the streak
    assert np.all(got["x"][:10] > got["x"][40:])


# ------------------------------------------------------------------ 9. refusals
def test_refusals(gpu, monkeypatch):
    L = gpu._lib
    lib = L.lib()
    err = lambda: lib.ns_last_error().decode()
    dp = ctypes.POINTER(ctypes.c_double)
    one = (ctypes.c_double * 1)(0.5)
    st = L.NsTracerStats()
    assert lib.ns_tracers_enable(None, 10) == L.NS_EINVAL and "null solver" in err()
    assert lib.ns_tracers_last(None, ctypes.byref(st)) == L.NS_EINVAL and "null solver" in err()
    gs = gpu.GpuSolver(gpu.polygon(ALL["lshape"]["vertices"], np.full(32, 1 / 32), np.full(32, 1 / 32), ALL["lshape"]["bc"]),
                       DT, RE)
    for call in (lambda: gs.add_tracers([0.25], [0.25]), gs.tracers, gs.tracer_stats, gs.sample_tracers,
                 lambda: gs.advance_tracers(DT, 1), gs.reset_tracers):
        with pytest.raises(gpu.NsError, match="tracers are not enabled"):
            call()
    for cap in (0, -3):
        with pytest.raises(gpu.NsError, match=f"capacity {cap} is not positive"):
            gs.enable_tracers(cap)
    gs.enable_tracers(4)
    with pytest.raises(gpu.NsError, match="already enabled"):
        gs.enable_tracers(4)
    gs.add_tracers([0.25, 0.3], [0.25, 0.8])
    with pytest.raises(gpu.NsError, match="3 seeds on top of 2 exceed the capacity 4"):
        gs.add_tracers([0.25] * 3, [0.25] * 3)
    with pytest.raises(gpu.NsError, match=r"seed 1 \(nan, 0.25\) is not finite"):
        gs.add_tracers([0.25, float("nan")], [0.25, 0.25])
    with pytest.raises(gpu.NsError, match=r"seed 1 \(inf, 0.25\) is not finite"):
        gs.add_tracers([0.25, float("inf")], [0.25, 0.25])
    with pytest.raises(gpu.NsError, match=r"seed 0 \(0.75, 0.25\) is not in a domain cell"):   # the L's missing quadrant
        gs.add_tracers([0.75], [0.25])
    with pytest.raises(gpu.NsError, match=r"seed 1 \(1, 0.25\) is not in a domain cell"):      # the box's end is outside
        gs.add_tracers([0.25, 1.0], [0.25, 0.25])
    with pytest.raises(gpu.NsError, match=r"seed 0 \(-1e-09, 0.25\) is not in a domain cell"):
        gs.add_tracers([-1e-9], [0.25])
    assert gs.tracer_stats()["n"] == 2   # (all or nothing)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(gpu.NsError, match="dt = .* is not finite"):
            gs.advance_tracers(bad, 1)
    with pytest.raises(gpu.NsError, match="steps = -1 is negative"):
        gs.advance_tracers(DT, -1)
    for first, n in ((0, 3), (2, 1), (-1, 1), (3, 0)):
        with pytest.raises(gpu.NsError, match=r"is outside \[0, 2\)"):
            gs.tracers(first, n)
    assert gs.tracers(2, 0)["x"].size == 0 and gs.tracers(1, 1)["x"][0] == 0.3
    # any output pointer may be NULL
    assert lib.ns_tracers_get(gs._h, 0, 2, None, None, None, None) == 0
    assert lib.ns_tracers_sample(gs._h, None, None) == 0
    gs.reset_tracers()
    assert gs.tracer_stats()["n"] == 0 and gs.tracers()["x"].size == 0
    gs.close()
    # nranks > 1 (a virtual slab: rank 2 of 4 with itself as every peer)
    monkeypatch.setenv("NSGPU_RCCL_LOOPBACK", "1")
    monkeypatch.setenv("NSGPU_VIRTUAL_ITERS", "4:1")
    gv = gpu.GpuSolver(gpu.cavity(128), 1.0 / 1024, 1000.0, device=0, rank=2, nranks=4)
    with pytest.raises(gpu.NsError, match="ns_tracers_enable: nranks > 1 is not supported"):
        gv.enable_tracers(10)
    gv.close()


# ------------------------------------------------------------------ 10. the driver's -tracers
def test_driver_tracers(gpu, tmp_path):
    n, steps, save = 32, 6, 3
    dt = 1.0 / (8 * n)
    (tmp_path / "grid").write_text(f"Vertices {{\n0 0\n0 1\n1 1\n1 0\n}}\nNx {{\n0 1 {n} -1\n}}\nNy {{\n0 1 {n} -1\n}}\n")
    (tmp_path / "sim").write_text(f"BC {{\n2 0\n2 1\n2 0\n2 0\n}}\ndt {dt!r}\nfinal_time {steps * dt!r}\nre 100.0\nsaveIter {save}\n")
    rng = np.random.default_rng(59)
    xs, ys = rng.uniform(0.1, 0.9, 40), rng.uniform(0.6, 0.98, 40)
    (tmp_path / "seeds.csv").write_text("x,y\n" + "".join(f"{float(x)!r},{float(y)!r}\n" for x, y in zip(xs, ys)))
    exe = os.path.join(HOST, "ns_main")
    run = lambda d, *opt: subprocess.run([exe, *opt, "../grid", "../sim"], capture_output=True, text=True, cwd=d,
                                         timeout=120).stdout
    (tmp_path / "with").mkdir(); (tmp_path / "without").mkdir()
    out1 = run(tmp_path / "with", "-tracers", "../seeds.csv")
    out0 = run(tmp_path / "without")
    assert "Solution Complete!" in out1 and "Solution Complete!" in out0
    assert not list((tmp_path / "without").glob("Tracers_*"))
    extra = [l for l in out1.splitlines() if l.startswith("tracers:")]
    assert len(extra) == 1 and out1.splitlines()[-2] == extra[0], out1
    assert [l for l in out1.splitlines() if not l.startswith("tracers:")] == out0.splitlines()
    # the same run through the Python handle
    gs = gpu.GpuSolver(gpu.cavity(n), dt, 100.0)
    gs.enable_tracers(40)
    gs.add_tracers(xs, ys)
    for it in range(1, steps + 1):
        gs.step()
        if it % save:
            continue
        got = gs.tracers()
        f = tmp_path / "with" / f"Tracers_{it}.csv"
        assert f.read_text().splitlines()[0] == "id,x,y,age,state"
        d = np.loadtxt(f, delimiter=",", skiprows=1)
        assert d.shape == (40, 5) and np.array_equal(d[:, 0], np.arange(40)) and np.array_equal(d[:, 4], got["state"])
        # printed with 15 significant digits from the same doubles: equal to a unit of the last printed digit
        for c, k in ((1, "x"), (2, "y"), (3, "age")):
            assert np.all(np.abs(d[:, c] - got[k]) <= 1e-14 * np.abs(got[k])), k
    w = extra[0].split()
    assert w[1::2] == ["n", "live", "exited", "stuck", "age_max"]
    assert [int(x) for x in w[2:9:2]] == [got[k] for k in ("n", "live", "exited", "stuck")]
    assert abs(float(w[10]) - got["age_max"]) <= 1e-9 * got["age_max"]
    gs.close()
