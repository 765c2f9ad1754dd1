"""The default step at the edges of what ns_create accepts: the deferred correction (k_rhs_sc) away from the uniform
square cavity, grids of 2 to 15 cells a side (K1's ring-only branch, wall bands wider than the grid, Thomas
recurrences over two rows, a 2-point eigenvector transform), and x-slabs of 10 to 24 rows.

Tolerances: bit identity where the project promises it (the deferred correction shares K5's corr1; async and sync
slabs); otherwise the bounds the suite already uses for the same comparison -- single kernels 1e-12 of the field's
max (test_gpu_parity.py), steps at rtol 1e-12 against the oracle's reference-faithful Krylov steps 1e-9
(test_full_steps_tight_rtol, test_direct_solve_steps_vs_reference_krylov_256), slabs against one rank 1e-9
(test_gpu_multirank.py)."""
import numpy as np
import pytest

import navierstokessolver_amd as nsa
from oracle import OGrid, OSolver
from test_gpu_multirank import launch, single

pytestmark = pytest.mark.gpu

BC_CAVITY = [(2, 0.0), (2, 1.0), (2, 0.0), (2, 0.0)]
BC_FLOW = [(0, 1.0), (2, 0.0), (0, 1.0), (2, 0.5)]   # inlet W, moving wall N, inlet-as-outlet E, moving wall S
MON = ("umin", "umax", "vmin", "vmax")


def pair(nsa, nx, ny, dt, re, bc=BC_CAVITY, xratio=-1, yratio=-1, **kw):
    og = OGrid.rectangle(nx, ny, bc=bc, xratio=xratio, yratio=yratio)
    gs = nsa.GpuSolver(nsa.rectangle(nx, ny, bc=bc, xratio=xratio, yratio=yratio), dt, re, **kw)
    return og, gs


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a).ravel() - np.asarray(b).ravel())) / max(np.max(np.abs(b)), 1e-300))


def rand(rng, n, scale=1.0):
    return scale * rng.uniform(-1, 1, n)


def bcname(bc):
    return "flow" if bc is BC_FLOW else "cavity"


# ------------------------------------------------------------------ A. the deferred correction
# (nx, ny, xratio, bc), each for one mechanism of k_rhs_sc
DEFER_GEOMS = [
    (40, 24, 1.02, BC_FLOW),      # x-stretched, non-square, inlets and moving walls
    (37, 64, 1.03, BC_CAVITY),    # x-stretched, odd nx
    (96, 120, -1, BC_CAVITY),     # mixed-radix ny
    (37, 63, -1, BC_FLOW),        # odd ny: the dense transforms; the last double2 pair's second column is padding
    (48, 124, -1, BC_CAVITY),     # ny exactly one strip (SW = 124)
    (48, 125, -1, BC_CAVITY),     # one column into a second strip
    (48, 126, -1, BC_CAVITY),     # two columns into a second strip
    (4, 16, -1, BC_CAVITY),       # ihi <= ilo: ring only
    (16, 4, -1, BC_CAVITY),       # jhi <= 2: whole-row ring
    (3, 16, -1, BC_FLOW),         # three rows
    (6, 16, 1.05, BC_CAVITY),     # two inner rows, stretched
]
DEFER_IDS = [f"{nx}x{ny}-{xr}-{bcname(bc)}" for nx, ny, xr, bc in DEFER_GEOMS]
# 4 async, a field read, 1 async, a phi write, 2 async, one sync, 3 async: every async step that follows an async step
# with nothing between them folds its predecessor's K5 into K1
DEFER_PATTERN = [0, 1, 1, 1, 0, 0, 1, 0, 0, 1, 1]


def _defer_scenario(gpu, nx, ny, xr, bc, dt, re):
    gs = gpu.GpuSolver(gpu.rectangle(nx, ny, bc=bc, xratio=xr), dt, re)
    st = [gs.step_async() for _ in range(4)]
    mid = [a.copy() for a in gs.fields()]                    # (a pending correction applied here)
    st += [gs.step_async()]
    gs.set(gpu.NS_ARR_PHI, gs.get(gpu.NS_ARR_PHI))           # (and here: the read applies it, the write keeps it so)
    st += [gs.step_async() for _ in range(2)]
    st += [gs.step()]                                        # (async -> sync)
    st += [gs.step_async() for _ in range(3)]
    last = gs.monitor()
    out = (st, mid, [a.copy() for a in gs.fields()], last)
    gs.close()
    return out


@pytest.mark.parametrize("nx,ny,xr,bc", DEFER_GEOMS, ids=DEFER_IDS)
def test_deferred_correction_edge_geometries(gpu, monkeypatch, nx, ny, xr, bc):
    """test_deferred_correction_is_bit_identical's scenario (plus a phi write between two async steps) on the grids
    k5_defer_ok also admits: x-stretched (the per-row fw / fe / hx table), mixed-radix, odd and small ny (the
    dense transforms), ny around one strip's 124 columns (the edge lanes' extra phi column), and grids without
    inner cells (the ring-only launch, its +inf min / max partials).  Against NSGPU_K5_DEFER=0: the same monitors,
    sweep counts and fields bit for bit."""
    dt, re = 1.0 / (8 * max(nx, ny)), 400.0
    monkeypatch.delenv("NSGPU_K5_DEFER", raising=False)
    sa, ma, fa, la = _defer_scenario(gpu, nx, ny, xr, bc, dt, re)
    # the gate is on for this grid: the kernel under test ran
    assert any(x["k5_deferred"] == 1 for x in sa), [x["k5_deferred"] for x in sa]
    monkeypatch.setenv("NSGPU_K5_DEFER", "0")
    sb, mb, fb, lb = _defer_scenario(gpu, nx, ny, xr, bc, dt, re)
    for x, y in zip(sa, sb):
        assert all((np.isnan(x[k]) and np.isnan(y[k])) or x[k] == y[k] for k in MON + ("it_u", "it_phi")), (x, y)
    assert la == lb
    for name, x, y in zip(("u_mid", "v_mid", "phi_mid", "u", "v", "phi"), ma + fa, mb + fb):
        assert np.array_equal(x, y), (name, float(np.max(np.abs(x - y))))
    assert [x["k5_deferred"] for x in sa] == DEFER_PATTERN, [x["k5_deferred"] for x in sa]
    assert all(x["k5_deferred"] == 0 for x in sb)


@pytest.mark.parametrize("nx,ny,xr,bc", [DEFER_GEOMS[k] for k in (0, 3, 5, 7, 8)],
                         ids=[DEFER_IDS[k] for k in (0, 3, 5, 7, 8)])
def test_deferred_correction_steps_vs_oracle(gpu, monkeypatch, nx, ny, xr, bc):
    """Bit identity with K5 only says the two GPU paths agree.  The absolute anchor: 6 async steps (5 deferred
    corrections, the last applied by the field read) at rtol 1e-12 against the oracle's reference-faithful Krylov
    steps at rtol 1e-13 -- u, v within 1e-9, test_full_steps_tight_rtol's bound for this comparison."""
    monkeypatch.delenv("NSGPU_K5_DEFER", raising=False)
    dt, re = 1.0 / (8 * max(nx, ny)), 400.0
    og, gs = pair(gpu, nx, ny, dt, re, bc, xr, rtol=1e-12)
    osv = OSolver(og, dt, re, rtol=1e-13)
    st = [gs.step_async() for _ in range(6)]
    for _ in range(6):
        osv.step()
    assert [x["k5_deferred"] for x in st] == [0, 1, 1, 1, 1, 1]
    u, v, _ = gs.fields()
    gs.close()
    ref = osv.get()
    du, dv = float(np.max(np.abs(u.ravel() - ref["u"]))), float(np.max(np.abs(v.ravel() - ref["v"])))
    print(f"{nx}x{ny}: deferred steps vs oracle max|du| {du:.2e} max|dv| {dv:.2e}")
    assert du <= 1e-9 and dv <= 1e-9, (du, dv)


# ------------------------------------------------------------------ B. tiny and odd grids
TINY = [(2, 2), (2, 3), (3, 2), (3, 3), (4, 4), (5, 4), (4, 5), (2, 9), (9, 2), (6, 6), (7, 5), (15, 15)]
TINY_GEOMS = [(nx, ny, -1, -1, bc) for nx, ny in TINY for bc in (BC_CAVITY, BC_FLOW)] + \
             [(6, 7, 1.07, 0.95, BC_CAVITY), (6, 7, 1.07, 0.95, BC_FLOW)]
TINY_IDS = [f"{nx}x{ny}-{xr}-{bcname(bc)}" for nx, ny, xr, yr, bc in TINY_GEOMS]


@pytest.mark.parametrize("nx,ny,xr,yr,bc", TINY_GEOMS, ids=TINY_IDS)
def test_tiny_grid_kernels(gpu, nx, ny, xr, yr, bc):
    """K1, K3 and K5 (test_k1_rhs_velocity, test_k3_divergence, test_k5_correct: the same random fields, seeds and
    bounds) on grids of 2 to 15 cells a side: every cell a wall cell or next to one, K1 all ring below 5 cells, the
    streaming K3 / K5 with one or two written lanes.  (The plain sum of K3: 1e-11 of sum |ref| -- at most 225 terms
    within 1e-12 each.)"""
    N = nx * ny
    # K1
    rng = np.random.default_rng(1)
    dt, re = 1e-3, 250.0
    og, gs = pair(gpu, nx, ny, dt, re, bc, xr, yr)
    u, v, phi, cu, cv = (rand(rng, N) for _ in range(5))
    for a, x in ((gpu.NS_ARR_U, u), (gpu.NS_ARR_V, v), (gpu.NS_ARR_PHI, phi), (gpu.NS_ARR_CU, cu), (gpu.NS_ARR_CV, cv)):
        gs.set(a, x)
    sums = gs.kernel(gpu.NS_K_RHS)
    gx, gy = og.grad_phi(phi)
    ru, rv, cu1, cv1 = og.rhs_velocity(dt, re, u, v, gx, gy, cu, cv)
    e1 = [rel(gs.get(a), r) for a, r in ((gpu.NS_ARR_RU, ru), (gpu.NS_ARR_RV, rv), (gpu.NS_ARR_CU, cu1),
                                         (gpu.NS_ARR_CV, cv1))]
    gs.close()
    # K3
    rng = np.random.default_rng(2)
    dt3 = 1.0 / 512
    og, gs = pair(gpu, nx, ny, dt3, 100.0, bc, xr, yr)
    u, v = rand(rng, N), rand(rng, N)
    gs.set(gpu.NS_ARR_U, u); gs.set(gpu.NS_ARR_V, v)
    sums3 = gs.kernel(gpu.NS_K_DIV)
    ref3 = og.divergence(dt3, u, v)
    e3 = rel(gs.get(gpu.NS_ARR_RPHI), ref3)
    gs.close()
    # K5
    rng = np.random.default_rng(3)
    dt5 = 1.0 / 256
    og, gs = pair(gpu, nx, ny, dt5, 100.0, bc, xr, yr)
    us, vs, phi = (rand(rng, N) for _ in range(3))
    gs.set(gpu.NS_ARR_U, us); gs.set(gpu.NS_ARR_V, vs); gs.set(gpu.NS_ARR_PHI, phi)
    mm = gs.kernel(gpu.NS_K_CORRECT)
    uc, vc, _, _ = og.correct(dt5, us, vs, phi)
    e5 = [rel(gs.get(gpu.NS_ARR_U), uc), rel(gs.get(gpu.NS_ARR_V), vc)]
    gs.close()
    print(f"{nx}x{ny}: K1 {max(e1):.2e} K3 {e3:.2e} K5 {max(e5):.2e}")
    assert max(e1) <= 1e-12, e1
    assert abs(sums[0] - np.sum(ru * ru)) <= 1e-11 * np.sum(ru * ru)
    assert e3 <= 1e-12
    assert abs(sums3[0] - ref3.sum()) <= 1e-11 * np.abs(ref3).sum()
    assert abs(sums3[1] - (ref3 * ref3).sum()) <= 1e-11 * (ref3 * ref3).sum()
    assert max(e5) <= 1e-12, e5
    np.testing.assert_allclose(mm[:4], [uc.min(), uc.max(), vc.min(), vc.max()], rtol=1e-12, atol=1e-15)


TINY_STEPS = [(2, 2, BC_CAVITY), (3, 3, BC_CAVITY), (4, 4, BC_CAVITY), (5, 7, BC_FLOW), (6, 5, BC_CAVITY),
              (8, 8, BC_FLOW), (4, 16, BC_CAVITY), (16, 4, BC_CAVITY), (3, 16, BC_FLOW), (2, 9, BC_CAVITY),
              (13, 11, BC_CAVITY)]


@pytest.mark.parametrize("nx,ny,bc", TINY_STEPS, ids=[f"{nx}x{ny}-{bcname(bc)}" for nx, ny, bc in TINY_STEPS])
def test_tiny_grid_full_steps(gpu, nx, ny, bc):
    """The default step (wall bands, RB-SOR Helmholtz passes, the direct Poisson solve -- dense transforms below 16
    columns) on grids down to 2 x 2, 6 steps at rtol 1e-12 against the oracle's reference-faithful Krylov steps at
    rtol 1e-13 (test_direct_solve_steps_vs_reference_krylov_256's comparison and bounds): the monitor within 1e-9
    at every step, u, v within 1e-9, phi modulo its mean within 1e-7 of its norm; the Poisson solve converges
    (it_phi < 200) and a checked residual is within rtol."""
    dt, re = 1.0 / (8 * max(nx, ny)), 400.0
    og, gs = pair(gpu, nx, ny, dt, re, bc, rtol=1e-12)
    osv = OSolver(og, dt, re, rtol=1e-13)
    dm = 0.0
    sts = []
    for _ in range(6):
        st = gs.step()
        mm, _ = osv.step()
        sts.append(st)
        dm = max(dm, float(np.max(np.abs(np.array([st[k] for k in MON]) - mm))))
    u, v, phi = gs.fields()
    gs.close()
    ref = osv.get()
    du, dv = float(np.max(np.abs(u.ravel() - ref["u"]))), float(np.max(np.abs(v.ravel() - ref["v"])))
    p, q = phi.ravel() - phi.mean(), ref["phi"] - ref["phi"].mean()
    ep = float(np.linalg.norm(p - q) / np.linalg.norm(q))
    print(f"{nx}x{ny}: monitor {dm:.2e} max|du| {du:.2e} max|dv| {dv:.2e} phi {ep:.2e} "
          f"it_phi {[s['it_phi'] for s in sts]} res_phi {[s['res_phi'] for s in sts]}")
    assert dm <= 1e-9, dm
    assert du <= 1e-9 and dv <= 1e-9, (du, dv)
    assert ep <= 1e-7, ep
    for st in sts:
        assert 0 < st["it_phi"] < 200, st["it_phi"]
        if st["phi_checked"] == 1:
            assert st["res_phi"] <= 1e-12, st["res_phi"]


# ------------------------------------------------------------------ C. thin slabs
# (nx, ny, ranks, rows per rank)
THIN = [
    (20, 64, 2, [10, 10]),            # the minimum
    (40, 32, 4, [10, 10, 10, 10]),    # interior ranks fed from both sides by 10-row neighbours
    (33, 64, 3, [11, 11, 11]),        # odd rows
    (25, 48, 2, [13, 12]),            # unequal; mixed-radix ny
    (39, 64, 3, [13, 13, 13]),        # the last size below 2 * HALO
    (64, 64, 4, [16, 16, 16, 16]),    # above 14, below the deep-ghost threshold
    (44, 128, 2, [22, 22]),           # the last even split without deep ghost rows
    (46, 128, 2, [24, 22]),           # (units of 2 rows: not 23 / 23 -- one slab still below the threshold)
    (47, 128, 2, [24, 23]),           # the first with deep ghost rows (every slab >= 23 rows)
]


def _rows(nx, nproc):
    return [b - a for a, b in (nsa.slab_range(nx, nproc, q) for q in range(nproc))]


def _slabs_vs_one_rank(tmp_path, nx, ny, nproc, rows, port):
    """6 steps at rtol 1e-11 on the slabs and on one rank (the environment's knobs on both):
    test_slabs_host_transport_match_single_rank's assertions; returns the slabs' sweeps per step."""
    assert _rows(nx, nproc) == rows   # (a change in ns_slab_range must not silently move the case)
    steps, rtol = 6, 1e-11
    r = launch(tmp_path, "--xport", "host", "--size", str(nx), "--size-y", str(ny), "--nsteps", str(steps),
               "--solver", str(nsa.NS_POISSON_MG), "--tol", str(rtol), nproc=nproc, port=port)
    assert str(r["status"]) == "ok", r["status"]
    u, v, phi, mm = single(nx, ny, steps, nsa.NS_POISSON_MG, rtol)
    assert r["u"].shape == u.shape
    du, dv = float(np.max(np.abs(r["u"] - u))), float(np.max(np.abs(r["v"] - v)))
    dmon = float(np.max(np.abs(r["mm"][:, :4] - mm[:, :4])))
    print(f"{nx}x{ny} on {nproc}: max|du| {du:.2e} max|dv| {dv:.2e} monitor {dmon:.2e} "
          f"it_u {r['mm'][:, 4]} / {mm[:, 4]} it_phi {r['mm'][:, 6]} / {mm[:, 6]}")
    assert du <= 1e-9 and dv <= 1e-9, (du, dv)
    np.testing.assert_allclose(r["mm"][:, :4], mm[:, :4], atol=1e-9)
    assert np.max(np.abs(r["mm"][:, 4] - mm[:, 4])) <= 2, (r["mm"][:, 4], mm[:, 4])
    one = mm[:, 6] == 1   # (the direct solve: one 'iteration' on one rank, so one on every slab)
    assert np.all(r["mm"][one, 6] == 1), (r["mm"][:, 6], mm[:, 6])
    return r["mm"][:, 4].astype(int)


@pytest.mark.parametrize("fps", [None, "0"], ids=["direct", "multigrid"])
@pytest.mark.parametrize("nx,ny,nproc,rows", THIN, ids=[f"{nx}x{ny}-{n}ranks" for nx, ny, n, _ in THIN])
def test_thin_slabs_match_single_rank(tmp_path, monkeypatch, nx, ny, nproc, rows, fps):
    """x-slabs of 10 to 24 rows (host transport, every rank on the one GPU) against one rank, 6 steps at rtol 1e-11
    -- test_slabs_host_transport_match_single_rank's assertions.  Below 23 rows the per-pass ghost-row exchanges run
    (no deep ghost rows), and below 14 to 18 (by the pass's cone) no pass has an interior to overlap its exchange
    with: it runs whole after the exchange.  Default: the direct
    Poisson solve; NSGPU_FPS=0: the multigrid (its sweep fallback where a slab cannot be coarsened)."""
    if fps is None:
        monkeypatch.delenv("NSGPU_FPS", raising=False)
    else:
        monkeypatch.setenv("NSGPU_FPS", fps)
    _slabs_vs_one_rank(tmp_path, nx, ny, nproc, rows, 29901 + 2 * THIN.index((nx, ny, nproc, rows)) + (fps is not None))


@pytest.mark.parametrize("nx,ny,nproc,rows", THIN[:5], ids=[f"{nx}x{ny}-{n}ranks" for nx, ny, n, _ in THIN[:5]])
def test_thin_slabs_take_three_sweep_passes(tmp_path, monkeypatch, nx, ny, nproc, rows):
    """Slabs of 10 to 13 rows -- thinner than 2 * HALO = 14 -- through the 3-sweep Helmholtz passes, whose 6 or 7
    ghost rows come from a neighbour that owns barely more.  With the wall bands on, these small grids (all band)
    converge in batches of 4 and 2 sweeps: pairs only.  NSGPU_HELM_BAND=0 leaves the whole solve to the global
    passes, whose batches then hold 3-sweep passes: a step with an odd sweep count had an odd batch, and an odd
    batch (3, 5 = 3 + 2 or 2 + 3, 7 = 3 + 2 + 2, ...: helm_sweeps) holds one.  The same assertions against one rank."""
    monkeypatch.delenv("NSGPU_FPS", raising=False)
    monkeypatch.setenv("NSGPU_HELM_BAND", "0")
    it_u = _slabs_vs_one_rank(tmp_path, nx, ny, nproc, rows, 29941 + THIN.index((nx, ny, nproc, rows)))
    assert any(k % 2 == 1 for k in it_u), it_u   # (a 3-sweep pass ran)


def test_thin_slabs_async_steps_match_sync(tmp_path, monkeypatch):
    """ns_step_async on two 10-row slabs: the same fields and, realigned by one call, the same monitor and
    iteration counts as ns_step, bit for bit (test_async_steps_on_slabs_match_sync at 128 x 96)."""
    monkeypatch.delenv("NSGPU_FPS", raising=False)
    assert _rows(20, 2) == [10, 10]
    args = ["--xport", "host", "--size", "20", "--size-y", "64", "--nsteps", "6", "--solver", str(nsa.NS_POISSON_MG),
            "--tol", "1e-11"]
    a = launch(tmp_path, *args, port=29931)
    b = launch(tmp_path, *args, "--async-steps", port=29933)
    assert str(a["status"]) == "ok" and str(b["status"]) == "ok", (a["status"], b["status"])
    for k in ("u", "v", "phi", "mm"):
        assert np.array_equal(a[k], b[k]), k


def test_slab_below_minimum_is_rejected_on_every_rank(tmp_path, monkeypatch):
    """19 rows on 2 ranks: 10 / 9.  ns_create refuses on BOTH ranks, naming the 9-row slab -- the rank whose own slab
    is wide enough must not go on to exchange ghost rows with a neighbour that has no solver."""
    monkeypatch.delenv("NSGPU_FPS", raising=False)
    assert _rows(19, 2) == [10, 9]
    r = launch(tmp_path, "--xport", "host", "--size", "19", "--size-y", "32", "--nsteps", "2", "--solver",
               str(nsa.NS_POISSON_MG), "--tol", "1e-11", port=29935)
    status = str(r["status"]).split("; ")
    assert len(status) == 2 and all(s.startswith("error") for s in status), status
    assert all("9 rows" in s for s in status), status
    assert set(r) == {"status"}   # (nothing ran: no fields gathered)
