"""tests/loads_ref.py -- the NumPy statement of the wall loads -- pinned to the CPU oracle by the exact discrete budgets
the scheme's boundary fluxes obey (no GPU).  Each identity is checked relative to sum A |field| with tolerance 1e-12
(the arithmetic alone gives <= 3e-14):

  viscous     every edge's info 0:  sum_cells A (L_V q) = sum over boundary faces of (ghost - q) / h ds
  flow rate   sum A div = sum of the faces' normal velocity times ds
  pressure    walls only, alpha = 0:  sum A grad phi = sum phi_cell n ds
  conduction  one Crank-Nicolson conduction step:  sum A (T1 - T0) = -(dt / 2) (H(T1) + H(T0)), H the summed
              conductive heat rate

plus the p column against og.pressure, the analytic Couette and conduction profiles, and the face list's bookkeeping."""
import math

import numpy as np
import pytest

from derived_ref import NEUMANN, WALL, DGrid
from loads_ref import SUMS, face_list, loads
from oracle import OGrid
from polygons import ALL, NARROW
from scalar_ref import oracle_bc_of

DT, RE = 1.0 / 256, 100.0
POLYS = {**ALL, **NARROW}
Q = {k: n for n, k in enumerate(SUMS)}


def ogrid(spec, bc=None):
    return OGrid(spec["vertices"], spec["xspec"], spec["yspec"], spec["bc"] if bc is None else bc)


def area(G):
    return np.outer(G.hx, G.hy)[G.mask]


@pytest.mark.parametrize("name", sorted(POLYS))
def test_viscous_and_flow_rate_budgets(name):
    sp = POLYS[name]
    bc = [(t, 0.0) for t, _ in sp["bc"]]
    og = ogrid(sp, bc)
    G = DGrid.from_oracle(og, bc)
    rng = np.random.default_rng(51)
    u, v = (rng.uniform(-1, 1, og.N) for _ in range(2))
    A = area(G)
    # re = 1: tx = (ghost - u) / h, so -fvx summed over the edges is the right-hand side; L_V q = q - (I - L_V) q
    _, S = loads(G, DT, 1.0, G.plane(u), G.plane(v), np.zeros((G.nx, G.ny)))
    for q, col in ((u, "fvx"), (v, "fvy")):
        lv = q - og.apply_helmholtz(1.0, q)
        lhs, rhs = math.fsum(A * lv), -math.fsum(S[:, Q[col]])
        err = abs(lhs - rhs) / math.fsum(A * np.abs(lv))
        print(f"{name} {col}: {err:.2e}")
        assert err <= 1e-12
    div = DT * og.divergence(DT, u, v)
    err = abs(math.fsum(A * div) - math.fsum(S[:, Q["q"]])) / math.fsum(A * np.abs(div))
    print(f"{name} q: {err:.2e}")
    assert err <= 1e-12


WALLED = sorted(n for n, sp in POLYS.items() if all(t == WALL for t, _ in sp["bc"]))


@pytest.mark.parametrize("name", WALLED)
def test_pressure_budget_on_walled_polygons(name):
    sp = POLYS[name]
    og = ogrid(sp)
    G = DGrid.from_oracle(og, sp["bc"])
    phi = np.random.default_rng(52).uniform(-1, 1, og.N)
    z = np.zeros((G.nx, G.ny))
    _, S = loads(G, 0.0, RE, z, z, G.plane(phi))          # (dt = 0: alpha = 0, P = phi)
    A = area(G)
    for g, col in zip(og.grad_phi(phi), ("fpx", "fpy")):
        err = abs(math.fsum(A * g) - math.fsum(S[:, Q[col]])) / math.fsum(A * np.abs(g))
        print(f"{name} {col}: {err:.2e}")
        assert err <= 1e-12


def test_walled_set_is_not_empty():
    assert len(WALLED) >= 5


@pytest.mark.parametrize("name", sorted(POLYS))
def test_p_column_is_the_oracles_pressure(name):
    sp = POLYS[name]
    og = ogrid(sp)
    G = DGrid.from_oracle(og, sp["bc"])
    phi = np.random.default_rng(53).uniform(-1, 1, og.N)
    z = np.zeros((G.nx, G.ny))
    faces, _ = loads(G, DT, RE, z, z, G.plane(phi))
    P = G.plane(og.pressure(DT / (2 * RE), phi))
    pmax = np.max(np.abs(P))
    for F in faces:
        want = np.array([P[i, j] for i, j, _ in F["cells"]])
        assert np.max(np.abs(F["p"] - want), initial=0.0) <= 1e-12 * pmax


@pytest.mark.parametrize("name", sorted(POLYS))
def test_every_face_once_and_the_perimeter(name):
    sp = POLYS[name]
    og = ogrid(sp)
    G = DGrid.from_oracle(og, sp["bc"])
    faces = face_list(G)
    listed = [c for F in faces for c in F["cells"]]
    want = {(int(i), int(j), k) for i, j in zip(*np.nonzero(G.mask)) for k in range(4) if G.tag[i, j, k] >= 0}
    assert len(listed) == len(set(listed)) and set(listed) == want
    for e, F in enumerate(faces):
        assert all(G.tag[i, j, k] == e for i, j, k in F["cells"])
        assert np.all(np.diff(F["s"]) > 0)
    V = sp["vertices"]
    perimeter = sum(abs(V[(k + 1) % len(V)][0] - V[k][0]) + abs(V[(k + 1) % len(V)][1] - V[k][1]) for k in range(len(V)))
    assert abs(sum(F["ds"].sum() for F in faces) - perimeter) <= 1e-12 * perimeter
    # each edge's own length too
    for k, F in enumerate(faces):
        a, b = V[k], V[(k + 1) % len(V)]
        assert abs(F["ds"].sum() - (abs(b[0] - a[0]) + abs(b[1] - a[1]))) <= 1e-12 * perimeter


@pytest.mark.parametrize("nx,ny,xr,yr", [(12, 9, -1, -1), (17, 20, 1.05, 0.95)])
def test_couette(nx, ny, xr, yr):
    U, lx = 0.75, 2.0
    bc = [(2, 0.0), (2, U), (2, 0.0), (2, 0.0)]           # edges W, N (the lid), E, S
    og = OGrid.rectangle(nx, ny, lx=lx, bc=bc, xratio=xr, yratio=yr)
    G = DGrid.from_oracle(og, bc)
    yc = np.cumsum(og.hy) - 0.5 * og.hy
    u = np.tile(U * yc, (nx, 1))
    z = np.zeros((nx, ny))
    _, S = loads(G, DT, RE, u, z, z)
    want = U * lx / RE
    assert abs(S[1, Q["fvx"]] + want) <= 1e-13 * want     # the lid drags the fluid along: the fluid pulls it back
    assert abs(S[3, Q["fvx"]] - want) <= 1e-13 * want
    assert not np.any(S[:, Q["fvy"]]) and not np.any(S[:, Q["q"]])


@pytest.mark.parametrize("nx,ny,xr,yr", [(12, 9, -1, -1), (17, 20, 1.05, 0.95)])
def test_conduction_profile(nx, ny, xr, yr):
    pe, ly = 40.0, 1.5
    bc = [(2, 0.0)] * 4
    sbc = [("dirichlet", 1.0), ("zerograd",), ("dirichlet", 0.0), ("zerograd",)]   # W = 1, N, E = 0, S
    og = OGrid.rectangle(nx, ny, ly=ly, bc=bc, xratio=xr, yratio=yr)
    G = DGrid.from_oracle(og, bc)
    xc = np.cumsum(og.hx) - 0.5 * og.hx
    T = np.tile((1.0 - xc)[:, None], (1, ny))
    z = np.zeros((nx, ny))
    _, S = loads(G, DT, RE, z, z, z, (pe, T, sbc))
    want = ly / pe
    assert abs(S[0, Q["heat"]] + want) <= 1e-13 * want    # heat enters through the hot wall
    assert abs(S[2, Q["heat"]] - want) <= 1e-13 * want
    assert S[1, Q["heat"]] == 0.0 and S[3, Q["heat"]] == 0.0
    assert not np.any(S[:, Q["heat_adv"]])


@pytest.mark.parametrize("nx,ny,xr,yr", [(12, 9, -1, -1), (17, 20, 1.05, 0.95)])
def test_conduction_budget_over_one_oracle_solve(nx, ny, xr, yr):
    pe, dt = 40.0, 1.0 / 64
    alpha = dt / (2 * pe)
    sbc = [("dirichlet", 1.0), ("zerograd",), ("dirichlet", -0.25), ("dirichlet", 0.5)]
    bc = [(2, 0.0)] * 4
    og = OGrid.rectangle(nx, ny, bc=oracle_bc_of(sbc), xratio=xr, yratio=yr)    # (the scalar's operator as a grid)
    G = DGrid(og.hx, og.hy, np.ones((nx, ny), bool), og.tag, bc)
    T0 = np.random.default_rng(54).uniform(-1, 1, (nx, ny))
    # the Dirichlet ghosts' constant 2 value / h^2 in the boundary cells: L T = L_hom T + cb
    cb = np.zeros((nx, ny))
    cb[0, :] += 2 * sbc[0][1] / og.hx[0] ** 2
    cb[-1, :] += 2 * sbc[2][1] / og.hx[-1] ** 2
    cb[:, 0] += 2 * sbc[3][1] / og.hy[0] ** 2
    # Crank-Nicolson: (I - alpha L) T1 = (I + alpha L) T0, L_hom from the oracle's I - alpha L_hom
    rhs = 2 * T0.ravel() - og.apply_helmholtz(alpha, T0.ravel()) + 2 * alpha * cb.ravel()
    T1, _ = og.solve_helmholtz(alpha, rhs, rtol=1e-13)
    T1 = T1.reshape(nx, ny)
    z = np.zeros((nx, ny))
    H = [math.fsum(loads(G, dt, RE, z, z, z, (pe, T, sbc))[1][:, Q["heat"]]) for T in (T0, T1)]
    A = np.outer(og.hx, og.hy)
    lhs = math.fsum((A * (T1 - T0)).ravel())
    err = abs(lhs + 0.5 * dt * (H[0] + H[1])) / math.fsum((A * np.abs(T1)).ravel())
    print(f"{nx}x{ny}: conduction budget {err:.2e} (sum A dT = {lhs:.3e})")
    assert err <= 1e-12
    assert abs(lhs) > 1e-6
