"""The passive scalar's right-hand side restated in NumPy: the normative definition of what
libnsgpu.so's k_rhs_t computes ("Passive scalar").  TEST INFRASTRUCTURE ONLY.

Sides are W, E, S, N.  Arrays are (nx, ny).  *gh[side] = (neu, c): the ghost across that side is
q if neu else -q + c (c = 2 x the Dirichlet value for the scalar; the velocity ghost constants
of ConstructGhostStencils for u and v)."""
import numpy as np


def minmod(a, b):
    return (b if abs(b) < abs(a) else a) if a * b > 0 else 0.0


def scalar_rhs(hx, hy, dt, pe, u, v, T, cT0, ugh, vgh, tgh):
    nx, ny = T.shape
    def gh(tab, side, q):
        neu, c = tab[side]
        return q if neu else -q + c
    def slope(q, tab, i, j, ax):
        if ax == 0:
            h, hp, hm = hx[i], i + 1 < nx, i >= 1
            a = (q[i+1, j] - q[i, j]) * 2 / (hx[i] + hx[i+1]) if hp else (gh(tab, 1, q[i, j]) - q[i, j]) / h
            b = (q[i, j] - q[i-1, j]) * 2 / (hx[i] + hx[i-1]) if hm else (q[i, j] - gh(tab, 0, q[i, j])) / h
        else:
            h, hp, hm = hy[j], j + 1 < ny, j >= 1
            a = (q[i, j+1] - q[i, j]) * 2 / (hy[j] + hy[j+1]) if hp else (gh(tab, 3, q[i, j]) - q[i, j]) / h
            b = (q[i, j] - q[i, j-1]) * 2 / (hy[j] + hy[j-1]) if hm else (q[i, j] - gh(tab, 2, q[i, j])) / h
        return minmod(a, b)
    def states(q, tab, i, j, ax, hi):          # (lower-side, upper-side) state at the cell's lower / upper face
        h = hx[i] if ax == 0 else hy[j]
        n, k = (nx, i) if ax == 0 else (ny, j)
        s = slope(q, tab, i, j, ax)
        if hi == 0:
            r = q[i, j] - h / 2 * s
            if k >= 1:
                ii, jj = (i - 1, j) if ax == 0 else (i, j - 1)
                l = q[ii, jj] + (hx[ii] if ax == 0 else hy[jj]) / 2 * slope(q, tab, ii, jj, ax)
            else:
                l = 0.5 * (q[i, j] + gh(tab, 0 if ax == 0 else 2, q[i, j]))
            return l, r
        l = q[i, j] + h / 2 * s
        if k + 1 < n:
            ii, jj = (i + 1, j) if ax == 0 else (i, j + 1)
            r = q[ii, jj] - (hx[ii] if ax == 0 else hy[jj]) / 2 * slope(q, tab, ii, jj, ax)
        else:
            r = 0.5 * (q[i, j] + gh(tab, 1 if ax == 0 else 3, q[i, j]))
        return l, r
    flux = lambda n1, n2, t1, t2: 0.5 * (n1 * t1 + n2 * t2 - abs(n1 + n2) * (t2 - t1))
    cT, rT, hpe = np.zeros_like(T), np.zeros_like(T), 0.5 / pe
    for i in range(nx):
        for j in range(ny):
            F = []
            for ax, hi in ((0, 0), (0, 1), (1, 0), (1, 1)):
                n1, n2 = states(u if ax == 0 else v, ugh if ax == 0 else vgh, i, j, ax, hi)
                t1, t2 = states(T, tgh, i, j, ax, hi)
                F.append(flux(n1, n2, t1, t2))
            c = (F[1] - F[0]) / hx[i] + (F[3] - F[2]) / hy[j]
            tc = T[i, j]
            D0 = hpe * (tc - T[i-1, j]) * 2 / (hx[i] + hx[i-1]) if i > 0 else hpe / hx[i] * (tc - gh(tgh, 0, tc))
            D1 = hpe * (T[i+1, j] - tc) * 2 / (hx[i] + hx[i+1]) if i + 1 < nx else -hpe / hx[i] * (tc - gh(tgh, 1, tc))
            D2 = hpe * (tc - T[i, j-1]) * 2 / (hy[j] + hy[j-1]) if j > 0 else hpe / hy[j] * (tc - gh(tgh, 2, tc))
            D3 = hpe * (T[i, j+1] - tc) * 2 / (hy[j] + hy[j+1]) if j + 1 < ny else -hpe / hy[j] * (tc - gh(tgh, 3, tc))
            r = tc + 0.5 * dt * cT0[i, j] + dt * ((D1 - D0) / hx[i] + (D3 - D2) / hy[j]) - 1.5 * dt * c
            for side, bnd, h in ((0, i == 0, hx[i]), (1, i == nx - 1, hx[i]), (2, j == 0, hy[j]), (3, j == ny - 1, hy[j])):
                if bnd and not tgh[side][0]:
                    r += dt * hpe / (h * h) * tgh[side][1]
            cT[i, j], rT[i, j] = c, r
    return rT, cT


# ---- helpers shared by test_scalar_ref.py and test_gpu_scalar.py
# cavity.rectangle / OGrid.rectangle list a rectangle's edges as W, N, E, S; the tables here are W, E, S, N
EDGE_OF_SIDE = (0, 2, 3, 1)
BC_WALL, BC_INLET, BC_NEUMANN = 2, 0, 4


def velocity_ghosts(bc):
    """(ugh, vgh) of a rectangle's velocity boundary conditions bc (edge order W, N, E, S; (type, info)):
    ConstructGhostStencils' constants -- a wall's info is its tangential speed, an inlet's its normal speed."""
    ugh, vgh = [], []
    for side in range(4):
        t, info = bc[EDGE_OF_SIDE[side]]
        if t == BC_NEUMANN:
            ugh.append((1, 0.0)); vgh.append((1, 0.0))
            continue
        normal_is_x = side < 2
        c = 2.0 * info
        if t == BC_WALL:     # the tangential component
            ugh.append((0, 0.0 if normal_is_x else c)); vgh.append((0, c if normal_is_x else 0.0))
        else:                # BC_INLET: the normal component
            ugh.append((0, c if normal_is_x else 0.0)); vgh.append((0, 0.0 if normal_is_x else c))
    return ugh, vgh


def scalar_ghosts(sbc):
    """tgh of per-edge scalar conditions sbc (edge order W, N, E, S; ("dirichlet", value) / ("zerograd",))."""
    out = []
    for side in range(4):
        b = sbc[EDGE_OF_SIDE[side]]
        out.append((1, 0.0) if b[0] == "zerograd" else (0, 2.0 * b[1]))
    return out


def oracle_bc_of(sbc):
    """The oracle grid on which solve_helmholtz is the scalar's operator: Dirichlet edges WALL, zero-gradient NEUMANN."""
    return [(BC_NEUMANN, 0.0) if b[0] == "zerograd" else (BC_WALL, 0.0) for b in sbc]


def sbc_of_ghosts(gh):
    """Per-edge scalar conditions (edge order W, N, E, S) that reproduce the per-side ghost table gh."""
    side_of_edge = (0, 3, 1, 2)
    return [("zerograd",) if gh[s][0] else ("dirichlet", gh[s][1] / 2) for s in side_of_edge]


# ---- the oracle identity: with the transverse velocity component zero (its ghost constants too), the scalar
# T = u (or v), cT0 = cu0, pe = re with u's own boundary conditions is advanced by ConstructRHS_V itself
BC_CAVITY = [(2, 0.0), (2, 1.0), (2, 0.0), (2, 0.0)]
BC_WMOVES = [(2, 0.7), (2, 0.0), (2, 0.0), (2, 0.0)]       # the W wall moves: v = +0.7 on it
BC_INLET_W = [(0, 0.8), (2, 0.0), (4, 0.0), (2, 0.0)]      # u = +0.8 through W, E NEUMANN
# (nx, ny, xratio, yratio, bc, the component the scalar stands for)
IDENTITY_CASES = [(12, 10, -1, -1, BC_CAVITY, "u"), (12, 10, 1.1, 0.9, BC_CAVITY, "u"),
                  (9, 14, -1, -1, BC_WMOVES, "v"), (12, 10, -1, -1, BC_INLET_W, "u")]


def identity_inputs(nx, ny, xr, yr, bc, comp, seed=11):
    """The oracle grid, dt, re and the fields of the identity: the scalar's component random, the other zero."""
    from oracle import OGrid
    rng = np.random.default_rng(seed)
    og = OGrid.rectangle(nx, ny, bc=bc, xratio=xr, yratio=yr)
    q, c0 = rng.uniform(-1, 1, (nx, ny)), rng.uniform(-1, 1, (nx, ny))
    z = np.zeros((nx, ny))
    u, v, cu, cv = (q, z, c0, z) if comp == "u" else (z, q, z, c0)
    return og, 1e-3, 250.0, u, v, cu, cv


def identity_oracle(og, dt, re, u, v, cu, cv, comp):
    """og_rhs_velocity with grad phi = 0: (rhs, convective term) of the scalar's component as (nx, ny) arrays."""
    z = og.z()
    ru, rv, cu1, cv1 = og.rhs_velocity(dt, re, u.ravel(), v.ravel(), z, z, cu.ravel(), cv.ravel())
    shape = (og.nx, og.ny)
    return (ru.reshape(shape), cu1.reshape(shape)) if comp == "u" else (rv.reshape(shape), cv1.reshape(shape))
