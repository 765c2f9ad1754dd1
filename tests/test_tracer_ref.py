"""CPU: the tracers' NumPy statement (tests/tracer_ref.py) against its own properties -- exactness on linear fields,
continuity, second order in time, every branch of the fate rule, and that a particle which is not LIVE is frozen.
The GPU kernel is judged against this statement (tests/test_gpu_tracers.py)."""
import math

import numpy as np
import pytest

from derived_ref import DGrid
from oracle import OGrid
from polygons import LSHAPE
from tracer_ref import EXITED, LIVE, STUCK, TGrid, Tracers

EPS = np.finfo(np.float64).eps
BC_CAVITY = [(2, 0.0), (2, 1.0), (2, 0.0), (2, 0.0)]
BC_CHANNEL = [(0, 1.0), (2, 0.0), (4, 0.0), (2, 0.0)]   # inlet W, walls N / S, NEUMANN outflow E


def rect(nx, ny, bc, xr=-1, yr=-1):
    return TGrid(DGrid.from_oracle(OGrid.rectangle(nx, ny, bc=bc, xratio=xr, yratio=yr), bc))


def lshape():
    og = OGrid(LSHAPE["vertices"], LSHAPE["xspec"], LSHAPE["yspec"], LSHAPE["bc"])
    return TGrid(DGrid.from_oracle(og, LSHAPE["bc"]))


# ------------------------------------------------------------------ 1. a field linear in x and y is sampled exactly
def test_linear_field_is_exact():
    T = rect(12, 10, BC_CAVITY, 1.1, 0.9)
    X, Y = np.meshgrid(T.xc, T.yc, indexing="ij")
    planes = [(0.3, -1.7, 0.9), (-0.8, 0.6, 2.1)]
    q = [a + b * X + c * Y for a, b, c in planes]
    rng = np.random.default_rng(7)
    # at least one cell from every boundary: all four nodes are cell centres
    xs = rng.uniform(T.xf[1], T.xf[-2], 500)
    ys = rng.uniform(T.yf[1], T.yf[-2], 500)
    worst = 0.0
    for d in range(2):
        a, b, c = planes[d]
        M = np.max(np.abs(q[d]))
        for x, y in zip(xs, ys):
            i, j = T.cell(x, y)
            err = abs(T.sample(q[d], d, x, y, i, j) - (a + b * x + c * y))
            worst = max(worst, err / M)
            assert err <= 16 * EPS * M, (d, x, y, err / (EPS * M))
    print(f"linear field: worst error {worst / EPS:.2f} eps max|q|")


# ------------------------------------------------------------------ 2. continuity
def lipschitz_field(T, rng):
    """A random field of amplitude M = 4 whose node-to-node slopes stay below 48 M per unit length on the 32 x 32
    L-shape (h = 1 / 32), so that two points 2e-9 apart differ by at most 0.96e-7 M: values in [-2, 4] (neighbours
    differ by <= 6 = 1.5 M over h), in [-2, 3] in the cells with a boundary face (the face values are 0 or the unit
    lid's 1: <= 3 = 0.75 M over h / 2).  The bound of the test below, 1e-7 max|q|, is this Lipschitz bound."""
    G = T.G
    q = np.where(G.mask, rng.uniform(-2.0, 4.0, (T.nx, T.ny)), 0.0)
    wall = G.mask & (G.tag >= 0).any(axis=2)
    q[wall] = rng.uniform(-2.0, 3.0, int(wall.sum()))
    q[4, 4] = 4.0
    return q


def test_sample_is_continuous_across_faces_and_quadrant_lines():
    T = lshape()
    G = T.G
    rng = np.random.default_rng(11)
    q = [lipschitz_field(T, rng), lipschitz_field(T, rng)]
    dlt, worst, npairs, skipped = 1e-9, 0.0, 0, 0

    def pair(d, p0, p1):
        nonlocal worst, npairs
        va = T.sample(q[d], d, *p0, *T.cell(*p0))
        vb = T.sample(q[d], d, *p1, *T.cell(*p1))
        worst = max(worst, abs(va - vb) / np.max(np.abs(q[d])))
        npairs += 1

    for i, j in zip(*np.nonzero(G.mask)):
        x0, x1, y0, y1 = T.xf[i], T.xf[i + 1], T.yf[j], T.yf[j + 1]
        fr = (0.13, 0.37, 0.61, 0.89)
        for d in range(2):
            for f in fr:
                x, y = x0 + f * (x1 - x0), y0 + f * (y1 - y0)
                # the cell's own quadrant lines
                pair(d, (T.xc[i] - dlt, y), (T.xc[i] + dlt, y))
                pair(d, (x, T.yc[j] - dlt), (x, T.yc[j] + dlt))
                # its E and N faces toward a neighbour in the domain
                if G.inside(i + 1, j):
                    # the sample is discontinuous only at a re-entrant corner: on the half of an x-face whose two cells
                    # disagree about the y-neighbour of that half (one interpolates to a cell centre, the other to
                    # its wall face)
                    sy = 1 if y >= T.yc[j] else -1
                    if G.inside(i, j + sy) != G.inside(i + 1, j + sy):
                        skipped += 1
                    else:
                        pair(d, (x1 - dlt, y), (x1 + dlt, y))
                if G.inside(i, j + 1):
                    pair(d, (x, y1 - dlt), (x, y1 + dlt))
    print(f"continuity: {npairs} pairs, worst difference {worst:.3e} max|q|, {skipped} re-entrant half-faces left out")
    assert skipped == 2 * 2   # the one x-face at the L's inner corner, its lower half: 2 of the 4 fractions, u and v
    assert worst <= 1e-7


# ------------------------------------------------------------------ 3. second order in time with the Euler start-up
def closing_error(n):
    T = rect(16, 16, BC_CAVITY)
    X, Y = np.meshgrid(T.xc, T.yc, indexing="ij")
    u, v = -(Y - 0.5), X - 0.5
    P = Tracers(T)
    P.add([0.8], [0.5])
    P.advance(u, v, 2 * math.pi / n, n)
    assert P.state[0] == LIVE
    return math.hypot(P.x[0] - 0.8, P.y[0] - 0.5)


def test_solid_body_rotation_is_second_order():
    e200, e400 = closing_error(200), closing_error(400)
    print(f"closing error: n = 200 {e200:.6e}, n = 400 {e400:.6e}, ratio {e200 / e400:.4f}")
    assert 3.9 <= e200 / e400 <= 4.1


# ------------------------------------------------------------------ 4 / 5. the fate rule, branch by branch; frozen state
def snapshot(P):
    return [a.copy() for a in (P.x, P.y, P.wu, P.wv, P.age, P.state)]


def test_fates_and_frozen_state():
    nx, ny = 24, 16
    hx, hy = 1.0 / nx, 1.0 / ny
    one = np.ones((nx, ny))
    snaps = []

    def run(T, x, y, u, v, dt, want, steps=1):
        P = Tracers(T)
        P.add([x], [y])
        P.advance(u, v, dt, steps)
        assert P.state[0] == want, (x, y, P.state[0], want)
        if want != LIVE and steps == 1:   # it did not move, nor age, nor keep a sample
            assert P.x[0] == x and P.y[0] == y and P.age[0] == 0.0 and P.wu[0] == 0.0 and P.wv[0] == 0.0
        snaps.append((P, u, v, dt))
        return P

    C = rect(nx, ny, BC_CHANNEL)
    # out through the NEUMANN E side; through the W inlet (against the stream)
    run(C, 1.0 - 0.5 * hx, 0.5, one, 0 * one, 0.8 * hx, EXITED)
    run(C, 0.5 * hx, 0.5, -one, 0 * one, 0.8 * hx, EXITED)
    # a second step takes it out: the first was an Euler step, the second AB2, the age is one step's
    P = run(C, 1.0 - 1.5 * hx, 0.5, one, 0 * one, 0.8 * hx, EXITED, steps=2)
    assert P.age[0] == 0.8 * hx and P.x[0] == (1.0 - 1.5 * hx) + 0.8 * hx * 1.0
    # a wall: STUCK (v = -1 in the bottom row: the sample there is between -1 and the wall's 0)
    run(C, 0.5, 0.3 * hy, 0 * one, -one, 2.0 * hy, STUCK)
    # out of the box in both axes: the x side is tested first -- NEUMANN E on the channel, a wall on the cavity
    run(C, 1.0 - 0.4 * hx, 0.4 * hy, one, -one, 2.0 * hy, EXITED)
    run(rect(nx, ny, BC_CAVITY), 1.0 - 0.4 * hx, 0.4 * hy, one, -one, 2.0 * hy, STUCK)
    # a jump past the L's inner corner into the missing quadrant: both face neighbours are in the domain -- STUCK
    Lg = lshape()
    h = 1.0 / 32
    m = Lg.G.mask
    P = run(Lg, 0.5 - 0.2 * h, 0.5 + 0.2 * h, np.where(m, 1.0, 0.0), np.where(m, -1.0, 0.0), 0.6 * h, STUCK)
    # ... and the same start with a small step stays LIVE (the case above is the jump, not the seed)
    run(Lg, 0.5 - 0.2 * h, 0.5 + 0.2 * h, np.where(m, 1.0, 0.0), np.where(m, -1.0, 0.0), 0.1 * h, LIVE)
    # a NaN position, a NaN sample
    P = Tracers(C)
    P.add([0.5, 0.25], [0.5, 0.5])
    P.x[0] = float("nan")
    bad = one.copy()
    bad[C.cell(0.25, 0.5)] = float("nan")
    P.advance(bad, 0 * one, 0.1 * hx)
    assert list(P.state) == [STUCK, STUCK] and P.x[1] == 0.25 and P.age[1] == 0.0
    snaps.append((P, one, 0 * one, 0.1 * hx))
    # 5. further steps change nothing in a particle that is not LIVE, bit for bit
    for P, u, v, dt in snaps:
        before, dead = snapshot(P), P.state != LIVE
        P.advance(u, v, dt, 5)
        for a, b in zip(before, snapshot(P)):
            assert np.array_equal(a[dead], b[dead], equal_nan=True)
    assert P.counts() == {"n": 2, "live": 0, "exited": 0, "stuck": 2, "age_max": 0.0}


def test_seeds_outside_the_domain_are_refused():
    P = Tracers(lshape())
    for x, y in ((0.75, 0.25), (-0.1, 0.5), (0.5, 1.0), (float("nan"), 0.5)):
        with pytest.raises(ValueError, match="seed 0"):
            P.add([x], [y])
    assert P.n == 0
