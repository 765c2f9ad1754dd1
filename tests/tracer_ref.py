"""Lagrangian tracer particles (ns_tracers_*) stated in NumPy ("Tracers").  This file is the normative
statement; the GPU kernel (k_tracer) is tested against it (tests/test_gpu_tracers.py) and it against its own
properties (tests/test_tracer_ref.py).  TEST INFRASTRUCTURE ONLY.

Coordinates: positions are physical, relative to the bounding box's lower-left corner.  xf[0] = 0, xf[i + 1] =
xf[i] + hx[i] (summed one by one in double), centres xc[i] = 0.5 (xf[i] + xf[i + 1]); yf, yc likewise.  A point
belongs to cell i with xf[i] <= x < xf[i + 1]; x < 0, x >= xf[nx] or a non-finite x is outside the box.

Sampling w = (u, v) at (x, y) in the domain cell (i, j), component d with plane q: bilinear between cell centres
toward the quadrant the point lies in (sx = +1 if x >= xc[i] else -1, sy likewise); where the neighbour in x (or y)
is not in the domain, the node is the cell's own boundary face and the value there 0.5 (q + ghost), ghost being that
face's velocity ghost of component d (derived_ref.DGrid.ghost_v's rule: q on a NEUMANN edge, -q + c_d otherwise, the
edge's profile entry where one is set).  Row by row: R(j') interpolates along x in row j' (its own x-node: the
neighbour's centre or the face of cell (i, j')), then a = R(j) and b = R(j + sy) -- or, with no neighbour in y, the
face value 0.5 (a + ghost(a)) of cell (i, j)'s own y-face -- are interpolated along y.

Advance: one AB2 step of size dt (Euler for a particle's first step); fate of the new position: LIVE in a domain cell,
else EXITED through a NEUMANN / INLET face and STUCK at a wall, at a corner jump, or on anything non-finite.  A
particle that is not LIVE keeps its x, y, w and age and is never touched again."""
import math

import numpy as np

from derived_ref import INLET, INLET_PARABOLIC, NEUMANN, DGrid

LIVE, EXITED, STUCK = 0, 1, 2


def faces(h):
    f = np.zeros(len(h) + 1)
    for i in range(len(h)):
        f[i + 1] = f[i] + h[i]
    return f


def locate(f, x):
    """The cell of x along one axis: -1 below the box, n at or above its end, None if x is not finite."""
    n = len(f) - 1
    if not math.isfinite(x):
        return None
    if x < 0.0:
        return -1
    if x >= f[n]:
        return n
    return int(np.searchsorted(f, x, side="right")) - 1


def sign(a):
    return (a > 0) - (a < 0)


class TGrid:
    """A DGrid with the tracers' coordinate tables."""

    def __init__(self, G: DGrid):
        self.G = G
        self.nx, self.ny = G.nx, G.ny
        self.xf, self.yf = faces(G.hx), faces(G.hy)
        self.xc, self.yc = 0.5 * (self.xf[:-1] + self.xf[1:]), 0.5 * (self.yf[:-1] + self.yf[1:])

    def inside(self, i, j):
        return i is not None and j is not None and self.G.inside(i, j)

    def cell(self, x, y):
        return locate(self.xf, x), locate(self.yf, y)

    def ghost(self, val, i, j, k, d):
        """The velocity ghost of component d across the boundary face k of the domain cell (i, j), of the value val."""
        G = self.G
        e = int(G.tag[i, j, k])
        t, info = G.bc[e]
        if t == NEUMANN:
            return val
        if e in G.profiles:
            info = G.profiles[e][j if k < 2 else i]
        comp = (0 if k < 2 else 1) if t in (INLET, INLET_PARABOLIC) else (1 if k < 2 else 0)
        return -val + (2.0 * info if d == comp else 0.0)

    def sample(self, q, d, x, y, i, j):
        """Component d (plane q) at (x, y), a point of the domain cell (i, j)."""
        G = self.G
        sx = 1 if x >= self.xc[i] else -1
        sy = 1 if y >= self.yc[j] else -1
        kx, ky = (1 if sx > 0 else 0), (3 if sy > 0 else 2)

        def row(jp):
            qc = q[i, jp]
            if G.inside(i + sx, jp):
                xn, qn = self.xc[i + sx], q[i + sx, jp]
            else:
                xn, qn = self.xf[i + 1 if sx > 0 else i], 0.5 * (qc + self.ghost(qc, i, jp, kx, d))
            wx = (x - self.xc[i]) / (xn - self.xc[i])
            return qc + wx * (qn - qc)

        a = row(j)
        if G.inside(i, j + sy):
            b, yn = row(j + sy), self.yc[j + sy]
        else:
            b, yn = 0.5 * (a + self.ghost(a, i, j, ky, d)), self.yf[j + 1 if sy > 0 else j]
        wy = (y - self.yc[j]) / (yn - self.yc[j])
        return a + wy * (b - a)

    def exits(self, i, j, k):
        return self.G.bc[int(self.G.tag[i, j, k])][0] in (NEUMANN, INLET, INLET_PARABOLIC)


class Tracers:
    """The particle set: x, y, the previous step's sample (wu, wv), age, state and the fresh flag, by stable index."""

    def __init__(self, G: DGrid):
        self.T = G if isinstance(G, TGrid) else TGrid(G)
        self.x, self.y, self.wu, self.wv, self.age = (np.zeros(0) for _ in range(5))
        self.state = np.zeros(0, dtype=np.int32)
        self.fresh = np.zeros(0, dtype=bool)

    @property
    def n(self):
        return self.x.size

    def add(self, x, y):
        x, y = np.asarray(x, dtype=np.float64).ravel(), np.asarray(y, dtype=np.float64).ravel()
        for k in range(x.size):
            if not self.T.inside(*self.T.cell(x[k], y[k])):
                raise ValueError(f"seed {k} is not in a domain cell")
        z = np.zeros(x.size)
        self.x, self.y = np.concatenate([self.x, x]), np.concatenate([self.y, y])
        self.wu, self.wv, self.age = (np.concatenate([a, z]) for a in (self.wu, self.wv, self.age))
        self.state = np.concatenate([self.state, np.full(x.size, LIVE, dtype=np.int32)])
        self.fresh = np.concatenate([self.fresh, np.ones(x.size, dtype=bool)])

    def sample(self, u, v):
        """w at the current positions; a particle that is not LIVE reports the sample it froze with."""
        T = self.T
        su, sv = self.wu.copy(), self.wv.copy()
        for p in np.nonzero(self.state == LIVE)[0]:
            i, j = T.cell(self.x[p], self.y[p])
            su[p], sv[p] = T.sample(u, 0, self.x[p], self.y[p], i, j), T.sample(v, 1, self.x[p], self.y[p], i, j)
        return su, sv

    def step(self, u, v, dt):
        T = self.T
        for p in np.nonzero(self.state == LIVE)[0]:
            x, y = self.x[p], self.y[p]
            i, j = T.cell(x, y)
            if not T.inside(i, j):
                self.state[p] = STUCK
                continue
            wu, wv = T.sample(u, 0, x, y, i, j), T.sample(v, 1, x, y, i, j)
            if not (math.isfinite(wu) and math.isfinite(wv)):
                self.state[p] = STUCK
                continue
            if self.fresh[p]:
                xn, yn = x + dt * wu, y + dt * wv
            else:
                xn, yn = x + dt * (1.5 * wu - 0.5 * self.wu[p]), y + dt * (1.5 * wv - 0.5 * self.wv[p])
            ip, jp = T.cell(xn, yn)
            if ip is None or jp is None:
                self.state[p] = STUCK
                continue
            if T.inside(ip, jp):
                self.x[p], self.y[p], self.wu[p], self.wv[p] = xn, yn, wu, wv
                self.age[p] += dt
                self.fresh[p] = False
                continue
            di, dj = sign(ip - i), sign(jp - j)
            if di != 0 and not T.inside(i + di, j):
                k = 1 if di > 0 else 0
            elif dj != 0 and not T.inside(i, j + dj):
                k = 3 if dj > 0 else 2
            else:
                self.state[p] = STUCK
                continue
            self.state[p] = EXITED if T.exits(i, j, k) else STUCK

    def advance(self, u, v, dt, steps=1):
        """`steps` steps in the fields u, v (nx x ny planes) held fixed."""
        u, v = (np.asarray(a, dtype=np.float64).reshape(self.T.nx, self.T.ny) for a in (u, v))
        for _ in range(steps):
            self.step(u, v, dt)

    def counts(self):
        live = self.state == LIVE
        return {"n": self.n, "live": int(live.sum()), "exited": int((self.state == EXITED).sum()),
                "stuck": int((self.state == STUCK).sum()), "age_max": float(self.age[live].max()) if live.any() else 0.0}
