"""The reference for boundary values that vary along an edge (ns_edge_profile; DESIGN.md 4, "Edge profiles"),
built from the oracle as it stands -- which knows one value per edge.  TEST INFRASTRUCTURE ONLY.

The ghost across an x-normal edge enters a cell's rhs_velocity / divergence / scalar right-hand side only through
that cell's own column j, the ghost across a y-normal edge only through its own row i: every ghost the stencils
evaluate lies across a face of the cell's own column (x-normal) or row (y-normal).  So the result in cell (i, j) on a
grid with profiles is exactly the oracle's result in that cell on the same grid with each profiled edge given the
UNIFORM value its profile has at j (x-normal) or at i (y-normal).  ProfiledGrid keeps one oracle grid per column
if only x-normal edges are profiled, one per row if only y-normal ones are, one per cell if both are, and stitches
the pieces.  The Helmholtz and Poisson solves and the correction do not see velocity ghosts (any of the grids
does), so a full step composes as buoyancy_ref.velocity_step does."""
import numpy as np

from oracle import OGrid
from scalar_ref import scalar_rhs, velocity_ghosts

INLET, INLET_PARABOLIC, WALL, NEUMANN = 0, 1, 2, 4
FIELDS = ("u", "v", "phi", "cu", "cv", "gx", "gy")


def rect_spec(nx, ny, bc, lx=1.0, ly=1.0, xr=-1, yr=-1):
    """OGrid.rectangle's polygon as a spec (polygons.py's form): edges W, N, E, S."""
    return dict(vertices=[(0, 0), (0, ly), (lx, ly), (lx, 0)], xspec=[[0, lx, nx, xr]], yspec=[[0, ly, ny, yr]],
                bc=list(bc))


def edge_is_xnormal(spec, e):
    V = spec["vertices"]
    a, b = V[e], V[(e + 1) % len(V)]
    return a[0] == b[0]


class ProfiledGrid:
    """spec: dict(vertices, xspec, yspec, bc); profiles: {edge: per-face info, ny values (x-normal edge) or nx}."""

    def __init__(self, spec, profiles):
        self.spec = spec
        self.base = OGrid(spec["vertices"], spec["xspec"], spec["yspec"], self._bc(spec["bc"], {}, 0, 0))
        og = self.base
        self.nx, self.ny, self.N = og.nx, og.ny, og.N
        ids = og.id.reshape(og.nx, og.ny)
        self.ci, self.cj = np.nonzero(ids >= 0)          # compact order: i outer, j inner
        assert np.array_equal(ids[self.ci, self.cj], np.arange(og.N))
        self.set_profiles(profiles)

    @staticmethod
    def _bc(bc, profiles, i, j):
        out = []
        for e, (t, info) in enumerate(bc):
            t = INLET if t == INLET_PARABOLIC else t      # (the oracle knows uniform edges only)
            if e in profiles:
                info = profiles[e][1][j if profiles[e][0] else i]
            out.append((t, float(info)))
        return out

    def set_profiles(self, profiles):
        """(Re)build the oracle grids: one per column / row / cell."""
        sp = self.spec
        P = {}
        for e, a in profiles.items():
            xn = edge_is_xnormal(sp, e)
            a = np.asarray(a, dtype=np.float64)
            assert a.size == (self.ny if xn else self.nx), (e, a.size)
            assert sp["bc"][e][0] != NEUMANN
            P[e] = (xn, a)
        anyx = any(xn for xn, _ in P.values())
        anyy = any(not xn for xn, _ in P.values())
        self.mode = "cell" if anyx and anyy else "col" if anyx else "row" if anyy else "one"
        make = lambda i, j: OGrid(sp["vertices"], sp["xspec"], sp["yspec"], self._bc(sp["bc"], P, i, j))
        if self.mode == "one":
            self.grids = [(make(0, 0), np.arange(self.N))]
        elif self.mode == "col":
            self.grids = [(make(0, j), np.nonzero(self.cj == j)[0]) for j in np.unique(self.cj)]
        elif self.mode == "row":
            self.grids = [(make(i, 0), np.nonzero(self.ci == i)[0]) for i in np.unique(self.ci)]
        else:
            self.grids = [(make(self.ci[k], self.cj[k]), np.array([k])) for k in range(self.N)]
        self.profiles = P
        return self

    def stitch(self, fn, nout):
        """fn(og) -> nout flat compact arrays; each cell's values from its own grid."""
        out = [np.zeros(self.N) for _ in range(nout)]
        for og, cells in self.grids:
            res = fn(og)
            for o, r in zip(out, res):
                o[cells] = np.asarray(r)[cells]
        return out

    def z(self):
        return np.zeros(self.N)

    def rhs_velocity(self, dt, re, u, v, gx, gy, cu, cv):
        return self.stitch(lambda og: og.rhs_velocity(dt, re, u, v, gx, gy, cu, cv), 4)

    def divergence(self, dt, us, vs):
        return self.stitch(lambda og: (og.divergence(dt, us, vs),), 1)[0]

    def scalar_rhs(self, dt, pe, u, v, T, cT0, tgh):
        """scalar_ref.scalar_rhs stitched (a rectangle: edges W, N, E, S; u, v, T, cT0 as (nx, ny)).  The stencil
        reaches two cells, so only the cells within two of a profiled side see its ghost: the others are one
        evaluation with the edges' own values, and each of those cells is evaluated on the block of cells within
        three of it (its whole stencil, with every existence test as on the full grid) with its own uniform values."""
        nx, ny = self.nx, self.ny
        hx, hy = self.base.hx, self.base.hy
        ugh, vgh = velocity_ghosts(self._bc(self.spec["bc"], {}, 0, 0))
        rT, cT = scalar_rhs(hx, hy, dt, pe, u, v, T, cT0, ugh, vgh, tgh)
        near = np.zeros((nx, ny), dtype=bool)
        for e in self.profiles:
            side = (0, 3, 1, 2)[e]                       # edge W, N, E, S -> side W, E, S, N
            if side == 0: near[:2] = True
            if side == 1: near[-2:] = True
            if side == 2: near[:, :2] = True
            if side == 3: near[:, -2:] = True
        for i, j in zip(*np.nonzero(near)):
            r0, r1, c0, c1 = max(i - 3, 0), min(i + 4, nx), max(j - 3, 0), min(j + 4, ny)
            ugh, vgh = velocity_ghosts(self._bc(self.spec["bc"], self.profiles, i, j))
            blk = (slice(r0, r1), slice(c0, c1))
            r, c = scalar_rhs(hx[r0:r1], hy[c0:c1], dt, pe, u[blk], v[blk], T[blk], cT0[blk], ugh, vgh, tgh)
            rT[i, j], cT[i, j] = r[i - r0, j - c0], c[i - r0, j - c0]
        return rT, cT

    def to_box(self, a):
        """A compact array on the bounding box (0 outside)."""
        out = np.zeros((self.nx, self.ny))
        out[self.ci, self.cj] = a
        return out

    def from_box(self, a):
        return np.asarray(a, dtype=np.float64).reshape(self.nx, self.ny)[self.ci, self.cj].copy()


def zero_state(pg):
    return {k: pg.z() for k in FIELDS}


def velocity_step(pg, dt, re, st, rtol=1e-13):
    """buoyancy_ref.velocity_step with the stitched rhs_velocity and divergence; solve_helmholtz, solve_poisson and
    correct do not see velocity ghosts (the base grid's)."""
    og = pg.base
    ru, rv, cu, cv = pg.rhs_velocity(dt, re, st["u"], st["v"], st["gx"], st["gy"], st["cu"], st["cv"])
    alpha = dt / (2 * re)
    us, _ = og.solve_helmholtz(alpha, ru, rtol=rtol)
    vs, _ = og.solve_helmholtz(alpha, rv, rtol=rtol)
    rp = pg.divergence(dt, us, vs)
    phi, _ = og.solve_poisson(rp, x0=st["phi"], rtol=rtol)
    u, v, gx, gy = og.correct(dt, us, vs, phi)
    return {"u": u, "v": v, "phi": phi, "cu": cu, "cv": cv, "gx": gx, "gy": gy}


def parabola_faces(h, k0, k1, mean):
    """NumPy restatement of ns_parabolic_profile (float64 positions)."""
    h = np.asarray(h, dtype=np.float64)
    out = np.zeros(h.size)
    X = np.concatenate([[0.0], np.cumsum(h[k0:k1])])
    s = X / X[-1]
    sa, sb = s[:-1], s[1:]
    out[k0:k1] = mean * (3 * (sa + sb) - 2 * (sa * sa + sa * sb + sb * sb))
    return out
