"""The derived fields of ns_derive -- pressure, vorticity, divergence, stream function and the integrals a run is
watched by -- stated in NumPy ("Derived fields").  This file is the normative statement; the GPU kernels
(k_derived_s, k_derived_grid, k_psi_base, k_psi_scan) are tested against it, and it against the oracle
(tests/test_derived_ref.py).  TEST INFRASTRUCTURE ONLY.

Fields are (nx, ny) bounding-box planes, i outer, 0 outside the domain.  Faces k: 0 W, 1 E, 2 S, 3 N.

Face values are Div_V's (FluidSolver.cpp:380-418): toward a neighbour in the domain q_nb r + q_c (1 - r) with
r = h_c / (h_nb + h_c); on a boundary face 0.5 (q_c + ghost) with that edge's velocity ghost of component d
(EvaluateGhostStencil_V): q_c on a NEUMANN edge, -q_c + c_d otherwise, c_d = 2 info in an inlet's normal and a
wall's tangential component and 0 in the other one, info the edge's own value or its profile's entry at the face
(ns_edge_profile: index j on an x-normal edge, i on a y-normal one).

  div  = (u_E - u_W) / hx + (v_N - v_S) / hy
  vort = (v_E - v_W) / hx - (u_N - u_S) / hy      (x-faces: v with component 1's ghost; y-faces: u with component 0's)
  P    = phi - dt / (2 re) L phi, L the Poisson matrix: 2 / (h (h + h_nb)) (phi_nb - phi_c) toward a neighbour, 0
         across a wall / inlet face, (2.5 phi_c - 2 phi_1 + 0.5 phi_2 - phi_c) / h^2 across a NEUMANN face (phi_1,
         phi_2 the next two cells inward)
  psi  at the (nx + 1) x (ny + 1) cell vertices: psi(0, 0) = 0, psi(i + 1, 0) = psi(i, 0) - v_S(i, 0) hx[i] (the S
         boundary-face value of cell (i, 0); 0 if it is outside), psi(i, j + 1) = psi(i, j) + F(i, j), F the x-face
         value of u between cells (i - 1, j) and (i, j) times hy[j]: the interior value (cell (i, j)'s W face) if both
         are in the domain, the one cell's boundary-face value if one is, 0 if neither.  psi(i, j) is the volume flux
         through the vertical line from the box's bottom to the vertex: a flux function, not a Poisson solve,
         path-independent only up to the column's accumulated div * area; zero-flux faces keep it constant across
         holes and outside regions.
  ke = 1/2 sum A (u^2 + v^2), enstrophy = 1/2 sum A vort^2, div_l2 = sqrt(sum A div^2), div_max = max |div|,
  cfl = dt max(|u| / hx + |v| / hy) over the domain's cells, A = hx hy; min / max of vort, P over them, of psi over
  the vertices."""
import numpy as np

INLET, INLET_PARABOLIC, WALL, NEUMANN = 0, 1, 2, 4
DI, DJ = (-1, 1, 0, 0), (0, 0, -1, 1)
STATS = ("ke", "enstrophy", "div_l2", "div_max", "cfl", "vort_min", "vort_max", "p_min", "p_max", "psi_min", "psi_max")


class DGrid:
    """hx, hy; mask (nx, ny) bool; tag (nx, ny, 4): the edge on each face of a domain cell (-1: the neighbour is in
    the domain); bc: (type, info) per edge; profiles: {edge: per-face info}."""

    def __init__(self, hx, hy, mask, tag, bc, profiles=None):
        self.hx, self.hy = np.asarray(hx, dtype=np.float64), np.asarray(hy, dtype=np.float64)
        self.nx, self.ny = self.hx.size, self.hy.size
        self.mask = np.asarray(mask, dtype=bool).reshape(self.nx, self.ny)
        self.tag = np.asarray(tag).reshape(self.nx, self.ny, 4)
        self.bc = [(int(t), float(i)) for t, i in bc]
        self.profiles = {int(e): np.asarray(a, dtype=np.float64) for e, a in (profiles or {}).items()}

    @classmethod
    def from_oracle(cls, og, bc, profiles=None):
        """The oracle grid's cells and face tags with the boundary conditions bc (the oracle's own, or a variant)."""
        return cls(og.hx, og.hy, og.id.reshape(og.nx, og.ny) >= 0, og.tag.reshape(og.nx, og.ny, 4), bc, profiles)

    def inside(self, i, j):
        return 0 <= i < self.nx and 0 <= j < self.ny and bool(self.mask[i, j])

    def plane(self, compact):
        out = np.zeros((self.nx, self.ny))
        out[self.mask] = compact
        return out

    def neumann(self, i, j, k):
        return self.bc[self.tag[i, j, k]][0] == NEUMANN

    def ghost_v(self, q, i, j, k, d):
        e = int(self.tag[i, j, k])
        t, info = self.bc[e]
        if t == NEUMANN:
            return q[i, j]
        if e in self.profiles:
            info = self.profiles[e][j if k < 2 else i]
        comp = (0 if k < 2 else 1) if t in (INLET, INLET_PARABOLIC) else (1 if k < 2 else 0)
        return -q[i, j] + (2.0 * info if d == comp else 0.0)

    def face(self, q, i, j, k, d):
        """The value of the component-d field q on face k of the domain cell (i, j)."""
        ii, jj = i + DI[k], j + DJ[k]
        if self.inside(ii, jj):
            hc, hn = (self.hx[i], self.hx[ii]) if k < 2 else (self.hy[j], self.hy[jj])
            r = hc / (hn + hc)
            return q[ii, jj] * r + q[i, j] * (1 - r)
        return 0.5 * (q[i, j] + self.ghost_v(q, i, j, k, d))

    def lap(self, p, i, j):
        s = 0.0
        for k in range(4):
            ii, jj = i + DI[k], j + DJ[k]
            h, hn = (self.hx[i], self.hx[ii] if 0 <= ii < self.nx else 0.0) if k < 2 else \
                    (self.hy[j], self.hy[jj] if 0 <= jj < self.ny else 0.0)
            if self.inside(ii, jj):
                s += 2.0 / (h * (h + hn)) * (p[ii, jj] - p[i, j])
            elif self.neumann(i, j, k):
                gh = 2.5 * p[i, j] - 2.0 * p[i - DI[k], j - DJ[k]] + 0.5 * p[i - 2 * DI[k], j - 2 * DJ[k]]
                s += (gh - p[i, j]) / (h * h)
        return s


def cell_fields(G, dt, re, u, v, phi):
    """div, vort, P as planes (0 outside)."""
    div, vort, P = (np.zeros((G.nx, G.ny)) for _ in range(3))
    alpha = dt / (2 * re)
    for i, j in zip(*np.nonzero(G.mask)):
        uW, uE, uS, uN = (G.face(u, i, j, k, 0) for k in range(4))
        vW, vE, vS, vN = (G.face(v, i, j, k, 1) for k in range(4))
        div[i, j] = (uE - uW) / G.hx[i] + (vN - vS) / G.hy[j]
        vort[i, j] = (vE - vW) / G.hx[i] - (uN - uS) / G.hy[j]
        P[i, j] = phi[i, j] - alpha * G.lap(phi, i, j)
    return div, vort, P


def xface_flux(G, u, i, j):
    """F(i, j): the flux through the x-face between cells (i - 1, j) and (i, j)."""
    a, b = G.inside(i - 1, j), G.inside(i, j)
    if b:
        return G.face(u, i, j, 0, 0) * G.hy[j]          # (interior value, or cell (i, j)'s W boundary face)
    if a:
        return G.face(u, i - 1, j, 1, 0) * G.hy[j]
    return 0.0


def stream_function(G, u, v):
    psi = np.zeros((G.nx + 1, G.ny + 1))
    for i in range(G.nx):
        vS = G.face(v, i, 0, 2, 1) if G.inside(i, 0) else 0.0
        psi[i + 1, 0] = psi[i, 0] - vS * G.hx[i]
    for i in range(G.nx + 1):
        for j in range(G.ny):
            psi[i, j + 1] = psi[i, j] + xface_flux(G, u, i, j)
    return psi


def derived(G, dt, re, u, v, phi, psi=True):
    """Everything ns_derive returns: the planes under p, vort, div, psi and the stats under their field names."""
    u, v, phi = (np.asarray(a, dtype=np.float64).reshape(G.nx, G.ny) for a in (u, v, phi))
    div, vort, P = cell_fields(G, dt, re, u, v, phi)
    m = G.mask
    A = np.outer(G.hx, G.hy)[m]
    out = {"p": P, "vort": vort, "div": div}
    out["ke"] = 0.5 * np.sum(A * (u[m] ** 2 + v[m] ** 2))
    out["enstrophy"] = 0.5 * np.sum(A * vort[m] ** 2)
    out["div_l2"] = np.sqrt(np.sum(A * div[m] ** 2))
    out["div_max"] = np.max(np.abs(div[m]))
    out["cfl"] = dt * np.max((np.abs(u) / G.hx[:, None] + np.abs(v) / G.hy[None, :])[m])
    out["vort_min"], out["vort_max"] = vort[m].min(), vort[m].max()
    out["p_min"], out["p_max"] = P[m].min(), P[m].max()
    out["psi_min"] = out["psi_max"] = float("nan")
    if psi:
        out["psi"] = stream_function(G, u, v)
        out["psi_min"], out["psi_max"] = out["psi"].min(), out["psi"].max()
    return out
