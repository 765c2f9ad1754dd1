"""(r5) The masked Poisson solve's capacitance method (ns_solver.cpp cap_setup / cap_solve, ns_fps.hip k_cap_*;
DESIGN.md 4) restated in numpy on the oracle's operators -- CPU, no GPU. The operators are oracle/ns_oracle.c's
og_apply_poisson, the restatement of the reference's assembled matrices (FluidSolver.cpp:105-163) on Grid.cpp:149-185's
polygons and on their bounding boxes. Checked:
  * the identity the method rests on: on the domain's rows, the masked operator is the bounding box's plus one rank-1
    term w_f d_f d_f^T per interface face f = (i in the domain, j outside), d_f = e_i - e_j -- the coupling to the
    cells outside vanishes;
  * the solve as the GPU runs it -- two box solves around the capacitance system, with C's columns and the
    regularisation (+ sum_c y_c y_c^T / m_c, one term per connected component c of the box's outside cells, y_c the
    indicator of the m_c faces that touch it) and border exactly as cap_setup / k_cap_col form them -- reproduces
    the masked operator's projected-sense solution to 1e-10.  Cases: an L-shape, whose box's walls make the box
    operator consistent with mean-free right-hand sides; a backward-facing step, whose box has the E outflow, so
    mode 0 is solved in the projected sense and the system is bordered by the domain's constant; polygons.NARROW:
    2-cell arms and throats, a 1-cell divider, and boxes whose outside falls into 2 to 4 components (a plus, a
    dumbbell, tees, a channel with a constriction and the E outflow);
  * the flood fill's component counts;
  * the matrix that is inverted is not singular up to rounding: C has one null vector per outside component, so the
    earlier single term 1 1^T / m left a T, a plus, a dumbbell and a constricted channel with singular values and
    Gauss-Jordan pivots of 1e-16 ... 1e-13 -- noise either side of k_gj_prep's 1e-12 guard.  The smallest singular
    value and the smallest |pivot| of the non-pivoting Gauss-Jordan must stay above 1e-3 of the `stairs` shape's
    (one component, 7 corners: the same matrix under either formulation; every regularised shape here stays within a
    factor 4 of it); the single-term formulation must fall below that floor.
The box solve F is the projected-sense solve the GPU's direct solve computes (L x = r + mu 1, mu fixed by
consistency), here by least squares."""
import functools

import numpy as np
import pytest

from oracle import OGrid
from polygons import NARROW, NARROW_COMPONENTS

WALL, NEU = (2, 0.0), (4, 0.0)
CASES = {
    # name: vertices, edge BCs, box BCs (rectangle order W, N, E, S), lx, nx, ny, bordered
    "lshape": ([(0, 0), (0, 1), (1, 1), (1, 0.5), (0.5, 0.5), (0.5, 0)], [WALL, (2, 1.0)] + [WALL] * 4,
               [WALL, (2, 1.0), WALL, WALL], 1.0, 12, 12, False),
    "step": ([(0, 0.5), (0, 1), (2, 1), (2, 0), (0.5, 0), (0.5, 0.5)], [(0, 1.0), WALL, NEU, WALL, WALL, WALL],
             [WALL, WALL, NEU, WALL], 2.0, 16, 8, True),
}
for _name, _P in NARROW.items():
    _out = any(t == 4 for t, _ in _P["bc"])         # (throat_out: the box's E column is the outflow)
    CASES[_name] = (_P["vertices"], _P["bc"], [WALL, WALL, NEU if _out else WALL, WALL], _P["xspec"][0][1],
                    _P["xspec"][0][2], _P["yspec"][0][2], _out)
COMPONENTS = dict(NARROW_COMPONENTS, lshape=1, step=1)


def dense(apply, n):
    A = np.empty((n, n))
    for k in range(n):
        e = np.zeros(n)
        e[k] = 1.0
        A[:, k] = apply(e)
    return A


def projected_solve(L, r):
    """x with L x = r + mu 1 for the mu that makes it consistent (the least-squares solution of [L, -1])."""
    n = L.shape[0]
    sol = np.linalg.lstsq(np.hstack([L, -np.ones((n, 1))]), r, rcond=None)[0]
    return sol[:n]


def outside_components(ids, nx, ny):
    """Label the box's cells outside the domain by connected component (4-neighbours), as cap_setup's flood fill."""
    lab = np.full(nx * ny, -1)
    nc = 0
    for s in range(nx * ny):
        if ids[s] >= 0 or lab[s] >= 0:
            continue
        lab[s] = nc
        stack = [s]
        while stack:
            i, j = divmod(stack.pop(), ny)
            for a, b in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)):
                if 0 <= a < nx and 0 <= b < ny and ids[a * ny + b] < 0 and lab[a * ny + b] < 0:
                    lab[a * ny + b] = nc
                    stack.append(a * ny + b)
        nc += 1
    return lab, nc


@functools.lru_cache(maxsize=None)
def setup(name):
    verts, bc, bbc, lx, nx, ny, bordered = CASES[name]
    og = OGrid(verts, [[0, lx, nx, -1]], [[0, 1, ny, -1]], bc)
    ob = OGrid.rectangle(nx, ny, lx=lx, ly=1.0, bc=bbc)
    assert og.nx == nx and og.ny == ny and ob.N == nx * ny
    Ld, Lb = dense(og.apply_poisson, og.N), dense(ob.apply_poisson, ob.N)
    ids = og.id.copy()
    dom = np.flatnonzero(ids >= 0)                 # box index of each domain cell, in compact-id order
    assert np.array_equal(ids[dom], np.arange(og.N))
    hx, hy = lx / nx, 1.0 / ny
    fi, fj, w = [], [], []                         # the interface faces (cap_setup's enumeration)
    for i in range(nx):
        for j in range(ny):
            if ids[i * ny + j] < 0:
                continue
            for di, dj, h in ((-1, 0, hx), (1, 0, hx), (0, -1, hy), (0, 1, hy)):
                a, b = i + di, j + dj
                if 0 <= a < nx and 0 <= b < ny and ids[a * ny + b] < 0:
                    fi.append(i * ny + j)
                    fj.append(a * ny + b)
                    w.append(1.0 / (h * h))
    m = len(fi)
    D = np.zeros((ob.N, m))
    D[fi, np.arange(m)] = 1.0
    D[fj, np.arange(m)] = -1.0
    lab, ncomp = outside_components(ids, nx, ny)
    return og, Ld, Lb, dom, D, np.array(w), bordered, lab[fj], ncomp


@functools.lru_cache(maxsize=None)
def system(name, reg):
    """The matrix the library inverts (reg "components": cap_setup / k_cap_col; "constant": the single term + 1 / m
    they formed before) and what the solve around it needs."""
    og, Ld, Lb, dom, D, w, bordered, fk, ncomp = setup(name)
    n, m = Lb.shape[0], D.shape[1]
    F = lambda r: projected_solve(Lb, r)            # noqa: E731 (the box's direct solve)
    Dw = D * w
    Z = np.column_stack([F(Dw[:, f]) for f in range(m)])
    if reg == "components":
        mc = np.bincount(fk, minlength=ncomp)
        R = (fk[:, None] == fk[None, :]) / mc[fk][None, :]
    else:
        R = 1.0 / m
    C = np.eye(m) + D.T @ Z + R                     # k_cap_col
    e1 = None
    if bordered:                                    # k_cap_col's border: column -D^T e1, row 1^T
        one_dom = np.zeros(n)
        one_dom[dom] = 1.0
        e1 = F(one_dom)
        M = np.zeros((m + 1, m + 1))
        M[:m, :m] = C
        M[:m, m] = -(D.T @ e1)
        M[m, :m] = 1.0
    else:
        M = C
    return M, F, Dw, e1


def gauss_jordan(M):
    """k_gj_prep / k_gj_step: the in-place inversion without pivoting; the inverse and the smallest |pivot|."""
    A = M.copy()
    pmin = np.inf
    for k in range(A.shape[0]):
        p = A[k, k]
        pmin = min(pmin, abs(p))
        t = A[k] / p
        t[k] = 1.0 / p
        u = A[:, k].copy()
        A -= np.outer(u, t)
        A[k] = t
        A[:, k] = -u * t[k]
        A[k, k] = t[k]
    return A, pmin


def conditioning(name, reg):
    M = system(name, reg)[0]
    return float(np.linalg.svd(M, compute_uv=False)[-1]), float(gauss_jordan(M)[1])


def noise_floor():
    """1e-3 of the stairs shape's smallest singular value and pivot (one component: the same under either
    regularisation)."""
    sv, piv = conditioning("stairs", "components")
    return 1e-3 * sv, 1e-3 * piv


@pytest.mark.parametrize("name", sorted(CASES))
def test_masked_operator_is_box_plus_interface_terms(name):
    og, Ld, Lb, dom, D, w = setup(name)[:6]
    Le = Lb + (D * w) @ D.T
    out = np.setdiff1d(np.arange(Lb.shape[0]), dom)
    scale = np.max(np.abs(Ld))
    assert np.max(np.abs(Le[np.ix_(dom, dom)] - Ld)) <= 1e-12 * scale
    assert np.max(np.abs(Le[np.ix_(dom, out)])) <= 1e-12 * scale


@pytest.mark.parametrize("name", sorted(CASES))
def test_capacitance_solve_matches_masked_projected_solve(name):
    og, Ld, Lb, dom, D, w, bordered = setup(name)[:7]
    n, m = Lb.shape[0], D.shape[1]
    rng = np.random.default_rng(7)
    b = rng.uniform(-1, 1, og.N)
    qd = b - b.mean()                               # r = b - mean on the domain (k_cap_rhs), 0 outside
    q = np.zeros(n)
    q[dom] = qd
    M, F, Dw, e1 = system(name, "components")
    Minv = gauss_jordan(M)[0]                        # (as the GPU: without pivoting, k_gj_*)
    z1 = F(q)
    g = D.T @ z1                                     # k_cap_gemv's gather
    y = Minv @ (np.append(g, 0.0) if bordered else g)
    x = F(q - Dw @ y[:m])                            # k_cap_scatter, then the second box solve
    if bordered:
        x = x + y[m] * e1                            # k_cap_axpy's lambda e1
    xd = x[dom]
    ref = projected_solve(Ld, qd)
    p, r = xd - xd.mean(), ref - ref.mean()
    assert np.max(np.abs(p - r)) <= 1e-10 * np.max(np.abs(r))
    res = Ld @ xd - qd
    res -= res.mean()                                # P (L x - q): the masked step's projected residual
    assert np.linalg.norm(res) <= 1e-10 * np.linalg.norm(qd)


@pytest.mark.parametrize("name", sorted(CASES))
def test_outside_component_count(name):
    nx, ny = CASES[name][4:6]
    og, fk, ncomp = setup(name)[0], setup(name)[7], setup(name)[8]
    assert ncomp == COMPONENTS[name]
    assert set(fk) == set(range(ncomp))             # every component is touched by a face
    lab, _ = outside_components(og.id, nx, ny)
    assert np.all((lab >= 0) == (og.id < 0))


@pytest.mark.parametrize("name", sorted(CASES))
def test_capacitance_matrix_is_not_inverted_on_noise(name):
    sv, piv = conditioning(name, "components")
    sv0, piv0 = noise_floor()
    print(f"{name}: smallest singular value {sv:.3e} (floor {sv0:.1e}), min |pivot| {piv:.3e} (floor {piv0:.1e})")
    assert sv >= sv0 and piv >= piv0, (sv, piv)


@pytest.mark.parametrize("name", sorted(CASES))
def test_single_term_regularisation_is_singular_on_split_complements(name):
    """The formulation before the per-component terms (+ 1 / m alone) fails the noise test exactly where the box's
    outside has more than one component, and is the same matrix where it has one."""
    sv, piv = conditioning(name, "constant")
    sv0, piv0 = noise_floor()
    if COMPONENTS[name] == 1:
        np.testing.assert_array_equal(system(name, "constant")[0], system(name, "components")[0])
        assert sv >= sv0 and piv >= piv0, (sv, piv)
    else:
        assert sv < sv0 and piv < piv0, (sv, piv)
