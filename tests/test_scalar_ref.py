"""CPU: the passive scalar's NumPy restatement (tests/scalar_ref.py) against the oracle.

With the transverse velocity identically zero (its ghost constants too), a scalar that IS the
normal velocity component -- T = u, cT0 = cu0, pe = re, the scalar's boundary conditions u's own
(Dirichlet value c0 / 2, zero-gradient on NEUMANN edges) -- is advanced by ConstructRHS_V itself:
the scalar flux 0.5 (n1 T1 + n2 T2 - |n1 + n2| (T2 - T1)) is fnn on the x-faces and fuv's value on
the y-faces (0).  So the restatement's rT, cT equal og_rhs_velocity's rhs_u, cu with grad phi = 0,
and likewise for T = v with u = 0.  The restatement must also commute with transposing the problem.
Tolerance: 1e-13 relative to max |oracle| (the two differ by rounding order only; 0.0 was observed)."""
import numpy as np
import pytest

from scalar_ref import IDENTITY_CASES, identity_inputs, identity_oracle, scalar_rhs, velocity_ghosts


def rel(a, b):
    return np.max(np.abs(np.asarray(a).ravel() - np.asarray(b).ravel())) / max(np.max(np.abs(b)), 1e-300)


@pytest.mark.parametrize("nx,ny,xr,yr,bc,comp", IDENTITY_CASES)
def test_restatement_is_the_oracles_velocity_rhs(nx, ny, xr, yr, bc, comp):
    og, dt, re, u, v, cu, cv = identity_inputs(nx, ny, xr, yr, bc, comp)
    ugh, vgh = velocity_ghosts(bc)
    other = vgh if comp == "u" else ugh
    assert all(c == 0.0 for _, c in other), "the identity needs the transverse component's ghost constants zero"
    tgh = ugh if comp == "u" else vgh
    rT, cT = scalar_rhs(og.hx, og.hy, dt, re, u, v, u if comp == "u" else v, cu if comp == "u" else cv, ugh, vgh, tgh)
    r_ref, c_ref = identity_oracle(og, dt, re, u, v, cu, cv, comp)
    print(f"{nx}x{ny} {comp}: rT {rel(rT, r_ref):.2e} cT {rel(cT, c_ref):.2e}")
    assert rel(rT, r_ref) <= 1e-13
    assert rel(cT, c_ref) <= 1e-13


def test_restatement_commutes_with_transposition():
    rng = np.random.default_rng(12)
    nx, ny = 7, 9
    hx = 0.1 * 1.1 ** np.arange(nx)
    hy = 0.2 * 0.9 ** np.arange(ny)
    u, v, T, c0 = (rng.uniform(-1, 1, (nx, ny)) for _ in range(4))
    ugh = [(0, 0.6), (1, 0.0), (0, 0.0), (0, 2.0)]
    vgh = [(0, -0.4), (1, 0.0), (0, 0.0), (0, 0.0)]
    # (no corner between two Dirichlet sides with non-zero constants: their two wall terms are added in side
    # order, which transposition swaps -- a rounding, not a symmetry, difference)
    tgh = [(0, 2.0), (1, 0.0), (0, 0.0), (1, 0.0)]
    rT, cT = scalar_rhs(hx, hy, 2e-3, 71.0, u, v, T, c0, ugh, vgh, tgh)
    sw = lambda tab: [tab[2], tab[3], tab[0], tab[1]]   # x <-> y: W <-> S, E <-> N
    rTt, cTt = scalar_rhs(hy, hx, 2e-3, 71.0, v.T.copy(), u.T.copy(), T.T.copy(), c0.T.copy(), sw(vgh), sw(ugh), sw(tgh))
    assert np.array_equal(rTt.T, rT)
    assert np.array_equal(cTt.T, cT)
