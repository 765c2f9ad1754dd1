"""One reference time step with Boussinesq buoyancy, composed from the oracle's own pieces: the normative
definition of what ns_step computes once ns_scalar_buoyancy is on ("Buoyancy").
TEST INFRASTRUCTURE ONLY.

The order is OSolver.step's (FluidSolver::Solve): rhs_velocity, [the force and its fold], solve_helmholtz x2 from
a zero guess, divergence, solve_poisson warm-started from phi, correct.  The force f = (bx, by) (T^n - tref) is
AB2 like the convective term, dt (1.5 f^n - 0.5 f^{n-1}), and is folded into the stored explicit term, which
rhs_velocity carries from step to step with exactly those weights:

    ru += 1.5 dt f_x        (rhs_velocity's ru already holds + 0.5 dt cu0, cu0 = cu^{n-1} - f_x^{n-1})
    cu -= f_x               (the state's cu after the step: convective minus force)

and the same for v with f_y.  All fields are flat arrays in the oracle's compact order (a rectangle's: i outer,
j inner).  The scalar is advanced by scalar_ref.scalar_rhs and solve_helmholtz on oracle_bc_of(sbc)."""
import numpy as np

from oracle import OGrid
from scalar_ref import oracle_bc_of, scalar_ghosts, scalar_rhs, velocity_ghosts

FIELDS = ("u", "v", "phi", "cu", "cv", "gx", "gy")


def zero_state(og):
    return {k: og.z() for k in FIELDS}


def force(T, bx, by, tref):
    """(f_x, f_y) per cell; T flat or (nx, ny)."""
    d = np.asarray(T, dtype=np.float64).ravel() - tref
    return bx * d, by * d


def velocity_step(og, dt, re, st, f=None, rtol=1e-13):
    """One step of the velocities and phi from the state st (a dict of FIELDS); f = (f_x, f_y) of T^n or None.
    Returns the new state; with f None it is OSolver.step's, operation for operation."""
    ru, rv, cu, cv = og.rhs_velocity(dt, re, st["u"], st["v"], st["gx"], st["gy"], st["cu"], st["cv"])
    if f is not None:
        ru = ru + (1.5 * dt) * f[0]
        rv = rv + (1.5 * dt) * f[1]
        cu = cu - f[0]
        cv = cv - f[1]
    alpha = dt / (2 * re)
    us, _ = og.solve_helmholtz(alpha, ru, rtol=rtol)
    vs, _ = og.solve_helmholtz(alpha, rv, rtol=rtol)
    rp = og.divergence(dt, us, vs)
    phi, _ = og.solve_poisson(rp, x0=st["phi"], rtol=rtol)
    u, v, gx, gy = og.correct(dt, us, vs, phi)
    return {"u": u, "v": v, "phi": phi, "cu": cu, "cv": cv, "gx": gx, "gy": gy}


class BuoyantRef:
    """The coupled reference on a rectangle: velocities with the force of T^n, the scalar with u^n, v^n."""

    def __init__(self, nx, ny, bc, sbc, dt, re, pe, bx=0.0, by=0.0, tref=0.0, xr=-1, yr=-1, rtol=1e-13):
        self.og = OGrid.rectangle(nx, ny, bc=bc, xratio=xr, yratio=yr)
        self.ogT = OGrid.rectangle(nx, ny, bc=oracle_bc_of(sbc), xratio=xr, yratio=yr)
        self.shape = (nx, ny)
        self.dt, self.re, self.pe, self.rtol = dt, re, pe, rtol
        self.bx, self.by, self.tref = bx, by, tref
        self.ugh, self.vgh = velocity_ghosts(bc)
        self.tgh = scalar_ghosts(sbc)
        self.st = zero_state(self.og)
        self.T = np.zeros(self.shape)
        self.cT = np.zeros(self.shape)

    def load(self, u, v, phi, cu, cv, T, cT):
        """The state of a solver between steps (cu, cv: convective minus force); grad phi formed from phi."""
        gx, gy = self.og.grad_phi(np.ravel(phi))
        self.st = {"u": np.ravel(u).copy(), "v": np.ravel(v).copy(), "phi": np.ravel(phi).copy(),
                   "cu": np.ravel(cu).copy(), "cv": np.ravel(cv).copy(), "gx": gx, "gy": gy}
        self.T = np.asarray(T, dtype=np.float64).reshape(self.shape).copy()
        self.cT = np.asarray(cT, dtype=np.float64).reshape(self.shape).copy()

    def step(self):
        u, v = self.st["u"].reshape(self.shape), self.st["v"].reshape(self.shape)
        rT, cT = scalar_rhs(self.og.hx, self.og.hy, self.dt, self.pe, u, v, self.T, self.cT, self.ugh, self.vgh,
                            self.tgh)
        on = self.bx != 0.0 or self.by != 0.0
        f = force(self.T, self.bx, self.by, self.tref) if on else None
        self.st = velocity_step(self.og, self.dt, self.re, self.st, f, self.rtol)
        Tn, _ = self.ogT.solve_helmholtz(self.dt / (2 * self.pe), rT.ravel(), x0=self.T.ravel(), rtol=self.rtol)
        self.T, self.cT = Tn.reshape(self.shape), cT
        return self

    def field(self, k):
        return self.st[k].reshape(self.shape)
