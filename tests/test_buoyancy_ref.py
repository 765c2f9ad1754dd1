"""CPU: the composed reference step of tests/buoyancy_ref.py against the oracle's own step, and its folded
body force against a plain AB2 that keeps the previous force in a variable."""
import numpy as np

from buoyancy_ref import FIELDS, BuoyantRef, force, velocity_step, zero_state
from oracle import OGrid, OSolver
from scalar_ref import scalar_rhs

BC_CAVITY = [(2, 0.0), (2, 1.0), (2, 0.0), (2, 0.0)]
WALLS = [(2, 0.0)] * 4
S_SIDE = [("dirichlet", 1.0), ("zerograd",), ("dirichlet", 0.0), ("zerograd",)]   # hot W, cold E, adiabatic N / S


def test_composed_step_without_force_is_the_oracles_step():
    nx, ny, dt, re = 12, 10, 1.0 / 96, 100.0
    og = OGrid.rectangle(nx, ny, bc=BC_CAVITY)
    osv = OSolver(og, dt, re, rtol=1e-13)
    st = zero_state(og)
    for k in range(4):
        osv.step()
        st = velocity_step(og, dt, re, st, None, rtol=1e-13)
        ref = osv.get()
        for q in FIELDS:
            d = float(np.max(np.abs(st[q] - ref[q])))
            assert d == 0.0, (k, q, d)
    assert np.max(np.abs(st["u"])) > 1e-3   # (the lid moved the fluid: not a comparison of zeros)


def test_folded_force_is_plain_ab2():
    nx, ny, dt, re, pe = 12, 10, 2e-3, 1 / 0.71, 1.0
    bx, by, tref = -120.0, 710.0, 0.5
    rng = np.random.default_rng(31)
    T0 = rng.uniform(0, 1, (nx, ny))
    fold = BuoyantRef(nx, ny, WALLS, S_SIDE, dt, re, pe, bx=bx, by=by, tref=tref)
    fold.T = T0.copy()
    # the plain form: cu, cv stay the convective terms, the previous step's force in a variable of its own
    og, ogT = fold.og, fold.ogT
    st, T, cT = zero_state(og), T0.copy(), np.zeros((nx, ny))
    fprev = (og.z(), og.z())
    alpha = dt / (2 * re)
    for k in range(3):
        fold.step()
        u, v = st["u"].reshape(nx, ny), st["v"].reshape(nx, ny)
        rT, cTn = scalar_rhs(og.hx, og.hy, dt, pe, u, v, T, cT, fold.ugh, fold.vgh, fold.tgh)
        f = force(T, bx, by, tref)
        ru, rv, cu, cv = og.rhs_velocity(dt, re, st["u"], st["v"], st["gx"], st["gy"], st["cu"], st["cv"])
        ru = ru + dt * (1.5 * f[0] - 0.5 * fprev[0])
        rv = rv + dt * (1.5 * f[1] - 0.5 * fprev[1])
        us, _ = og.solve_helmholtz(alpha, ru)
        vs, _ = og.solve_helmholtz(alpha, rv)
        phi, _ = og.solve_poisson(og.divergence(dt, us, vs), x0=st["phi"])
        un, vn, gx, gy = og.correct(dt, us, vs, phi)
        st = {"u": un, "v": vn, "phi": phi, "cu": cu, "cv": cv, "gx": gx, "gy": gy}
        Tn, _ = ogT.solve_helmholtz(dt / (2 * pe), rT.ravel(), x0=T.ravel())
        T, cT, fprev = Tn.reshape(nx, ny), cTn, f
        for q in ("u", "v"):
            e = np.max(np.abs(fold.st[q] - st[q])) / np.max(np.abs(st[q]))
            assert e <= 1e-13, (k, q, e)
        assert np.max(np.abs(fold.T - T)) <= 1e-13 * np.max(np.abs(T))
        # the folded state's explicit term is convective minus force
        assert np.max(np.abs(fold.st["cv"] - (cv - f[1]))) <= 1e-13 * np.max(np.abs(f[1]))
        assert np.max(np.abs(fold.st["cu"] - (cu - f[0]))) <= 1e-13 * np.max(np.abs(f[0]))
    assert np.max(np.abs(st["v"])) > 1e-2   # (the force moved the fluid)
