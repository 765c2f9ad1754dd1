"""GPU: the four observers of the flow -- derived fields, tracer particles, running statistics, wall loads -- on ONE
solver with timing on, against solvers that carry one of them each and against a solver that carries none.

The observers share the entry prologue, the buffer ownership and the interval recorder's drain; each per-feature test
has one observer per solver.  Here they run side by side: nothing one of them does may show in another's results, in
the step's counts, its monitor or its fields.  Every comparison is between two device runs of the same arithmetic, so
every bar is bit for bit.

Two things the grids force on the set-up:
  * a masked polygon carries no scalar (ns_scalar_enable refuses it), so the L-shape runs without one and its
    statistics without NS_AVG_SCALAR;
  * derived() settles a deferred correction (it reads the fields), which the step's k5_deferred and K5 counts show.
    The solver without observers is therefore settled after every step as well, by reading its fields.  The solvers
    with one step-side observer are not: under step_async on the cavity they run the deferred-K5 path, and their
    results must still equal the all-observer solver's bit for bit."""
import numpy as np
import pytest

from derived_ref import DGrid
from oracle import OGrid
from polygons import ALL
from test_gpu_loads import scalar_cavity
from test_gpu_tracers import BC_CAVITY, COUNTS, deep_seeds
from tracer_ref import TGrid

pytestmark = pytest.mark.gpu
STEPS, N = 8, 32
STEP_KEYS = ("it_u", "it_phi", "k5_deferred", "n_checks") + COUNTS
MONITOR = ("umin", "umax", "vmin", "vmax")
DERIVED_PLANES = ("p", "vort", "div", "psi")
DERIVED_SUMS = ("ke", "enstrophy", "div_l2", "div_max", "cfl", "vort_min", "vort_max", "p_min", "p_max", "psi_min", "psi_max")


def cavity_case(gpu):
    mk = lambda: scalar_cavity(gpu, n=N, timing=True)
    og = OGrid.rectangle(N, N, bc=BC_CAVITY)
    probe = mk()
    T = TGrid(DGrid(probe.hx, probe.hy, og.id.reshape(N, N) >= 0, og.tag, BC_CAVITY))
    probe.close()
    return mk, T, True


def lshape_case(gpu):
    P = ALL["lshape"]
    og = OGrid(P["vertices"], P["xspec"], P["yspec"], P["bc"])
    mk = lambda: gpu.GpuSolver(gpu.polygon(P["vertices"], og.hx, og.hy, P["bc"]), 1.0 / (8 * N), 400.0, timing=True)
    return mk, TGrid(DGrid.from_oracle(og, P["bc"])), False


CASES = {"cavity32": cavity_case, "lshape": lshape_case}


@pytest.mark.parametrize("mode", ["step", "step_async"])
@pytest.mark.parametrize("grid", list(CASES))
def test_observers_side_by_side(gpu, grid, mode):
    mk, T, scalar = CASES[grid](gpu)
    xs, ys = deep_seeds(T, 100, np.random.default_rng(58))
    on = {"tracers": lambda g: (g.enable_tracers(100), g.add_tracers(xs, ys)),
          "avg": lambda g: g.enable_averages(every=2, second=True, pressure=True, scalar=scalar),
          "loads": lambda g: g.enable_loads(every=3),
          "derived": lambda g: None}
    plain, full = mk(), mk()
    one = {k: mk() for k in on}
    for k, enable in on.items():
        enable(full)
        enable(one[k])
    tstats = {"full": [], "one": []}
    dstats = {"full": [], "one": []}
    for k in range(STEPS):
        a, b = getattr(plain, mode)(), getattr(full, mode)()
        for g in one.values():
            getattr(g, mode)()
        # (the tracers' intervals of a step are dropped by the next one: read per step, as the per-feature test does)
        tstats["full"].append(full.tracer_stats())
        tstats["one"].append(one["tracers"].tracer_stats())
        dstats["full"].append(full.derived())
        dstats["one"].append(one["derived"].derived())
        plain.fields()   # (settles a deferred correction, as derived() did on the other: see the module's docstring)
        assert [b[q] for q in STEP_KEYS] == [a[q] for q in STEP_KEYS], (k, a, b)
        if mode == "step" or k > 0:
            assert [b[q] for q in MONITOR] == [a[q] for q in MONITOR], (k, a, b)
    if mode == "step_async":
        assert full.monitor() == plain.monitor()
    # the flow: fields, and T where there is one
    state = lambda g: g.fields() + ((g.scalar(),) if scalar else ())
    for x, y, what in zip(state(plain), state(full), ("u", "v", "phi", "T")):
        assert np.array_equal(x, y), f"the observers changed {what}"
    # tracers
    for f, o in zip(tstats["full"], tstats["one"]):
        assert f["n_kernels"] == o["n_kernels"] == 1 and f["t_kernel_ms"] > 0.0 and o["t_kernel_ms"] > 0.0
        assert all(f[q] == o[q] for q in ("n", "live", "exited", "stuck", "age_max")), (f, o)
    again = full.tracer_stats()
    assert again["n_kernels"] == 0 and again["t_kernel_ms"] == 0.0 and again["n"] == 100
    tf, to = full.tracers(), one["tracers"].tracers()
    for q in ("x", "y", "age", "state"):
        assert np.array_equal(tf[q], to[q]), q
    assert np.any(tf["x"] != xs) and tf["live"] == 100
    # running statistics: every=2 -> steps 0, 2, 4, 6
    sf, so = full.average_stats(), one["avg"].average_stats()
    assert sf["n_kernels"] == so["n_kernels"] > 0 and sf["t_kernel_ms"] > 0.0 and so["t_kernel_ms"] > 0.0
    assert (sf["n"], sf["steps"]) == (so["n"], so["steps"]) == (4, STEPS)
    again = full.average_stats()
    assert again["n_kernels"] == 0 and again["t_kernel_ms"] == 0.0 and again["n"] == 4
    af, ao = full.averages(), one["avg"].averages()
    want = {"u", "v", "p", "uu", "vv", "uv", "pp", "n"} | ({"T", "TT", "uT", "vT"} if scalar else set())
    assert set(af) == set(ao) == want
    for q in sorted(want - {"n"}):
        assert np.array_equal(af[q], ao[q]), q
    assert af["uu"].any()
    # wall loads: every=3 -> steps 0, 3, 6
    lf, lo = full.load_stats(), one["loads"].load_stats()
    assert lf["n_kernels"] == lo["n_kernels"] > 0 and lf["t_kernel_ms"] > 0.0 and lo["t_kernel_ms"] > 0.0
    assert (lf["total"], lf["held"], lf["steps"]) == (lo["total"], lo["held"], lo["steps"]) == (3, 3, STEPS)
    again = full.load_stats()
    assert again["n_kernels"] == 0 and again["t_kernel_ms"] == 0.0 and again["total"] == 3
    (hf, rf), (ho, ro) = full.load_history(), one["loads"].load_history()
    assert hf.tolist() == ho.tolist() == [0, 3, 6] and np.array_equal(rf, ro) and rf[1:].any()
    # derived fields, after every step
    for k, (f, o) in enumerate(zip(dstats["full"], dstats["one"])):
        assert f["n_kernels"] == o["n_kernels"] > 0 and f["t_kernel_ms"] > 0.0 and o["t_kernel_ms"] > 0.0
        for q in DERIVED_PLANES:
            assert np.array_equal(f[q], o[q]), (k, q)
        assert [f[q] for q in DERIVED_SUMS] == [o[q] for q in DERIVED_SUMS], (k, f, o)
    for g in (plain, full, *one.values()):
        g.close()
