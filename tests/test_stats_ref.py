"""CPU: the running flow statistics' restatement (tests/stats_ref.py) against the two-pass definition, its exact
cases and the time step's bookkeeping.

Tolerance: the project's 1e-12 of the plane's max (tried with this exact update on fields whose fluctuation is
comparable to their mean: <= 1e-15; with a mean 500 x the fluctuation 2e-13 -- the conditioning of the variance, not
of the update)."""
import numpy as np
import pytest

from stats_ref import KEYS, PAIRS, RunningStats, StepDriver, two_pass

SHAPE = (40, 70)


def rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def stack_of(n, seed):
    rng = np.random.default_rng(seed)
    # a mean of order 1 with a fluctuation of order 1 around it
    base = {k: rng.uniform(-1, 1, SHAPE) for k in "uvpT"}
    return {k: base[k] + rng.uniform(-1, 1, (n,) + SHAPE) for k in "uvpT"}


@pytest.mark.parametrize("n", [1, 2, 7, 12, 40])
def test_restatement_vs_two_pass(n):
    st = stack_of(n, 100 + n)
    rs = RunningStats(SHAPE, second=True, pressure=True, scalar=True)
    for k in range(n):
        rs.sample(**{q: st[q][k] for q in "uvpT"})
    got, ref = rs.result(), two_pass(st)
    assert got["n"] == n and sorted(got) == sorted(KEYS + ("n",))
    worst = 0.0
    for k in KEYS:
        if k in PAIRS and n == 1:
            assert not got[k].any(), k   # (a single sample: exactly 0; the reference's own 0 has no scale)
            continue
        e = rel(got[k], ref[k])
        worst = max(worst, e)
        assert e <= 1e-12, (k, e)
    print(f"n = {n}: worst relative deviation {worst:.2e}")


@pytest.mark.parametrize("flags", [(False, False, False), (True, False, False), (True, True, False),
                                   (True, False, True), (False, True, True)])
def test_planes_kept(flags):
    second, pressure, scalar = flags
    rs = RunningStats((3, 4), second=second, pressure=pressure, scalar=scalar)
    want = {"u", "v"} | ({"p"} if pressure else set()) | ({"T"} if scalar else set())
    if second:
        want |= {"uu", "vv", "uv"} | ({"pp"} if pressure else set()) | ({"TT", "uT", "vT"} if scalar else set())
    assert set(rs.result()) == want | {"n"}
    assert "up" not in rs.result() and "pT" not in rs.result()


def test_single_sample_is_exact():
    st = stack_of(1, 7)
    rs = RunningStats(SHAPE, pressure=True, scalar=True)
    rs.sample(**{q: st[q][0] for q in "uvpT"})
    r = rs.result()
    for q in "uvpT":
        assert np.array_equal(r[q], st[q][0]), q
    for k in PAIRS:
        assert not rs.S[k].any() and not r[k].any(), k


def test_constant_input_is_exact():
    st = stack_of(1, 8)
    rs = RunningStats(SHAPE, pressure=True, scalar=True)
    for _ in range(5):
        rs.sample(**{q: st[q][0] for q in "uvpT"})
    r = rs.result()
    assert r["n"] == 5
    for q in "uvpT":
        assert np.array_equal(r[q], st[q][0]), q
    for k in PAIRS:
        assert not rs.S[k].any() and not r[k].any(), k


def test_nothing_sampled_is_zero():
    r = RunningStats((3, 4)).result()
    assert r["n"] == 0 and all(not r[k].any() for k in ("u", "v", "uu", "vv", "uv"))


@pytest.mark.parametrize("every,nsteps,want", [(1, 7, [0, 1, 2, 3, 4, 5, 6]), (3, 7, [0, 3, 6]), (2, 10, [0, 2, 4, 6, 8]),
                                               (10, 7, [0])])
def test_every_bookkeeping(every, nsteps, want):
    rng = np.random.default_rng(9)
    states = [{q: rng.uniform(-1, 1, (5, 6)) for q in "uv"} for _ in range(nsteps + 1)]
    drv = StepDriver(RunningStats((5, 6)), every)
    for k in range(nsteps):
        drv.step(**states[k])
    assert drv.sampled == want and drv.steps == nsteps and drv.stats.n == len(want)
    ref = two_pass({q: np.stack([states[k][q] for k in want]) for q in "uv"})
    for k in ("u", "v", "uu", "vv", "uv"):
        if len(want) == 1 and k in PAIRS:
            continue
        assert rel(drv.stats.result()[k], ref[k]) <= 1e-12, k
    # the final state by hand: n + 1
    drv.sample_now(**states[nsteps])
    assert drv.stats.n == len(want) + 1 and drv.sampled[-1] is None
    ref = two_pass({q: np.stack([states[k][q] for k in want + [nsteps]]) for q in "uv"})
    for k in ("u", "v", "uu", "vv", "uv"):
        assert rel(drv.stats.result()[k], ref[k]) <= 1e-12, k
    # reset: the spin-up cut-off -- the count of steps starts again
    drv.reset()
    assert drv.stats.n == 0 and drv.steps == 0 and not drv.stats.result()["u"].any()
    drv.step(**states[1])
    assert drv.sampled == [0] and np.array_equal(drv.stats.result()["u"], states[1]["u"])
