"""GPU: what the step's kernel timing reports (ns_stats.t_* / n_*, the figures bench.py prints per kernel).

Every solve path's timed kernels are pinned by their COUNTS, which are deterministic (the arithmetic of a run is
fixed): tests/golden/timing_counts.json, recorded by tests/golden/make_timing_counts.py (its CASES: 3 step() + 3
step_async() each, every path that times something).  A run with timing=True must reproduce the record exactly,
report a positive, finite time on exactly the lines it counted, and leave the computation untouched (timing=False:
bit-identical fields, the same iteration counts and monitors)."""
import importlib.util
import json
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_timing_counts", os.path.join(GOLDEN, "make_timing_counts.py"))
mtc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mtc)
RECORD = json.load(open(os.path.join(GOLDEN, "timing_counts.json")))["cases"]


def test_record_covers_every_timing_line():
    """The committed record: a case per entry of CASES; every n_* counter non-zero somewhere, the band line as one
    and as two intervals, a two-field Helmholtz pass counted as 2 (make_timing_counts.coverage_gaps)."""
    assert sorted(RECORD) == sorted(mtc.CASES)
    assert mtc.coverage_gaps(RECORD) == []


@pytest.mark.parametrize("name", list(mtc.CASES))
def test_timing_counts_and_times(gpu, name):
    case = mtc.CASES[name]
    st, srhs, mon, fields = mtc.run_case(gpu, case, True)
    got = mtc.record(st, srhs)
    print(name, [[s[k] for k in mtc.KEYS] for s in got["steps"]], srhs)
    # 1. the counts are the record's
    assert got == RECORD[name]
    # 2. a time on exactly the lines that counted, all finite
    for k, s in enumerate(st):
        for t, n in mtc.LINES:
            assert math.isfinite(s[t]) and (s[t] > 0) == (s[n] > 0), (k, t, s[t], n, s[n])
    # 3. timing does not touch the computation
    st0, srhs0, mon0, fields0 = mtc.run_case(gpu, case, False)
    key = ("it_u", "it_v", "it_phi", "umin", "umax", "vmin", "vmax")
    for a, b in zip(st, st0):
        assert all(a[q] == b[q] or (math.isnan(a[q]) and math.isnan(b[q])) for q in key), (a, b)
        assert all(b[n] == 0 and b[t] == 0.0 for t, n in mtc.LINES)
    assert mon == mon0
    for a, b in zip(fields, fields0):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("fn", ["time_poisson", "time_poisson_fp32"])
def test_time_poisson_sum_and_span(gpu, fn):
    """ns_time_poisson*: the average is the per-interval sum over the sweeps, and the span from the first sweep's
    start to the last one's end cannot be (much) shorter than that sum -- 0.5: the two are measured by different
    event pairs, a bound on a gross error (a span over the wrong events), not on overhead."""
    n, iters = 256, 20
    js = gpu.GpuSolver(gpu.cavity(n), 1.0 / (8 * n), 1000.0, poisson=gpu.NS_POISSON_JACOBI, omega=1.0)
    js.fill_random(0x5EED)
    for _ in range(2):   # (the second call reuses the first one's events)
        r = getattr(js, fn)(3, iters)
        assert all(math.isfinite(float(v)) for v in r.values()), r
        assert r["avg_ms"] > 0
        assert abs(r["total_ms"] - r["avg_ms"] * iters) <= 1e-12 * r["total_ms"]
        assert r["span_ms"] >= 0.5 * r["total_ms"]
    js.close()
