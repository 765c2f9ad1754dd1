#!/usr/bin/env python3
"""Measure the running flow statistics on the cavity ("Flow statistics"): prints one JSON line.

Default: k_moments against K5.  Per instantiation one solver with timing == 1, warm-up + synchronous steps at
every = 1, so each step carries one sample; the dispatch-stamped durations ns_avg_stats.t_kernel_ms and
ns_stats.t_k5_kernel_ms come from the same steps of the same session.  With pressure the statistics' line is two
kernels -- the derived pass storing P (24 + 8 B/cell) and k_moments --; the derived pass alone is timed on the same
state by one ns_derive asking for P only, and taken off.  Achieved bytes/s at the algorithmic counts (means only 48
B/cell, with second moments 96, + 40 with pressure, + 72 with the scalar) as a share of K5's rate (40 B/cell; the
bar: 0.85).

--step-cost: ns_step_async in the driver's form (steps back to back, one ns_monitor at the end) with the averages
off, every = 1 and every = 10 (u, v with second moments), three alternating windows each: ms per step.

Needs the GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K5_BYTES = 40
S_WALLS = [("zerograd",), ("dirichlet", 1.0), ("zerograd",), ("dirichlet", 0.0)]
# name: (second, pressure, scalar, k_moments' bytes per cell)
CASES = {
    "means": (False, False, False, 48),
    "second": (True, False, False, 96),
    "means+p": (False, True, False, 48 + 8 + 16),
    "second+p": (True, True, False, 96 + 40),
    "means+T": (False, False, True, 48 + 8 + 16),
    "second+T": (True, False, True, 96 + 72),
    "means+p+T": (False, True, True, 48 + 2 * (8 + 16)),
    "second+p+T": (True, True, True, 96 + 40 + 72),
}


def kernels(nsa, a, name):
    second, pressure, scalar, nbytes = CASES[name]
    n = a.n
    s = nsa.GpuSolver(nsa.cavity(n), nsa.cavity_dt(n), a.re, device=0, timing=True)
    if scalar:
        s.enable_scalar(71.0, S_WALLS)
    s.enable_averages(every=1, second=second, pressure=pressure, scalar=scalar)
    k5, tm, td = [], [], []
    for it in range(a.warmup + a.steps):
        st = s.step()
        av = s.average_stats()
        d = s.derived(p=True, vort=False, div=False, psi=False) if pressure else {"t_kernel_ms": 0.0, "n_kernels": 0}
        if it < a.warmup or st["n_k5_kernels"] != 1 or av["n_kernels"] != (2 if pressure else 1):
            continue
        k5.append(st["t_k5_kernel_ms"])
        td.append(d["t_kernel_ms"])
        tm.append(av["t_kernel_ms"] - d["t_kernel_ms"])
    s.close()
    if not k5:
        raise SystemExit(f"{name}: no timed kernel pairs")
    cells = n * n
    rate = lambda t, b: b * cells / (statistics.median(t) * 1e-3)
    out = {"bytes_per_cell": nbytes, "moments_us": statistics.median(tm) * 1e3, "min_us": min(tm) * 1e3,
           "max_us": max(tm) * 1e3, "GBs": rate(tm, nbytes) / 1e9, "k5_us": statistics.median(k5) * 1e3,
           "k5_GBs": rate(k5, K5_BYTES) / 1e9}
    out["over_k5_rate"] = out["GBs"] / out["k5_GBs"]
    if pressure:
        out["derived_p_us"] = statistics.median(td) * 1e3
    return out


def step_cost(nsa, a):
    n = a.n
    modes = {"off": 0, "every1": 1, "every10": 10}
    solvers = {}
    for name, every in modes.items():
        s = nsa.GpuSolver(nsa.cavity(n), nsa.cavity_dt(n), a.re, device=0)
        if every:
            s.enable_averages(every=every, second=True)
        for _ in range(a.warmup):
            s.step_async()
        s.monitor()
        solvers[name] = s
    out = {k: [] for k in modes}
    for _ in range(3):
        for name, s in solvers.items():
            t0 = time.perf_counter()
            for _ in range(a.steps):
                s.step_async()
            s.monitor()
            out[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    for s in solvers.values():
        s.close()
    return {"ms_per_step": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--re", type=float, default=1000.0)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--step-cost", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("avg_bench.py needs the GPU")
    import navierstokessolver_amd as nsa
    out = {"n": a.n, "steps": a.steps, "warmup": a.warmup}
    if a.step_cost:
        out.update(step_cost(nsa, a))
    else:
        out["cases"] = {name: kernels(nsa, a, name) for name in a.cases.split(",")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
