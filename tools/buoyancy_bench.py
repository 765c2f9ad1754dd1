#!/usr/bin/env python3
"""Measure Boussinesq buoyancy on the cavity ("Buoyancy"): prints one JSON line.

  * k_rhs_t plain against its buoyant variants (y forced: 80 B/cell; x and y: 112 B/cell): each kernel's own
    duration (the dispatch stamps ns_scalar_stats.t_rhs_kernel_ms reports, timing == 1) over synchronous
    steps of one solver per variant, the solvers stepping in turn so all run in the same session; achieved
    bytes/s at the algorithmic byte counts and the buoyant rates as a share of the plain kernel's;
  * the step cost: ms/step of the driver's form (ns_step_async, the last monitor inside the timed window,
    timing off) with a scalar, buoyancy off against on (y forced), alternating over `--reps` windows.

Needs the GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes / s (bench.py's HBM_PEAK_GBS)
BYTES = {"plain": 48, "y": 80, "xy": 112}   # u, v, T, cT0 read, cT, rT written; + r, c read and written per component
FORCE = {"plain": None, "y": dict(by=1.0, tref=0.5), "xy": dict(by=1.0, bx=0.25, tref=0.5)}
LID = [("zerograd",), ("dirichlet", 1.0), ("zerograd",), ("dirichlet", 0.0)]   # hot lid, cold floor (edges W, N, E, S)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--re", type=float, default=1000.0)
    ap.add_argument("--pe", type=float, default=710.0)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("buoyancy_bench.py needs the GPU")
    import navierstokessolver_amd as nsa
    n, dt = a.n, nsa.cavity_dt(a.n)
    cells = n * n

    def make(force, timing):
        s = nsa.GpuSolver(nsa.cavity(n), dt, a.re, device=0, timing=timing)
        s.enable_scalar(a.pe, LID)
        if force:
            s.set_buoyancy(**force)
        return s

    # ---- kernel times: synchronous steps of one timed solver per variant, in turn
    sv = {k: make(f, True) for k, f in FORCE.items()}
    for _ in range(a.warmup):
        for s in sv.values():
            s.step()
    t = {k: [] for k in sv}
    its = {k: [] for k in sv}
    for _ in range(a.steps):
        for k, s in sv.items():
            st = s.step()
            ss = s.scalar_stats()
            if ss["n_rhs_kernels"] == 1:
                t[k].append(ss["t_rhs_kernel_ms"])
            its[k].append(st["it_u"])
    for s in sv.values():
        s.close()
    if not all(t.values()):
        raise SystemExit("no timed kernels")
    out = {"n": n, "steps": a.steps, "reps": a.reps, "pe": a.pe, "kernel_us": {}}
    rate = {}
    for k, v in t.items():
        m = statistics.median(v)
        rate[k] = BYTES[k] * cells / (m * 1e-3)
        out["kernel_us"][k] = {"median": m * 1e3, "min": min(v) * 1e3, "max": max(v) * 1e3, "bytes_per_cell": BYTES[k],
                               "GBs": rate[k] / 1e9, "hbm_frac": rate[k] / HBM_PEAK,
                               "helm_sweeps_per_step": statistics.mean(its[k])}
    out["y_over_plain_rate"] = rate["y"] / rate["plain"]
    out["xy_over_plain_rate"] = rate["xy"] / rate["plain"]

    # ---- step cost: the driver's form, buoyancy off and on alternating
    pair = {"off": make(None, False), "on": make(FORCE["y"], False)}
    ms = {k: [] for k in pair}
    for s in pair.values():
        for _ in range(a.warmup):
            s.step_async()
        s.monitor()
    for _ in range(a.reps):
        for k, s in pair.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                s.step_async()
            s.monitor()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
    for s in pair.values():
        s.close()
    out["ms_per_step_off"] = {"median": statistics.median(ms["off"]), "all": ms["off"]}
    out["ms_per_step_on"] = {"median": statistics.median(ms["on"]), "all": ms["on"]}
    out["buoyancy_ms_per_step"] = out["ms_per_step_on"]["median"] - out["ms_per_step_off"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
