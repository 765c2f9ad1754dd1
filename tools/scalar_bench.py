#!/usr/bin/env python3
"""Measure the passive scalar on the cavity ("Passive scalar"): prints one JSON line.

  * k_rhs_t against K1: both kernels' own durations (the dispatch stamps ns_stats.t_rhs_kernel_ms and
    ns_scalar_stats.t_rhs_kernel_ms report, timing == 1) over synchronous steps of ONE solver, so the two
    run on the same fields in the same session; achieved bytes/s at their algorithmic byte counts
    (K1 64 B/cell: u, v, cu0, cv0 read, cu, cv, ru, rv written; k_rhs_t 48: u, v, T, cT0 read, cT, rT
    written) and as a share of the HBM peak;
  * the step cost: ms/step of the driver's form (ns_step_async, the last monitor inside the timed
    window, timing off) with and without a scalar, the two solvers alternating over `--reps` windows.

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
K1_BYTES, RHS_T_BYTES = 64, 48
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
        raise SystemExit("scalar_bench.py needs the GPU")
    import navierstokessolver_amd as nsa
    n, dt = a.n, nsa.cavity_dt(a.n)
    cells = n * n

    def make(scalar, timing):
        s = nsa.GpuSolver(nsa.cavity(n), dt, a.re, device=0, timing=timing)
        if scalar:
            s.enable_scalar(a.pe, LID)
        return s

    # ---- kernel times: synchronous steps of one timed solver
    s = make(True, True)
    for _ in range(a.warmup):
        s.step()
    k1, kt, its = [], [], []
    for _ in range(a.steps):
        st = s.step()
        ss = s.scalar_stats()
        if st["n_rhs_kernels"] == 1 and ss["n_rhs_kernels"] == 1:
            k1.append(st["t_rhs_kernel_ms"])
            kt.append(ss["t_rhs_kernel_ms"])
        its.append(ss["it_t"])
    s.close()
    if not k1:
        raise SystemExit("no timed kernel pairs")
    m1, mt = statistics.median(k1), statistics.median(kt)
    r1, rt = K1_BYTES * cells / (m1 * 1e-3), RHS_T_BYTES * cells / (mt * 1e-3)

    # ---- step cost: the driver's form, the two solvers alternating
    pair = {False: make(False, False), True: make(True, False)}
    ms = {False: [], True: []}
    for sv in pair.values():
        for _ in range(a.warmup):
            sv.step_async()
        sv.monitor()
    for _ in range(a.reps):
        for scalar, sv in pair.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                sv.step_async()
            sv.monitor()
            torch.cuda.synchronize()
            ms[scalar].append((time.perf_counter() - t0) / a.steps * 1e3)
    for sv in pair.values():
        sv.close()
    out = {
        "n": n, "steps": a.steps, "reps": a.reps, "pe": a.pe,
        "k1_us": {"median": m1 * 1e3, "min": min(k1) * 1e3, "max": max(k1) * 1e3, "bytes_per_cell": K1_BYTES,
                  "GBs": r1 / 1e9, "hbm_frac": r1 / HBM_PEAK},
        "k_rhs_t_us": {"median": mt * 1e3, "min": min(kt) * 1e3, "max": max(kt) * 1e3, "bytes_per_cell": RHS_T_BYTES,
                       "GBs": rt / 1e9, "hbm_frac": rt / HBM_PEAK},
        "k_rhs_t_over_k1_rate": rt / r1,
        "scalar_sweeps_per_step": statistics.mean(its),
        "ms_per_step_without": {"median": statistics.median(ms[False]), "all": ms[False]},
        "ms_per_step_with": {"median": statistics.median(ms[True]), "all": ms[True]},
    }
    out["scalar_ms_per_step"] = out["ms_per_step_with"]["median"] - out["ms_per_step_without"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
