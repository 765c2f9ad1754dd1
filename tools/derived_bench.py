#!/usr/bin/env python3
"""Measure ns_derive's cell pass on the cavity ("Derived fields"): prints one JSON line.

k_derived_s against K5, the same strip walk: both kernels' own durations (the dispatch stamps ns_stats.t_k5_kernel_ms
and ns_derived_stats.t_kernel_ms report, timing == 1) over synchronous steps of ONE solver, so they run on the same
fields in the same session -- after each step one ns_derive storing P, vorticity and divergence (24 B/cell read + 24
written = 48) and one stats-only (24); K5 moves 40 B/cell (phi, u*, v* read, u, v written).  Achieved bytes/s at these
algorithmic counts, as a share of the HBM peak and of K5's rate (the bar: 0.85, the scalar right-hand side's).

--psi N: no timing, just N calls asking for psi alone after a few steps -- run it under a kernel trace
(rocprofv3 --kernel-trace --stats; tools/trace_summary.py) to read k_psi_base's and k_psi_scan's durations, which
ns_derived_stats does not carry.

Needs the GPU; there is no fallback."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12   # bytes / s (bench.py's HBM_PEAK_GBS)
K5_BYTES, FULL_BYTES, STATS_BYTES = 40, 48, 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--re", type=float, default=1000.0)
    ap.add_argument("--psi", type=int, default=0)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("derived_bench.py needs the GPU")
    import navierstokessolver_amd as nsa
    L = nsa._lib
    n, dt = a.n, nsa.cavity_dt(a.n)
    cells = n * n
    s = nsa.GpuSolver(nsa.cavity(n), dt, a.re, device=0, timing=not a.psi)
    for _ in range(a.warmup):
        s.step()
    dp = ctypes.POINTER(ctypes.c_double)
    if a.psi:
        psi = np.empty((n + 1, n + 1))
        out = L.NsDerived(None, None, None, psi.ctypes.data_as(dp))
        st = L.NsDerivedStats()
        for _ in range(a.psi):
            L.check(L.lib().ns_derive(s._h, ctypes.byref(out), ctypes.byref(st)))
        print(json.dumps({"n": n, "psi_calls": a.psi, "psi_min": st.psi_min, "psi_max": st.psi_max}))
        s.close()
        return
    planes = [np.empty((n, n)) for _ in range(3)]   # (one set of host buffers for every call)
    full = L.NsDerived(*[p.ctypes.data_as(dp) for p in planes], None)
    k5, tf, ts = [], [], []
    last = None
    for _ in range(a.steps):
        st = s.step()
        d3, d0 = L.NsDerivedStats(), L.NsDerivedStats()
        L.check(L.lib().ns_derive(s._h, ctypes.byref(full), ctypes.byref(d3)))
        L.check(L.lib().ns_derive(s._h, None, ctypes.byref(d0)))
        if st["n_k5_kernels"] == 1 and d3.n_kernels == 1 and d0.n_kernels == 1:
            k5.append(st["t_k5_kernel_ms"])
            tf.append(d3.t_kernel_ms)
            ts.append(d0.t_kernel_ms)
        last = d3
    s.close()
    if not k5:
        raise SystemExit("no timed kernel triples")

    def line(t, nbytes):
        m = statistics.median(t)
        r = nbytes * cells / (m * 1e-3)
        return {"median": m * 1e3, "min": min(t) * 1e3, "max": max(t) * 1e3, "bytes_per_cell": nbytes, "GBs": r / 1e9,
                "hbm_frac": r / HBM_PEAK}

    out = {"n": n, "steps": a.steps, "k5_us": line(k5, K5_BYTES), "derived_full_us": line(tf, FULL_BYTES),
           "derived_stats_us": line(ts, STATS_BYTES)}
    out["full_over_k5_rate"] = out["derived_full_us"]["GBs"] / out["k5_us"]["GBs"]
    out["stats_over_k5_rate"] = out["derived_stats_us"]["GBs"] / out["k5_us"]["GBs"]
    out["last"] = {k: getattr(last, k) for k in ("ke", "enstrophy", "div_l2", "div_max", "cfl")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
