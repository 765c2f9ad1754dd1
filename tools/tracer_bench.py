#!/usr/bin/env python3
"""Measure the tracer kernel inside the time step ("Tracers"): prints one JSON line.

The n x n cavity after `--spinup` steps, `--particles` tracers (default 2^22: one in every fourth cell of 4096^2, at
0.3 of the cell), seeded twice in ONE solver: "ordered" -- in cell order, i outer and j inner like the field planes, so
a wave's 64 particles gather from neighbouring columns of one row pair -- and "permuted" -- the same positions in a
random order, so every particle gathers from its own corner of the planes.  Per order, over `--steps` synchronous steps:
the particle kernel's own duration (the dispatch stamp ns_tracer_stats.t_kernel_ms reports, timing == 1) as median and
range, ns per particle-step, and the rate of its streamed bytes -- 44 B read + 44 B written per live particle (x, y,
wu, wv, age and the state word; a live particle past its first step does not rewrite the word, which the count
ignores) -- with the eight gathered field values (4 of u, 4 of v: 64 B per particle if none is shared) counted
separately, not in the rate.  The step's wall time with and without the particles is reported as a cost.

Needs the GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_BYTES, GATHER_BYTES = 88, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--particles", type=int, default=1 << 22)
    ap.add_argument("--spinup", type=int, default=200)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--re", type=float, default=1000.0)
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tracer_bench.py needs the GPU")
    import navierstokessolver_amd as nsa
    n, dt = a.n, nsa.cavity_dt(a.n)
    stride = max(1, int(round((n * n / a.particles) ** 0.5)))
    ii, jj = np.meshgrid(np.arange(0, n, stride), np.arange(0, n, stride), indexing="ij")
    xs, ys = ((ii.ravel() + 0.3) / n)[:a.particles], ((jj.ravel() + 0.3) / n)[:a.particles]
    npart = xs.size
    s = nsa.GpuSolver(nsa.cavity(n), dt, a.re, device=0, timing=True)
    for _ in range(a.spinup):
        s.step_async()
    s.monitor()

    def steps_ms(collect):
        """wall time per synchronous step, and the particle kernel's durations if there are particles"""
        tk = []
        t0 = time.perf_counter()
        for _ in range(a.steps):
            s.step()
            if collect:
                st = s.tracer_stats()
                if st["n_kernels"] == 1:
                    tk.append(st["t_kernel_ms"])
        return (time.perf_counter() - t0) * 1e3 / a.steps, tk, (st if collect else None)

    off_ms, _, _ = steps_ms(False)
    s.enable_tracers(npart)
    out = {"n": n, "particles": npart, "steps": a.steps, "spinup": a.spinup, "step_ms_off": off_ms}
    perm = np.random.default_rng(1).permutation(npart)
    for name, order in (("ordered", None), ("permuted", perm)):
        s.reset_tracers()
        s.add_tracers(xs if order is None else xs[order], ys if order is None else ys[order])
        on_ms, tk, st = steps_ms(True)
        if not tk:
            raise SystemExit("no timed particle kernel")
        m = statistics.median(tk)
        out[name] = {"kernel_us": {"median": m * 1e3, "min": min(tk) * 1e3, "max": max(tk) * 1e3},
                     "ns_per_particle_step": m * 1e6 / npart,
                     "streamed_GBs": STREAM_BYTES * st["live"] / (m * 1e-3) / 1e9,
                     "streamed_bytes_per_particle": STREAM_BYTES, "gathered_bytes_per_particle": GATHER_BYTES,
                     "step_ms_on": on_ms, "step_cost_ms": on_ms - off_ms,
                     "live": st["live"], "exited": st["exited"], "stuck": st["stuck"], "age_max": st["age_max"]}
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
