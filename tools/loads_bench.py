#!/usr/bin/env python3
"""Measure the wall loads on the cavity ("Wall loads"): prints one JSON line.

Default: the sampling kernels' dispatch-stamped time.  One solver with timing == 1, warm-up + synchronous steps at
every = 1, so each step carries one sample of two launches (k_load_faces over the 4 n boundary faces, k_load_edges);
ns_load_stats.t_kernel_ms per sample, next to K5's time from the same steps.

--step-cost: ns_step_async in the driver's form (steps back to back, one ns_monitor at the end) with the loads off,
every = 1 and every = 10, three alternating windows each: ms per step.

--headline PARENT_LIB: bench.py --gpus 1 --steps S --warmup W with this tree's library and with PARENT_LIB (a build of
the parent commit's library, selected through NSGPU_LIB), alternating, --rounds times each, one process per run: the
headline MLUPS of both.  With the loads off no launch changes, so the two spreads should overlap.

Needs the GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernels(nsa, a):
    n = a.n
    s = nsa.GpuSolver(nsa.cavity(n), nsa.cavity_dt(n), a.re, device=0, timing=True)
    s.enable_loads(every=1, capacity=16)
    tl, k5 = [], []
    for it in range(a.warmup + a.steps):
        st = s.step()
        ls = s.load_stats()
        if it < a.warmup or ls["n_kernels"] != 2 or st["n_k5_kernels"] != 1:
            continue
        tl.append(ls["t_kernel_ms"])
        k5.append(st["t_k5_kernel_ms"])
    s.close()
    if not tl:
        raise SystemExit("no timed samples")
    return {"faces": 4 * n, "sample_us": statistics.median(tl) * 1e3, "min_us": min(tl) * 1e3, "max_us": max(tl) * 1e3,
            "k5_us": statistics.median(k5) * 1e3}


def step_cost(nsa, a):
    n = a.n
    modes = {"off": 0, "every1": 1, "every10": 10}
    solvers = {}
    for name, every in modes.items():
        s = nsa.GpuSolver(nsa.cavity(n), nsa.cavity_dt(n), a.re, device=0)
        if every:
            s.enable_loads(every=every, capacity=64)
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


def headline(a):
    """bench.py's own result line, this tree's library and the parent's in turn (a fresh process each)."""
    out = {"this": [], "parent": []}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup)]
    for _ in range(a.rounds):
        for name in ("parent", "this"):
            env = dict(os.environ)
            env.pop("NSGPU_LIB", None)
            if name == "parent":
                env["NSGPU_LIB"] = os.path.abspath(a.headline)
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.run_timeout, cwd=ROOT)
            if r.returncode != 0:    # (nothing more on the GPU after a failed run)
                raise SystemExit(f"bench.py ({name}) exited with {r.returncode}:\n{r.stderr[-2000:]}")
            line = [l for l in r.stdout.splitlines() if l.startswith("{") and '"value"' in l][-1]
            out[name].append(json.loads(line)["value"])
            print(f"{name}: {out[name][-1]:.0f} MLUPS", file=sys.stderr, flush=True)
    return {"headline_mlups": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--re", type=float, default=1000.0)
    ap.add_argument("--step-cost", action="store_true")
    ap.add_argument("--headline", metavar="PARENT_LIB", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--run-timeout", type=float, default=200.0)
    a = ap.parse_args()
    out = {"n": a.n, "steps": a.steps, "warmup": a.warmup}
    if a.headline:
        out.update(headline(a))
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("loads_bench.py needs the GPU")
        import navierstokessolver_amd as nsa
        if a.step_cost:
            out.update(step_cost(nsa, a))
        else:
            out.update(kernels(nsa, a))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
