"""Record the per-step kernel-timing COUNTS of libnsgpu.so (tests/golden/timing_counts.json) -- needs the GPU; run
from the repo root:
    python tests/golden/make_timing_counts.py
Each case of CASES runs 3 step() and then 3 step_async() calls plus monitor() with timing=True, through the public
Python API only, and stores per step every n_* timing counter of ns_stats, n_checks, it_u and it_phi (scalar cases:
scalar_stats()["n_rhs_kernels"] too).  The arithmetic of a run is fixed, so the counts are deterministic: the file
pins which kernels every solve path times (tests/test_gpu_timing.py compares a run against it and imports CASES /
run_case from here).  Regenerate it only with a change that means to alter what is timed."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "..", ".."), os.path.join(HERE, "..", "..", "oracle"), os.path.join(HERE, "..")):
    if os.path.abspath(p) not in sys.path:
        sys.path.insert(0, os.path.abspath(p))

OUT = os.path.join(HERE, "timing_counts.json")
# ns_stats' timing lines: (elapsed-time field, its counter); the direct solve's three phases share n_fps_solves
LINES = [("t_poisson_kernel_ms", "n_poisson_kernels"), ("t_restrict_kernel_ms", "n_restrict_kernels"),
         ("t_cycle_kernel_ms", "n_cycle_kernels"), ("t_guess_kernel_ms", "n_guess_kernels"),
         ("t_helm_kernel_ms", "n_helm_kernels"), ("t_rhs_kernel_ms", "n_rhs_kernels"),
         ("t_band_kernel_ms", "n_band_kernels"), ("t_k5_kernel_ms", "n_k5_kernels"),
         ("t_fps_dct_ms", "n_fps_solves"), ("t_fps_tri_ms", "n_fps_solves"), ("t_fps_idct_ms", "n_fps_solves")]
COUNTERS = sorted({n for _, n in LINES})
KEYS = COUNTERS + ["n_checks", "it_u", "it_phi"]

BC_CHANNEL = [(0, 1.0), (2, 0.0), (4, 0.0), (2, 0.0)]   # inlet W, walls N / S, NEUMANN outflow E
S_CAVITY = [("zerograd",), ("dirichlet", 1.0), ("zerograd",), ("dirichlet", 0.0)]   # hot lid, cold floor
MG = {"NSGPU_FPS": "0"}
STREAM = dict(MG, NSGPU_PAIR_MIN_CELLS="0")


def _cavity(n, env=None, re=1000.0, **kw):
    return dict(grid=("cavity", n), dt=1.0 / (8 * n), re=re, env=env or {}, kw=kw)


# name -> case (grid, dt, Re, the knobs set at ns_create, GpuSolver keywords); the comment: the path it is here for
CASES = {
    "cavity128": _cavity(128),                                          # fused direct solve, K1, K5 (normal, deferred)
    "cavity256": _cavity(256),                                          # ... and the wall bands (two launches)
    "cavity128_markers": _cavity(128, {"NSGPU_EXT_TIMING": "0"}),        # marker events instead of dispatch stamps
    "cavity256_markers": _cavity(256, {"NSGPU_EXT_TIMING": "0"}),
    "cavity256_unfused": _cavity(256, {"NSGPU_FPS_FUSE": "0"}),          # the direct solve's own forward transform
    "cavity256_passes3": _cavity(256, {"NSGPU_FPS_PASSES": "3"}),
    "dense96x80": dict(grid=("rect", 96, 80, dict(yratio=1.02)), dt=1.0 / 768, re=400.0, env={}, kw={}),   # rocBLAS
    "cavity256_mg": _cavity(256, MG),                                   # multigrid, LDS-tiled finest level
    "cavity256_mg_stream": _cavity(256, STREAM),                         # streamed finest level: n_cycle_kernels
    "cavity256_mg_gin": _cavity(256, dict(STREAM, NSGPU_GIN="1")),       # n_guess_kernels
    "cavity64_rbsor": _cavity(64, poisson="NS_POISSON_RBSOR"),            # pois_solve
    "cavity64_jacobi": _cavity(64, poisson="NS_POISSON_JACOBI"),
    "channel256x64_krylov": dict(grid=("rect", 256, 64, dict(lx=4.0, ly=1.0, bc=BC_CHANNEL)), dt=1.0 / 512, re=100.0,
                                 env={"NSGPU_FPS_OUTFLOW": "0"}, kw={}),   # BiCGStab, timed V-cycle preconditioner
    "cavity256_band6": _cavity(256, {"NSGPU_BAND6": "1"}),               # the band pair as one interval
    "cavity256_re200": _cavity(256, re=200.0),                          # 3-sweep batches: ONE two-field launch
    "cavity256_re200_split": _cavity(256, {"NSGPU_HELM_UV": "0"}, re=200.0),   # ... as two one-field launches
    "cavity128_scalar": dict(_cavity(128), scalar=dict(pe=100.0)),       # the scalar's right-hand side
    "cavity128_buoyant": dict(_cavity(128), scalar=dict(pe=100.0, by=1.0)),
    "lshape": dict(grid=("polygon", "lshape"), dt=1.0 / 1024, re=200.0, env={}, kw={}),   # masked: lines that stay zero
    "cavity256_loopback": _cavity(256, {"NSGPU_RCCL_LOOPBACK": "1"}),    # split launches under the dispatch stamp
    "slab256_mg": _cavity(256, dict(MG, NSGPU_RCCL_LOOPBACK="1", NSGPU_VIRTUAL_ITERS="4:2,6:3"), rank=1, nranks=2),
    "slab256_direct": _cavity(256, {"NSGPU_RCCL_LOOPBACK": "1", "NSGPU_VIRTUAL_ITERS": "4:1"}, rank=1, nranks=2),
}
# the knobs the cases set: cleared for every other case, so that a caller's environment cannot leak in
KNOBS = sorted({k for c in CASES.values() for k in c["env"]})


def make_grid(nsa, spec):
    if spec[0] == "cavity":
        return nsa.cavity(spec[1])
    if spec[0] == "rect":
        return nsa.rectangle(spec[1], spec[2], **spec[3])
    from oracle import OGrid
    from polygons import ALL
    P = ALL[spec[1]]
    og = OGrid(P["vertices"], P["xspec"], P["yspec"], P["bc"])
    return nsa.polygon(P["vertices"], og.hx, og.hy, P["bc"])


def run_case(nsa, case, timing):
    """3 step() + 3 step_async() + monitor(): (per-step stats dicts, scalar n_rhs_kernels per step or None, monitor,
    the final fields).  The knobs are read at ns_create; the environment is restored before returning."""
    saved = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(case["env"])
        kw = dict(case["kw"])
        if "poisson" in kw:
            kw["poisson"] = getattr(nsa, kw["poisson"])
        gs = nsa.GpuSolver(make_grid(nsa, case["grid"]), case["dt"], case["re"], device=0, timing=timing, **kw)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    sc = case.get("scalar")
    if sc:
        gs.enable_scalar(sc["pe"], S_CAVITY)
        if "by" in sc:
            gs.set_buoyancy(sc["by"])
    st, srhs = [], []
    for k in range(6):
        st.append(gs.step() if k < 3 else gs.step_async())
        if sc:
            srhs.append(gs.scalar_stats()["n_rhs_kernels"])
    mon = gs.monitor()
    fields = [a.copy() for a in gs.fields()] + ([gs.scalar().copy()] if sc else [])
    gs.close()
    return st, (srhs if sc else None), mon, fields


def record(st, srhs):
    r = {"steps": [{k: int(s[k]) for k in KEYS} for s in st]}
    if srhs is not None:
        r["scalar_n_rhs_kernels"] = [int(x) for x in srhs]
    return r


def coverage_gaps(rec):
    """What the case list must show (a list of complaints, empty when it does): every counter non-zero somewhere,
    the band line as one and as two intervals, a 3-sweep two-field Helmholtz launch counted as its two components."""
    steps = lambda name: rec[name]["steps"]
    every = [s for name in rec for s in steps(name)]
    gaps = [f"{c} is zero in every case" for c in COUNTERS if not any(s[c] > 0 for s in every)]
    bands = {s["n_band_kernels"] for s in every}
    if not {1, 2} <= bands:
        gaps.append(f"n_band_kernels takes {sorted(bands)}, not both 1 and 2")
    # helm_uv (the default): a batch of exactly 3 sweeps is ONE two-field launch, counted 2 -- the count of its
    # split form (NSGPU_HELM_UV=0: a launch per component)
    uv = [s for s in steps("cavity256_re200") if s["it_u"] == 3]
    if not uv or any(s["n_helm_kernels"] != 2 for s in uv):
        gaps.append("no 3-sweep two-field Helmholtz pass counted as 2 in cavity256_re200")
    if [s["n_helm_kernels"] for s in steps("cavity256_re200")] != [s["n_helm_kernels"] for s in steps("cavity256_re200_split")]:
        gaps.append("the two-field pass and its split form count differently")
    if not any(x > 0 for name in rec for x in rec[name].get("scalar_n_rhs_kernels", [])):
        gaps.append("scalar n_rhs_kernels is zero in every case")
    return gaps


def main():
    import navierstokessolver_amd as nsa
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    rec = {}
    for name, case in CASES.items():
        st, srhs, _, _ = run_case(nsa, case, True)
        rec[name] = record(st, srhs)
        print(name, [[s[k] for k in KEYS] for s in rec[name]["steps"]], srhs, flush=True)
    json.dump({"generator": "tests/golden/make_timing_counts.py", "keys": KEYS, "cases": rec}, open(out, "w"), indent=1)
    print("wrote", out)
    gaps = coverage_gaps(rec)
    if gaps:
        raise SystemExit("the case list does not cover the timing lines: " + "; ".join(gaps))


if __name__ == "__main__":
    main()
