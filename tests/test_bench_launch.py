"""bench.py --gpus N starts its own N ranks when no launcher set WORLD_SIZE (the
driver's `python3 bench.py --gpus N` form must reach every rank).  CPU: the probe hook
(NSBENCH_LAUNCH_PROBE) makes each rank report its rank / world and exit before any GPU call.
GPU: the whole N = 2 branch on one GPU through the host transport."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_self_launches_n_ranks():
    env = dict(os.environ, NSBENCH_LAUNCH_PROBE="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    # (--n and --re are abbreviations of torch.distributed.run options: they must reach the ranks)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--steps", "1", "--n", "512",
                        "--re", "100"], capture_output=True, text=True, env=env, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    # (the ranks share the child's stdout: their lines may interleave)
    probes = [json.loads(m) for m in re.findall(r"\{[^{}]*\}", r.stdout)]
    assert sorted(p["probe_rank"] for p in probes) == [0, 1, 2]
    assert all(p["world"] == 3 for p in probes)
    assert sorted(p["local_rank"] for p in probes) == [0, 1, 2]
    assert all(p["n"] == 512 and p["re"] == 100.0 for p in probes)


def test_bench_failed_rank_reports_and_exits_nonzero():
    """a rank that fails (an RCCL init or collective error raises NsError) prints a JSON
    error line and exits non-zero, and the job ends instead of leaving its peers hanging in a collective.
    CPU: NSBENCH_FAIL_RANK injects the failure on rank 1 before any GPU call; rank 0 is left waiting in
    the process-group set-up until torch.distributed.run tears it down."""
    env = dict(os.environ, NSBENCH_FAIL_RANK="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "NSBENCH_LAUNCH_PROBE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--n", "64"],
                       capture_output=True, text=True, env=env, timeout=240, cwd=ROOT)
    assert r.returncode != 0
    errs = [json.loads(m) for m in re.findall(r"\{[^{}]*\}", r.stdout)]
    assert any(e.get("error") and e.get("rank") == 1 and e.get("value") is None for e in errs), r.stdout[-2000:]


def test_bench_options_default_to_the_plain_run():
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def test_bench_dump_sample_is_fixed_and_within_budget(tmp_path):
    """--dump-outputs on planes larger than the budget: every plane at the same cells, which depend on the
    plane's shape alone (two runs, two builds: the same cells), float64, the files together below 64 MB;
    planes within the budget are written whole."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    import navierstokessolver_amd as nsa

    class Planes:
        def __init__(self, shape):
            self.shape = shape
            self.planes = {w: np.random.default_rng(w).standard_normal(shape)
                           for w in (nsa.NS_ARR_U, nsa.NS_ARR_V, nsa.NS_ARR_PHI)}

        def get(self, which):
            return self.planes[which]

    mon = {"umin": -0.25, "umax": 1.0, "vmin": -0.5, "vmax": 0.5}
    big = Planes((2048, 1100))   # 2.25M cells: above the 48 MiB / (3 planes x 8 B) = 2M cells a plane may take
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), big, mon, 0, 1)
    idx = bench.dump_sample(big.shape, bench.DUMP_BUDGET_BYTES // 24)
    assert idx.size == bench.DUMP_BUDGET_BYTES // 24 and np.all(np.diff(idx) >= 0)
    assert 0 <= idx[0] and idx[-1] < 2048 * 1100 and np.unique(idx).size > 0.6 * idx.size
    assert np.array_equal(idx, bench.dump_sample(big.shape, idx.size))
    assert sorted(os.listdir(tmp_path / "a")) == ["monitor.npy", "phi.npy", "u.npy", "v.npy"]
    for name, w in (("u", nsa.NS_ARR_U), ("v", nsa.NS_ARR_V), ("phi", nsa.NS_ARR_PHI)):
        a = np.load(tmp_path / "a" / f"{name}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, big.planes[w].ravel()[idx])
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{name}.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "monitor.npy"), [-0.25, 1.0, -0.5, 0.5])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 10 ** 6
    small = Planes((48, 20))
    bench.dump_outputs(str(tmp_path / "s"), small, mon, 1, 2)
    assert sorted(os.listdir(tmp_path / "s")) == ["phi_rank1.npy", "u_rank1.npy", "v_rank1.npy"]
    assert np.array_equal(np.load(tmp_path / "s" / "v_rank1.npy"), small.planes[nsa.NS_ARR_V])


def _bench(args, timeout=300):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "NSBENCH_LAUNCH_PROBE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                       env=env, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run times --steps steps and runs nothing beside them (no Jacobi-sweep leg, no CPU baseline), and
    --dump-outputs writes what the last timed step left: whole float64 planes at this size, whose extrema are the
    line's monitor (K5's fused min / max of the same u, v: equal to the last bit)."""
    import numpy as np
    r = _bench(["--gpus", "1", "--n", "256", "--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path / "o")])
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["unit"] == "MLUPS"
    assert abs(d["value"] - 256 * 256 / d["ms_per_step"] / 1e3) <= 1e-9 * d["value"]
    assert "cpu_baseline" not in d and "parity_vs_oracle" not in d
    assert not any(k.startswith("jacobi") for k in d["kernels"]) and d["roofline"] is not None
    out = {f[:-4]: np.load(tmp_path / "o" / f) for f in sorted(os.listdir(tmp_path / "o"))}
    assert sorted(out) == ["monitor", "phi", "u", "v"]
    assert all(a.dtype == np.float64 for a in out.values())
    assert out["u"].shape == out["v"].shape == out["phi"].shape == (256, 256)
    assert all(np.all(np.isfinite(a)) for a in out.values())
    mon = [d["monitor_last_step"][k] for k in ("umin", "umax", "vmin", "vmax")]
    assert np.array_equal(out["monitor"], mon)
    assert mon == [out["u"].min(), out["u"].max(), out["v"].min(), out["v"].max()]


@pytest.mark.gpu
def test_bench_full_run_keeps_the_other_legs():
    """--full: the Jacobi-sweep roofline kernels and the CPU baseline with its parity check run after the timed
    steps, as every run did before the option existed (parity: SURVEY 8(c)'s 1e-6, set in cpu_baseline)."""
    r = _bench(["--gpus", "1", "--n", "256", "--steps", "3", "--warmup", "2", "--full"])
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][-1])
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    assert d["kernels"]["jacobi_sweep"]["achieved"] > 0 and d["kernels"]["jacobi_sweep_fp32"]["achieved"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["parity_vs_oracle"]["ok"], d["cpu_baseline"]


@pytest.mark.gpu
def test_bench_two_ranks_host_transport():
    """bench.py's N > 1 branch end to end on one GPU (--transport host: both
    ranks on device 0, ghost rows / gathers / reductions through gloo) -- the self-launch, the slab
    step, the per-rank timing max and the rank-0 JSON line.  stdout holds exactly ONE line (the
    relay sends everything that is not a JSON line to stderr), it says n_gpus 2 and the host
    transport, and its last monitor equals one rank's run of the same workload (the slab step
    matches one rank: tests/test_gpu_multirank.py; tolerance 1e-9)."""
    common = ["--n", "512", "--steps", "4", "--warmup", "3", "--no-cpu", "--time-every", "1"]
    r2 = _bench(["--gpus", "2", "--transport", "host", *common])
    lines = [ln for ln in r2.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r2.stdout[-2000:]
    d2 = json.loads(lines[0])
    assert d2["n_gpus"] == 2 and d2["config"]["transport"].startswith("host")
    assert d2["config"]["local_rows_rank0"] == 256
    assert d2["value"] > 0 and d2["roofline"] is not None
    #  the multi-rank line says where its time went: every rank's ms / step and slab,
    # the per-step collectives (r5: 2 on an unchecked direct solve -- the Helmholtz check's scalar bus and
    # the recurrences' one allgather) and exchange groups, the link bytes; the RCCL version on the RCCL transport
    ranks = d2["ranks"]
    assert [x["rank"] for x in ranks] == [0, 1] and [x["rows"] for x in ranks] == [256, 256]
    assert all(x["ms_per_step"] > 0 for x in ranks)
    assert abs(max(x["ms_per_step"] for x in ranks) - d2["ms_per_step"]) <= 1e-6 * d2["ms_per_step"]
    c = d2["comm"]
    assert 2 <= c["collectives_per_step"] <= 5 and c["exchanges_per_step"] >= 1 and c["x_link_bytes_per_step"] > 0
    assert "rccl_version" in c
    d1 = json.loads([ln for ln in _bench(common).stdout.splitlines() if ln.strip()][-1])
    assert d1["n_gpus"] == 1 and "ranks" not in d1 and "comm" not in d1
    for k in ("umin", "umax", "vmin", "vmax"):
        assert abs(d2["monitor_last_step"][k] - d1["monitor_last_step"][k]) <= 1e-9, (k, d2["monitor_last_step"],
                                                                                         d1["monitor_last_step"])
