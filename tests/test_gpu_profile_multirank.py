"""Edge profiles on x-slabs: 2 processes on one GPU over the host transport (tests/mr_profile_worker.py) against
one rank, at the slab tests' tolerance (1e-9 at rtol 1e-11, test_gpu_multirank.py).  The y-normal edges' tables
are indexed by the global row across the slab boundary, and the deep ghost rows of the slabs' launches read them
with rows outside [0, nx) (clamped)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import navierstokessolver_amd as nsa
from mr_profile_worker import profiles_of

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def launch(tmp_path, *args, port=29581, nproc=2):
    out = tmp_path / "r.npz"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(HERE, "mr_profile_worker.py"),
           "--output", str(out), *args]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=150, env=dict(os.environ))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return dict(np.load(out, allow_pickle=False))


CASES = {
    # N and S inlets profiled (W, E walls): the direct solve with the fused divergence, and the multigrid
    "ns-direct": ("2:0,0:1,2:0,0:1", "1:201,3:202", {}),
    "ns-multigrid": ("2:0,0:1,2:0,0:1", "1:201,3:202", {"NSGPU_FPS": "0"}),
    # the channel: W inlet profiled, E NEUMANN (the last slab), and the N wall's tangential speed
    "channel": ("0:1,2:0,4:0,2:0", "0:203,1:204", {}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_profiled_slabs_match_single_rank(tmp_path, monkeypatch, name):
    bcs, prof, env = CASES[name]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    n, steps, rtol = 64, 6, 1e-11
    r = launch(tmp_path, "--size", str(n), "--nsteps", str(steps), "--tol", str(rtol), "--bc", bcs, "--prof", prof)
    assert str(r["status"]) == "ok", r["status"]
    bc = [(int(t), float(i)) for t, i in (e.split(":") for e in bcs.split(","))]
    res = []
    for with_profile in (True, False):
        gs = nsa.GpuSolver(nsa.rectangle(n, n, bc=bc), 1.0 / (8 * n), 100.0, rtol=rtol, device=0)
        if with_profile:
            for e, p in profiles_of(prof, n, n).items():
                gs.set_edge_profile(e, p)
        mm = np.array([list(gs.step().values())[:7] for _ in range(steps)])
        res.append((gs.fields(), mm))
        gs.close()
    (u, v, _), mm = res[0]
    du, dv = float(np.max(np.abs(r["u"] - u))), float(np.max(np.abs(r["v"] - v)))
    print(f"{name}: du {du:.2e} dv {dv:.2e}")
    assert r["u"].shape == u.shape
    assert du <= 1e-9 and dv <= 1e-9, (du, dv)
    np.testing.assert_allclose(r["mm"][:, :4], mm[:, :4], atol=1e-9)
    # (the profiles were seen: the same grid without them is elsewhere)
    assert np.max(np.abs(res[1][0][0] - u)) > 1e-3
