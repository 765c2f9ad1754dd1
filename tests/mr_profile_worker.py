"""Worker for tests/test_gpu_profile_multirank.py (launched by torch.distributed.run): `nsteps` steps of a
rectangle on an x-slab per rank (every rank on GPU 0, host transport) with seeded random edge profiles -- the
same table on every rank, indexed by the global row on the y-normal edges -- gathered on rank 0 and saved."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401
import torch.distributed as dist

import navierstokessolver_amd as nsa
from navierstokessolver_amd.dist import TorchHostTransport


def profile(seed, n):
    return np.random.default_rng(seed).uniform(0.5, 1.5, n)


def profiles_of(text, nx, ny):
    """"edge:seed,..." -> {edge: values}; a rectangle's edges W, N, E, S (W / E: ny values, N / S: nx)."""
    out = {}
    for item in text.split(","):
        e, seed = (int(x) for x in item.split(":"))
        out[e] = profile(seed, ny if e in (0, 2) else nx)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--size-y", type=int, default=0)
    ap.add_argument("--nsteps", type=int, default=6)
    ap.add_argument("--tol", type=float, default=1e-11)
    ap.add_argument("--bc", required=True, help="edge BCs W,N,E,S as type:info,...")
    ap.add_argument("--prof", required=True, help="profiled edges as edge:seed,...")
    ap.add_argument("--output", required=True)
    a = ap.parse_args()
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    n, ny = a.size, a.size_y or a.size
    status = "ok"
    try:
        bc = [(int(t), float(i)) for t, i in (e.split(":") for e in a.bc.split(","))]
        gs = nsa.GpuSolver(nsa.rectangle(n, ny, bc=bc), 1.0 / (8 * n), 100.0, rank=rank, nranks=world, device=0,
                           rtol=a.tol, host_transport=TorchHostTransport(dist))
        for e, p in profiles_of(a.prof, n, ny).items():
            gs.set_edge_profile(e, p)
        mm = [list(gs.step().values())[:7] for _ in range(a.nsteps)]
        u, v, phi = gs.fields()
    except Exception as e:  # report, don't hang the other rank
        status = f"error: {e}"
        u = v = phi = np.zeros((1, ny))
        mm = []
    parts = [None] * world
    dist.all_gather_object(parts, (status, u, v, phi, mm))
    if rank == 0:
        st = [p[0] for p in parts]
        if all(s == "ok" for s in st):
            np.savez(a.output, u=np.concatenate([p[1] for p in parts]), v=np.concatenate([p[2] for p in parts]),
                     phi=np.concatenate([p[3] for p in parts]), mm=np.array(parts[0][4]), status="ok")
        else:
            np.savez(a.output, status="; ".join(st))
    dist.barrier()
    dist.destroy_process_group()
