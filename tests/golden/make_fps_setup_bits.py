"""Record what the direct Poisson solve's setup tables compute, bit for bit (tests/golden/fps_setup_bits.json) -- needs
the GPU; run from the repo root:
    python tests/golden/make_fps_setup_bits.py
Through the public Python API only, so the same file records any commit of the library.  Each case of CASES runs its
flow from rest for 4 step_async() calls and a monitor() and stores the SHA-256 of the bytes of u, v and phi, every
step's it_u, it_phi, res_u, res_v (floats as hex) and the monitor.  The slab cases (SLABS) go through tests/mr_worker.py
on the host transport (--async-steps --hash): every rank's SHA-256 of its slab of u, v, phi and rank 0's per-step
(umin, umax, vmin, vmax, it_u, it_v, it_phi), the monitor realigned to its step.  Every case runs twice; a case whose
two runs differ is recorded as {"unstable": true} and named on stdout.  The cases of TOLERANCE are not bits either: the
dense transforms go through rocSOLVER and rocBLAS, whose results depend on what the process ran before (measured with
one and the same library: alone in a process the case gives one set of bits, after another dense solve another, a
few ulp apart) -- their fields go to fps_setup_fields.npz and are compared at the given relative tolerance.
tests/test_gpu_fps_setup_bits.py replays the cases against the record (it imports CASES / SLABS / run_case / run_slabs
from here).  Regenerate it only with a change that means to alter what the direct solve computes."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.abspath(os.path.join(HERE, ".."))
for p in (os.path.join(HERE, "..", ".."), os.path.join(HERE, "..", "..", "oracle"), TESTS):
    if os.path.abspath(p) not in sys.path:
        sys.path.insert(0, os.path.abspath(p))

OUT = os.path.join(HERE, "fps_setup_bits.json")
FIELDS = os.path.join(HERE, "fps_setup_fields.npz")
STEPS = 4
RE = 100.0
BC_CHANNEL = [(0, 1.0), (2, 0.0), (4, 0.0), (2, 0.0)]   # inlet W, walls N / S, NEUMANN outflow E


def _rect(nx, ny, env=None, lx=None, **kw):
    """The cavity on nx x ny cells, square unless lx is given (test_gpu_fps_fixed.py's step: dt from the smaller
    spacing, Re 100)."""
    L = lx if lx else nx / ny
    return dict(grid=("rect", nx, ny, dict(lx=L, **kw)), dt=min(L / nx, 1.0 / ny) / 8, re=RE, env=env or {})


# name -> case; the comment: the part of the setup it is here for
CASES = {
    "33x16": _rect(33, 16),                                   # no pivot shortcut, one ragged chunk
    "40x96": _rect(40, 96),                                   # mixed radix
    "64x256": _rect(64, 256),                                 # two blocks, nx - 1 = 63: shortcut off
    "200x512": _rect(200, 512),                               # a FIXED chunk after a general one, ragged chunk, group
    "200x512_ptab0": _rect(200, 512, {"NSGPU_FPS_PTAB": "0"}),
    "200x512_ptab1": _rect(200, 512, {"NSGPU_FPS_PTAB": "1"}),
    "200x512_passes3": _rect(200, 512, {"NSGPU_FPS_PASSES": "3"}),
    "520x1024": _rect(520, 1024),                             # blocks with different first fixed chunks
    "2048x512_lx8": _rect(2048, 512, lx=8.0),                 # hx = 2 hy: block 0's fixed point inside the grid
    "96x128_xratio": _rect(96, 128, xratio=1.02),             # shortcut mode forced to 0
    "64x96_yratio": _rect(64, 96, yratio=1.02),               # dense transforms (rocSOLVER / rocBLAS)
    "32x16384": _rect(32, 16384),                             # the 8192-point table
    # outE: the channel as test_gpu_fps.py::_channel builds it (h = 4 / nx, dt = h / 8, Re 1000)
    "channel128x256": dict(grid=("rect", 128, 256, dict(lx=4.0, ly=256 * 4.0 / 128, bc=BC_CHANNEL)), dt=4.0 / 128 / 8,
                           re=1000.0, env={}),
    # a masked domain with the box's direct preconditioner
    "lshape_pc": dict(grid=("polygon", "lshape"), dt=1.0 / 1024, re=200.0, env={"NSGPU_CAP": "0", "NSGPU_FPS_PC": "1"}),
}


def _slab(n, ny, nproc, env=None, bc=None):
    return dict(n=n, ny=ny, nproc=nproc, env=env or {}, bc=bc)


SLABS = {
    "slab96x256_r2": _slab(96, 256, 2),                        # slab edges on chunk boundaries: 48
    "slab96x256_r3": _slab(96, 256, 3),                        # ... 32, 64
    "slab200x512_r3": _slab(200, 512, 3),                      # 72 / 64 / 64 rows, slabs starting mid-chunk
    "slab200x512_r3_onegather0": _slab(200, 512, 3, {"NSGPU_FPS_ONEGATHER": "0"}),
    "slab200x512_r3_onegather1": _slab(200, 512, 3, {"NSGPU_FPS_ONEGATHER": "1"}),
    "slab200x512_r3_defer0": _slab(200, 512, 3, {"NSGPU_FPS_DEFER": "0"}),
    "slab200x512_r3_defer1": _slab(200, 512, 3, {"NSGPU_FPS_DEFER": "1"}),
    "slab_channel128x256_r2": _slab(128, 256, 2, bc=BC_CHANNEL),   # the outflow row on the last slab
}
# not bits: u, v and phi (modulo its mean) to this relative tolerance -- test_direct_solve_dense_matches_krylov's
TOLERANCE = {"64x96_yratio": 1e-8}
# the knobs the cases set: cleared for every other case, so that a caller's environment cannot leak in
KNOBS = sorted({k for c in list(CASES.values()) + list(SLABS.values()) for k in c["env"]})


class _Env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in KNOBS}
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def make_grid(nsa, spec):
    if spec[0] == "rect":
        return nsa.rectangle(spec[1], spec[2], **spec[3])
    from oracle import OGrid
    from polygons import ALL
    P = ALL[spec[1]]
    og = OGrid(P["vertices"], P["xspec"], P["yspec"], P["bc"])
    return nsa.polygon(P["vertices"], og.hx, og.hy, P["bc"])


def _sha(x):
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def run_case(nsa, case, fields=None):
    """The record of one single-rank case (the knobs are read at ns_create; the environment is restored); u, v, phi
    appended to `fields` if it is a list."""
    with _Env(case["env"]):
        gs = nsa.GpuSolver(make_grid(nsa, case["grid"]), case["dt"], case["re"], device=0)
    st = [gs.step_async() for _ in range(STEPS)]
    mon = gs.monitor()
    u, v, phi = gs.fields()
    gs.close()
    if fields is not None:
        fields += [u.copy(), v.copy(), phi.copy()]
    return {"u": _sha(u), "v": _sha(v), "phi": _sha(phi),
            "steps": [{"it_u": int(s["it_u"]), "it_phi": int(s["it_phi"]), "res_u": float(s["res_u"]).hex(),
                       "res_v": float(s["res_v"]).hex()} for s in st],
            "monitor": [float(x).hex() for x in mon]}


def run_slabs(case, port):
    """The record of one slab case: tests/mr_worker.py under torch.distributed.run, every rank on the one GPU."""
    with tempfile.TemporaryDirectory() as tmp, _Env(case["env"]):
        out = os.path.join(tmp, "r.npz")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={case['nproc']}",
               "--master-addr=127.0.0.1", f"--master-port={port}", os.path.join(TESTS, "mr_worker.py"), "--output", out,
               "--xport", "host", "--size", str(case["n"]), "--size-y", str(case["ny"]), "--nsteps", str(STEPS),
               "--async-steps", "--hash"]
        if case["bc"]:
            cmd += ["--bc", ",".join(f"{t}:{i}" for t, i in case["bc"])]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=150, env=dict(os.environ))
        assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
        r = dict(np.load(out, allow_pickle=False))
    assert str(r["status"]) == "ok", r["status"]
    return {"u": r["u"].tobytes().hex(), "v": r["v"].tobytes().hex(), "phi": r["phi"].tobytes().hex(),
            "steps": [[float(x).hex() for x in row] for row in r["mm"]]}


def main():
    import navierstokessolver_amd as nsa
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    only = sys.argv[2].split(",") if len(sys.argv) > 2 else None
    rec, unstable, fields = {}, [], {}
    runs = [(n, lambda c=c, n=n: run_case(nsa, c, fields.setdefault(n, []) if n in TOLERANCE else None))
            for n, c in CASES.items()]
    runs += [(n, lambda c=c, k=k: run_slabs(c, 29901 + k)) for k, (n, c) in enumerate(SLABS.items())]
    for name, run in runs:
        if only and name not in only:
            continue
        a, b = run(), run()
        if name in TOLERANCE:
            rec[name] = {"tolerance": TOLERANCE[name],
                         "steps": [{"it_u": s["it_u"], "it_phi": s["it_phi"]} for s in a["steps"]]}
        elif a == b:
            rec[name] = a
        else:
            rec[name] = {"unstable": True}
            unstable.append(name)
        print(name, "UNSTABLE" if a != b else a["phi"][:16], a["steps"], flush=True)
    json.dump({"generator": "tests/golden/make_fps_setup_bits.py", "cases": rec}, open(out, "w"), indent=1)
    if fields:
        np.savez_compressed(os.path.join(os.path.dirname(out), os.path.basename(FIELDS)),
                            **{f"{n}_{q}": f[k] for n, f in fields.items() for k, q in enumerate(("u", "v", "phi"))})
    print("wrote", out, "; unstable:", unstable)


if __name__ == "__main__":
    main()
