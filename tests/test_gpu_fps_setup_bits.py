"""GPU: what the direct Poisson solve's setup (fps_setup: the host tables of ns_fps_tables.h, their device arena, the
dense eigenpairs, the FIXED chunks' check) makes the solver compute, pinned bit for bit.

tests/golden/fps_setup_bits.json was recorded by tests/golden/make_fps_setup_bits.py (its CASES and SLABS: each flow
from rest, 4 step_async() calls and a monitor()) on the commit before the tables moved into their header; every case
ran twice there with the same bits.  A run must reproduce the record exactly: the SHA-256 of u, v and phi, every step's
it_u, it_phi, res_u, res_v and the monitor (one rank); every rank's hashes and rank 0's per-step monitor and iteration
counts (slabs, through tests/mr_worker.py on the host transport: the worker returns no res_u / res_v, so the slab
records hold none).  The setup only prepares tables, so any difference is a table, a pivot or a layout that changed.

One case is not bits: 64 x 96 with yratio 1.02, the dense transforms (rocSOLVER's eigenpairs, rocBLAS GEMMs).  With one
and the same library its result depends on what the process ran before: alone in a process it gave the recorded hashes
every time (the recording commit's library and the one with the header alike), after test_gpu_fps.py's dense solves
both gave another set, a few ulp away (monitor -0x1.d2c613a094f07p-6 against -0x1.d2c613a094f10p-6).  So its u, v and
phi (modulo its mean) are compared with the recorded fields (tests/golden/fps_setup_fields.npz) to 1e-8 of their
maximum, test_direct_solve_dense_matches_krylov's tolerance, and it_u and it_phi exactly."""
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_fps_setup_bits", os.path.join(GOLDEN, "make_fps_setup_bits.py"))
mfb = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mfb)
RECORD = json.load(open(os.path.join(GOLDEN, "fps_setup_bits.json")))["cases"]


def test_record_holds_every_case_as_bits():
    assert sorted(RECORD) == sorted(list(mfb.CASES) + list(mfb.SLABS))
    assert not [n for n, r in RECORD.items() if r.get("unstable")]
    assert sorted(n for n, r in RECORD.items() if "tolerance" in r) == sorted(mfb.TOLERANCE)


@pytest.mark.parametrize("name", list(mfb.CASES))
def test_setup_bits_one_rank(gpu, name):
    fields = []
    got = mfb.run_case(gpu, mfb.CASES[name], fields)
    print(name, got)
    if name not in mfb.TOLERANCE:
        assert got == RECORD[name]
        return
    tol, ref = RECORD[name]["tolerance"], np.load(mfb.FIELDS)
    assert [(s["it_u"], s["it_phi"]) for s in got["steps"]] == [(s["it_u"], s["it_phi"]) for s in RECORD[name]["steps"]]
    for q, x in zip(("u", "v", "phi"), fields):
        y = ref[f"{name}_{q}"]
        if q == "phi":
            x, y = x - x.mean(), y - y.mean()
        d = float(np.max(np.abs(x - y)) / np.max(np.abs(y)))
        print(f"{name} {q}: {d:.3e} of max|{q}|")
        assert d <= tol, (q, d)


@pytest.mark.parametrize("name", list(mfb.SLABS))
def test_setup_bits_slabs(gpu, name):
    got = mfb.run_slabs(mfb.SLABS[name], 29941 + list(mfb.SLABS).index(name))
    print(name, got)
    assert got == RECORD[name]
