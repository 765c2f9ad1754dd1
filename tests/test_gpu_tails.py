"""(r7) On one rank the step's small launches between the big kernels are folded into their neighbours: K1''s norms and
min / max wait for the Helmholtz check's reduction (one launch of four workgroups, k_reduce_step: K1' leaves its sum
partials where no launch before that check writes), and the two group scans and k_fps_mid of the direct solve run as one
launch (k_fps_midscan).  The paths that keep their own launches are the reference here: NSGPU_K5_DEFER=0 (K1 with its
own reduction: bit-equal, test_deferred_correction_is_bit_identical's criterion), NSGPU_FPS_PASSES=3 (the three-pass
recurrences with their scan launches: test_two_pass_recurrences_equal_three_pass's 1e-12 of max|phi|) and, for the
fused transform's partials and mean next to the new launches, NSGPU_FPS_FUSE=0 (test_fused_divergence_equals_k3's
bounds: u, v and the monitor to 1e-12, phi modulo its mean to 1e-11 of its max).

Every case is the cavity from rest at Re 100, square cells, 6 ns_step_async calls and a closing monitor().  Shapes
(nx x ny), the smallest at which each piece takes another path:
  16 x 64      one chunk, one group, the pair transform, 8 row-pair partials, idle lanes past ny;
  72 x 128     a ragged last chunk (72 = 4 x 16 + 8) and group (5 chunks = 4 + 1);
  520 x 1024   the row transform, 33 chunks in 9 groups (above FPS_SSEG, below the segmented scan's 16), ragged;
  1040 x 1024  65 chunks in 17 groups: the segmented scan, with an empty last segment; 1040 row partials (> 1024:
               a second round of the reductions' 1024 lanes);
  2048 x 1024  with NSGPU_STRIP_ROWS=16: 1152 Helmholtz partials per field and > 1024 K1 partials."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS = 6
RE = 100.0
SHAPES = [(16, 64, {}), (72, 128, {}), (520, 1024, {}), (1040, 1024, {}), (2048, 1024, {"NSGPU_STRIP_ROWS": "16"})]
IDS = [f"{nx}x{ny}" for nx, ny, _ in SHAPES]
KEYS = ("umin", "umax", "vmin", "vmax", "it_u", "it_phi", "res_u", "res_v")

_runs = {}


def _run(gpu, nx, ny, env, tag=""):
    """One run (cached per shape and environment; `tag` asks for another run of the same)."""
    key = (nx, ny, tuple(sorted(env.items())), tag)
    if key in _runs:
        return _runs[key]
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        gs = gpu.GpuSolver(gpu.rectangle(nx, ny, lx=nx / ny), 1.0 / (8 * max(nx, ny)), RE)
        stats = [gs.step_async() for _ in range(STEPS)]
        mon = gs.monitor()
        after = gs.step_async()          # (the step after a monitor(): no reduction is left pending across it)
        mon2 = gs.monitor()
        fields = [a.copy() for a in gs.fields()]
        gs.close()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    _runs[key] = dict(stats=stats, mon=mon, after=after, mon2=mon2, fields=fields)
    return _runs[key]


def _same(x, y):
    return (np.isnan(x) and np.isnan(y)) or x == y


def demean(x):
    x = np.asarray(x).ravel()
    return x - x.mean()


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("nx,ny,env", SHAPES, ids=IDS)
def test_folded_reductions_equal_the_undeferred_step_bit_for_bit(gpu, nx, ny, env):
    a = _run(gpu, nx, ny, env)
    b = _run(gpu, nx, ny, {**env, "NSGPU_K5_DEFER": "0"})
    # the deferred path ran: every async step after the first folded its predecessor's K5 into K1'
    assert [s["k5_deferred"] for s in a["stats"]] == [0] + [1] * (STEPS - 1), [s["k5_deferred"] for s in a["stats"]]
    assert all(s["k5_deferred"] == 0 for s in b["stats"])
    for x, y in zip(a["stats"] + [a["after"]], b["stats"] + [b["after"]]):
        assert all(_same(x[k], y[k]) for k in KEYS), (x, y)
    assert a["mon"] == b["mon"] and a["mon2"] == b["mon2"]
    assert all(np.isfinite(v) for v in a["mon2"])
    for x, y in zip(a["fields"], b["fields"]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("nx,ny,env", SHAPES, ids=IDS)
def test_default_step_against_the_unfused_divergence(gpu, nx, ny, env):
    a = _run(gpu, nx, ny, env)
    b = _run(gpu, nx, ny, {**env, "NSGPU_FPS_FUSE": "0"})
    (u, v, phi), (ur, vr, phir) = a["fields"], b["fields"]
    du, dv, dp = np.max(np.abs(u - ur)), np.max(np.abs(v - vr)), rel(demean(phi), demean(phir))
    dm = np.max(np.abs(np.array(a["mon2"]) - np.array(b["mon2"])))
    print(f"{nx}x{ny} fused vs K3: |du| {du:.3e} |dv| {dv:.3e} phi {dp:.3e} monitor {dm:.3e}")
    assert all(s["it_phi"] == 1 for s in a["stats"] + b["stats"])
    np.testing.assert_allclose(a["mon"], b["mon"], atol=1e-12)
    np.testing.assert_allclose(a["mon2"], b["mon2"], atol=1e-12)
    assert du <= 1e-12 and dv <= 1e-12, (du, dv)
    assert dp <= 1e-11, dp


@pytest.mark.parametrize("nx,ny,env", SHAPES, ids=IDS)
def test_merged_middle_kernel_against_three_pass_recurrences(gpu, nx, ny, env):
    a = _run(gpu, nx, ny, env)
    b = _run(gpu, nx, ny, {**env, "NSGPU_FPS_PASSES": "3"})
    dp = rel(demean(a["fields"][2]), demean(b["fields"][2]))
    du = max(np.max(np.abs(x - y)) for x, y in zip(a["fields"][:2], b["fields"][:2]))
    print(f"{nx}x{ny} two-pass (merged middle) vs three-pass: phi {dp:.3e} |du, dv| {du:.3e}")
    assert dp <= 1e-12, dp


@pytest.mark.parametrize("nx,ny,env", SHAPES, ids=IDS)
def test_two_solvers_built_alike_agree_bit_for_bit(gpu, nx, ny, env):
    """A partial read before it was written, or after a later launch overwrote it, shows here."""
    a = _run(gpu, nx, ny, env)
    b = _run(gpu, nx, ny, env, tag="again")
    for x, y in zip(a["stats"] + [a["after"]], b["stats"] + [b["after"]]):
        assert all(_same(x[k], y[k]) for k in KEYS), (x, y)
    assert a["mon"] == b["mon"] and a["mon2"] == b["mon2"]
    for x, y in zip(a["fields"], b["fields"]):
        assert np.array_equal(x, y)
