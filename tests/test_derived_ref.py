"""tests/derived_ref.py -- the NumPy statement of ns_derive's fields -- pinned to the CPU oracle (no GPU).

div is K3 without its 1 / dt, so dt * og.divergence; P is og.pressure; the vorticity of (u, v) is the divergence of
(v, -u) where every velocity ghost treats both components alike -- still walls (ghost -q) and NEUMANN edges (ghost q)
-- so on that variant of each grid vort = dt * og.divergence(dt, v, -u).  All to 1e-12 of the plane's max: the
arithmetic alone gives ~1e-14.  The stream function has no oracle counterpart: it is pinned by its identities."""
import numpy as np
import pytest

from derived_ref import DGrid, NEUMANN, WALL, cell_fields, derived, stream_function
from oracle import OGrid
from polygons import ALL, NARROW
from profile_ref import rect_spec

DT, RE = 1.0 / 256, 100.0
CAVITY = [(2, 0.0), (2, 1.0), (2, 0.0), (2, 0.0)]
CHANNEL = [(0, 1.0), (2, 0.0), (4, 0.0), (2, 0.0)]   # inlet W, walls N / S, NEUMANN outflow E
SPECS = {**ALL, **NARROW,
         "rect_13x9s": rect_spec(13, 9, CAVITY, xr=1.1, yr=0.9),
         "channel_16x8": rect_spec(16, 8, CHANNEL, lx=2.0)}


def ogrid(spec, bc=None):
    return OGrid(spec["vertices"], spec["xspec"], spec["yspec"], spec["bc"] if bc is None else bc)


def still(bc):
    """Every wall and inlet a still wall, NEUMANN edges as they are."""
    return [(t, i) if t == NEUMANN else (WALL, 0.0) for t, i in bc]


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("name", sorted(SPECS))
def test_div_and_pressure_are_the_oracles(name):
    sp = SPECS[name]
    og = ogrid(sp)
    G = DGrid.from_oracle(og, sp["bc"])
    rng = np.random.default_rng(31)
    u, v, phi = (rng.uniform(-1, 1, og.N) for _ in range(3))
    div, _, P = cell_fields(G, DT, RE, G.plane(u), G.plane(v), G.plane(phi))
    ed = rel(div[G.mask], DT * og.divergence(DT, u, v))
    ep = rel(P[G.mask], og.pressure(DT / (2 * RE), phi))
    print(f"{name}: div {ed:.2e} P {ep:.2e}")
    assert ed <= 1e-12 and ep <= 1e-12
    assert not np.any(div[~G.mask]) and not np.any(P[~G.mask])


@pytest.mark.parametrize("name", sorted(SPECS))
def test_vorticity_is_the_oracles_divergence_of_the_rotated_field(name):
    sp = SPECS[name]
    bc = still(sp["bc"])
    og = ogrid(sp, bc)
    G = DGrid.from_oracle(og, bc)
    rng = np.random.default_rng(32)
    u, v = (rng.uniform(-1, 1, og.N) for _ in range(2))
    _, vort, _ = cell_fields(G, DT, RE, G.plane(u), G.plane(v), np.zeros((G.nx, G.ny)))
    e = rel(vort[G.mask], DT * og.divergence(DT, v, -u))
    print(f"{name}: vort {e:.2e}")
    assert e <= 1e-12


def test_lid_face_value_is_the_lid_speed():
    s, nx, ny = 0.75, 9, 7
    sp = rect_spec(nx, ny, [(2, 0.0), (2, s), (2, 0.0), (2, 0.0)], yr=1.1)
    og = ogrid(sp)
    G = DGrid.from_oracle(og, sp["bc"])
    z = np.zeros((nx, ny))
    for i in range(nx):
        assert G.face(z, i, ny - 1, 3, 0) == s          # u_N = 0.5 (0 + (-0 + 2 s))
        assert G.face(z, i, ny - 1, 3, 1) == 0.0        # (the wall's normal component)
    _, vort, _ = cell_fields(G, DT, RE, z, z, z)
    assert np.array_equal(vort[:, -1], np.full(nx, -(s - 0.0) / og.hy[-1]))   # vort = -(u_N - u_S) / hy
    assert not np.any(vort[:, :-1])
    rng = np.random.default_rng(33)
    u = rng.uniform(-1, 1, (nx, ny))
    assert max(abs(G.face(u, i, ny - 1, 3, 0) - s) for i in range(nx)) <= 4e-16


def test_lid_profile_changes_the_lid_row_by_the_formulas_amount():
    s, nx, ny = 1.0, 10, 8
    sp = rect_spec(nx, ny, [(2, 0.0), (2, s), (2, 0.0), (2, 0.0)])
    og = ogrid(sp)
    x = (np.arange(nx) + 0.5) / nx
    prof = s * (1 - (2 * x - 1) ** 16) ** 2              # the regularised lid
    rng = np.random.default_rng(34)
    u, v, phi = (rng.uniform(-1, 1, (nx, ny)) for _ in range(3))
    d0, w0, p0 = cell_fields(DGrid.from_oracle(og, sp["bc"]), DT, RE, u, v, phi)
    d1, w1, p1 = cell_fields(DGrid.from_oracle(og, sp["bc"], {1: prof}), DT, RE, u, v, phi)
    assert np.array_equal(d0, d1) and np.array_equal(p0, p1)
    assert np.array_equal(w0[:, :-1], w1[:, :-1])
    want = -(prof - s) / og.hy[-1]                       # vort = ... - (u_N - u_S) / hy, u_N = info at the face
    assert rel(w1[:, -1] - w0[:, -1], want) <= 1e-12
    assert np.max(np.abs(want)) > 0.5


@pytest.mark.parametrize("name", ["rect_13x9s", "channel_16x8"])
def test_psi_column_identity(name):
    """psi(i + 1, j) - psi(i, j) + v_S-face(i, j) hx[i] = sum_{j' < j} div(i, j') hx[i] hy[j'] on a rectangle."""
    sp = SPECS[name]
    og = ogrid(sp)
    G = DGrid.from_oracle(og, sp["bc"])
    rng = np.random.default_rng(35)
    u, v = (rng.uniform(-1, 1, (G.nx, G.ny)) for _ in range(2))
    psi = stream_function(G, u, v)
    div, _, _ = cell_fields(G, DT, RE, u, v, np.zeros((G.nx, G.ny)))
    worst = 0.0
    for i in range(G.nx):
        acc = 0.0
        for j in range(G.ny):
            lhs = psi[i + 1, j] - psi[i, j] + G.face(v, i, j, 2, 1) * G.hx[i]
            worst = max(worst, abs(lhs - acc))
            acc += div[i, j] * G.hx[i] * G.hy[j]
    print(f"{name}: psi identity {worst:.2e} of {np.max(np.abs(psi)):.2e}")
    assert worst <= 1e-13 * np.max(np.abs(psi))


def test_uniform_channel_flow():
    sp = SPECS["channel_16x8"]
    # u = 1 everywhere slips along the walls only if they move with it: the channel with N / S walls at speed 1
    bc = [(0, 1.0), (2, 1.0), (4, 0.0), (2, 1.0)]
    og = ogrid(sp, bc)
    G = DGrid.from_oracle(og, bc)
    one, z = np.ones((G.nx, G.ny)), np.zeros((G.nx, G.ny))
    r = derived(G, DT, RE, one, z, z)
    Y = np.concatenate([[0.0], np.cumsum(og.hy)])
    assert np.array_equal(r["psi"], np.tile(Y, (G.nx + 1, 1)))
    assert not np.any(r["vort"]) and not np.any(r["div"])
    assert r["enstrophy"] == 0.0 and r["div_max"] == 0.0
    assert r["ke"] == pytest.approx(0.5 * 2.0 * 1.0, rel=1e-14)
    assert r["cfl"] == pytest.approx(DT / og.hx[0], rel=1e-14)


@pytest.mark.parametrize("name,columns", [("lshape", range(17, 33)), ("u_div1", [])])
def test_psi_is_constant_across_outside_cells(name, columns):
    """Vertex columns (fixed i) that cross only outside cells, and those along a wall (its normal velocity's face
    value is 0.5 (u + (-u + 0)) = 0 exactly; every edge of these two shapes is a wall): differences exactly 0."""
    sp = SPECS[name]
    og = ogrid(sp)
    G = DGrid.from_oracle(og, sp["bc"])
    assert all(t == WALL for t, _ in sp["bc"])
    rng = np.random.default_rng(36)
    psi = stream_function(G, G.plane(rng.uniform(-1, 1, og.N)), G.plane(rng.uniform(-1, 1, og.N)))
    seen = 0
    for i in range(G.nx + 1):
        for j in range(G.ny):
            if not (G.inside(i - 1, j) and G.inside(i, j)):
                assert psi[i, j + 1] - psi[i, j] == 0.0, (i, j)
                seen += not G.inside(i - 1, j) and not G.inside(i, j)
    assert seen > 0 or name == "u_div1"   # (the divider is one cell thick: a wall on either side of each line)
    if name == "lshape":      # the notch x > 0.5, y < 0.5: vertex rows 17 .. 32 are flat up to j = 16
        for i in columns:
            assert np.all(psi[i, :17] == psi[i, 0])
    else:                     # the divider's outside cells (column 9, j >= 6): both vertex rows between arm and divider
        assert G.mask[9, 5] and not G.mask[9, 6]
