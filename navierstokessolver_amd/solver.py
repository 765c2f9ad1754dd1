"""Python handle over one ns_solver (libnsgpu.so).  Plumbing for tests and bench.py;
the reference-compatible host API is the C++ Grid / FluidSolver in host/."""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field

import numpy as np

from . import _lib as L


@dataclass
class Edge:
    """One polygon edge (Edge, /root/reference/SRC/Grid.h:20-26)."""
    nx: int
    ny: int
    type: int = L.NS_BC_WALL
    info: float = 0.0


@dataclass
class GridSpec:
    """Geometry handed to ns_create: spacings plus edges.  A rectangle leaves cell_id /
    face_edge None; any other polygon (cavity.polygon) carries the bounding box's
    compact ids (-1 outside; Grid.cpp:149-162) and per-cell boundary-edge tags (W,E,S,N;
    Cell::edges, Grid.h:33)."""
    hx: np.ndarray
    hy: np.ndarray
    edges: list = field(default_factory=list)
    cell_id: np.ndarray | None = None
    face_edge: np.ndarray | None = None

    @property
    def mask(self):
        """nx x ny booleans: the cells inside the domain (all of them for a rectangle)."""
        if self.cell_id is None:
            return np.ones((self.nx, self.ny), dtype=bool)
        return np.asarray(self.cell_id).reshape(self.nx, self.ny) >= 0

    @property
    def nx(self):
        return len(self.hx)

    @property
    def ny(self):
        return len(self.hy)


def _dptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


class GpuSolver:
    """One x-slab (the whole grid when nranks == 1) resident on one MI355X."""

    def __init__(self, grid: GridSpec, dt: float, re: float, *, poisson=L.NS_POISSON_MG, rtol=1e-8,
                 max_iters=0, omega=0.0, omega_v=0.0, check_every=0, device=-1, timing=False,
                 rank=0, nranks=1, nccl_id: bytes | None = None, mg_pre=0, mg_post=0, mg_coarse_iters=0,
                 host_transport=None, mg_omega=0.0):
        self.grid = grid
        self.hx = np.ascontiguousarray(grid.hx, dtype=np.float64)
        self.hy = np.ascontiguousarray(grid.hy, dtype=np.float64)
        self._edges = (L.NsEdge * len(grid.edges))(*[L.NsEdge(e.nx, e.ny, e.type, e.info) for e in grid.edges])
        ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        self._cid = self._ftag = None
        if grid.cell_id is not None:
            self._cid = np.ascontiguousarray(grid.cell_id, dtype=np.int32)
            self._ftag = np.ascontiguousarray(grid.face_edge, dtype=np.int32)
            assert self._cid.size == self.hx.size * self.hy.size and self._ftag.size == 4 * self._cid.size
        desc = L.NsGridDesc(self.hx.size, self.hy.size, _dptr(self.hx), _dptr(self.hy), len(grid.edges),
                            self._edges, ip(self._cid) if self._cid is not None else None,
                            ip(self._ftag) if self._ftag is not None else None)
        self._nccl = ctypes.create_string_buffer(nccl_id, len(nccl_id)) if nccl_id else None
        prm = L.NsParams(dt, re, poisson, rtol, max_iters, omega, omega_v, check_every, device,
                         1 if timing else 0, rank, nranks,
                         ctypes.cast(self._nccl, ctypes.c_void_p) if self._nccl is not None else None,
                         mg_pre, mg_post, mg_coarse_iters,
                         ctypes.pointer(host_transport.struct) if host_transport is not None else None,
                         mg_omega)
        self._transport = host_transport  # keep the callbacks alive
        self._scalar = False
        self._tracers = 0   # particles added so far (add_tracers / reset_tracers)
        h = ctypes.c_void_p()
        L.check(L.lib().ns_create(ctypes.byref(desc), ctypes.byref(prm), ctypes.byref(h)))
        self._h = h
        self.dt, self.re = dt, re
        self.rank, self.nranks = rank, nranks
        self.i0, self.i1 = L.slab_range(self.hx.size, nranks, rank)
        # the Helmholtz SOR weight libnsgpu.so derives (ns_create): 2 / (1 + sqrt(1 - rho^2))
        if omega_v > 0:
            self.omega_v = omega_v
        else:
            t = dt / re * (1 / self.hx.min() ** 2 + 1 / self.hy.min() ** 2)
            rho = t / (1 + t)
            self.omega_v = 2 / (1 + (1 - rho * rho) ** 0.5)
        self.shape = (self.i1 - self.i0, self.hy.size)
        # the multigrid smoother's over-relaxation (ns_create: 1.1 unless given; NSGPU_MG_OMEGA wins)
        self.mg_omega = float(os.environ.get("NSGPU_MG_OMEGA", mg_omega if mg_omega > 0 else 1.1))

    # ---- lifecycle
    def close(self):
        if getattr(self, "_h", None):
            L.lib().ns_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- stepping
    def step(self) -> dict:
        st = L.NsStats()
        L.check(L.lib().ns_step(self._h, ctypes.byref(st)))
        d = st.as_dict()
        if self._scalar:
            ss = self.scalar_stats()
            d["tmin"], d["tmax"] = ss["tmin"], ss["tmax"]
        return d

    def step_async(self) -> dict:
        """ns_step_async: one step without the closing host sync; umin..vmax are the previous
        step_async's monitor values (NaN on the first), monitor() returns the latest."""
        st = L.NsStats()
        L.check(L.lib().ns_step_async(self._h, ctypes.byref(st)))
        return st.as_dict()

    def monitor(self) -> tuple:
        mm = np.empty(4, dtype=np.float64)
        L.check(L.lib().ns_monitor(self._h, _dptr(mm)))
        return tuple(float(x) for x in mm)

    # ---- state
    def get(self, which: int) -> np.ndarray:
        out = np.empty(self.shape, dtype=np.float64)
        L.check(L.lib().ns_get_array(self._h, which, _dptr(out)))
        return out

    def set(self, which: int, a) -> None:
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(self.shape))
        L.check(L.lib().ns_set_array(self._h, which, _dptr(a)))

    def fields(self):
        """u, v, phi as the slab's nx_local x ny bounding-box planes (ns_get_array)."""
        return self.get(L.NS_ARR_U), self.get(L.NS_ARR_V), self.get(L.NS_ARR_PHI)

    def local_cells(self) -> tuple:
        """(first compact id, count) of this slab's in-domain cells (ns_local_cells)."""
        a, n = ctypes.c_int64(), ctypes.c_int64()
        L.check(L.lib().ns_local_cells(self._h, ctypes.byref(a), ctypes.byref(n)))
        return a.value, n.value

    def fields_compact(self):
        """u, v, phi in the reference's compact Vec order (ns_get_fields; Grid.cpp:149-162)."""
        n = self.local_cells()[1]
        u, v, p = (np.empty(n) for _ in range(3))
        L.check(L.lib().ns_get_fields(self._h, _dptr(u), _dptr(v), _dptr(p)))
        return u, v, p

    def set_fields_compact(self, u=None, v=None, phi=None, cu0=None, cv0=None) -> None:
        """ns_set_fields: any of u, v, phi, convectiveDer_u0 / _v0 in compact Vec order."""
        n = self.local_cells()[1]
        keep = [None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel())
                for a in (u, v, phi, cu0, cv0)]
        for a in keep:
            if a is not None and a.size != n:
                raise ValueError(f"compact field of {a.size} values; this slab holds {n} cells")
        L.check(L.lib().ns_set_fields(self._h, *[None if a is None else _dptr(a) for a in keep]))

    # ---- boundary values that vary along an edge (ns_edge_profile)
    def set_edge_profile(self, edge: int, info) -> None:
        """Per-face bcInfo of one WALL / INLET_UNI edge (the grid's edge order): info[k] at k = the face's column j
        for an x-normal edge (ny values) or its global row i for a y-normal edge (nx values of the whole grid, on
        every rank); entries where the edge has no face are ignored.  Between steps, any number of times."""
        a = np.ascontiguousarray(np.asarray(info, dtype=np.float64).ravel())
        L.check(L.lib().ns_edge_profile(self._h, int(edge), _dptr(a), a.size))

    def clear_edge_profile(self, edge: int) -> None:
        """Back to the edge's own value (its info)."""
        e = self.grid.edges[edge] if 0 <= int(edge) < len(self.grid.edges) else None
        n = 0 if e is None else (self.grid.ny if e.nx != 0 else self.grid.nx)
        L.check(L.lib().ns_edge_profile(self._h, int(edge), None, n))

    # ---- derived fields (ns_derive: one rank)
    def derived(self, p: bool = True, vort: bool = True, div: bool = True, psi: bool = True) -> dict:
        """Pressure, vorticity and divergence as (nx, ny) planes (0 outside a polygon), the stream function at the
        (nx + 1, ny + 1) cell vertices -- each only if asked for -- and ns_derived_stats under its field names (ke,
        enstrophy, div_l2, div_max, cfl, vort_min / max, p_min / max, psi_min / max: NaN without psi).  Between
        steps; all four False is a stats-only pass."""
        nx, ny = self.shape
        want = {"p": p, "vort": vort, "div": div, "psi": psi}
        arrs = {k: np.empty((nx + 1, ny + 1) if k == "psi" else (nx, ny), dtype=np.float64) for k, w in want.items() if w}
        out = L.NsDerived(*[_dptr(arrs[k]) if k in arrs else None for k in ("p", "vort", "div", "psi")])
        st = L.NsDerivedStats()
        L.check(L.lib().ns_derive(self._h, ctypes.byref(out), ctypes.byref(st)))
        return {**arrs, **st.as_dict()}

    # ---- tracer particles (ns_tracers_*: one rank)
    def enable_tracers(self, capacity: int) -> None:
        """Room for `capacity` Lagrangian particles; once per solver.  While particles exist, every step() /
        step_async() carries them by dt in u^n, v^n on the device."""
        L.check(L.lib().ns_tracers_enable(self._h, int(capacity)))
        self._tracers = 0

    def add_tracers(self, x, y) -> None:
        """Append particles at (x, y): physical coordinates relative to the bounding box's lower-left corner, each in
        a domain cell.  All or nothing; indices are stable, so adding between steps draws streaklines."""
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).ravel())
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).ravel())
        if x.size != y.size:
            raise ValueError(f"{x.size} x coordinates, {y.size} y coordinates")
        L.check(L.lib().ns_tracers_add(self._h, _dptr(x), _dptr(y), x.size))
        self._tracers += x.size

    def tracers(self, first: int = 0, n: int | None = None) -> dict:
        """x, y, age, state (NS_TRACER_LIVE / EXITED / STUCK) of particles [first, first + n) (default: all of them)
        and the counts after the latest advance under ns_tracer_stats' field names."""
        st = self.tracer_stats()
        n = st["n"] - first if n is None else int(n)
        x, y, age = (np.empty(max(n, 0), dtype=np.float64) for _ in range(3))
        state = np.empty(max(n, 0), dtype=np.int32)
        L.check(L.lib().ns_tracers_get(self._h, int(first), n, _dptr(x), _dptr(y), _dptr(age),
                                       state.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return {"x": x, "y": y, "age": age, "state": state, **st}

    def tracer_stats(self) -> dict:
        st = L.NsTracerStats()
        L.check(L.lib().ns_tracers_last(self._h, ctypes.byref(st)))
        return st.as_dict()

    def sample_tracers(self):
        """(u, v) at the particles' current positions in the current fields."""
        n = self._tracers   # (not tracer_stats(): ns_tracers_last hands the latest advance's kernel time out once)
        u, v = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64)
        L.check(L.lib().ns_tracers_sample(self._h, _dptr(u), _dptr(v)))
        return u, v

    def advance_tracers(self, dt: float, steps: int = 1) -> None:
        """`steps` advances of dt in the current u, v held fixed (pathlines of a steady field)."""
        L.check(L.lib().ns_tracers_advance(self._h, float(dt), int(steps)))

    def reset_tracers(self) -> None:
        L.check(L.lib().ns_tracers_reset(self._h))
        self._tracers = 0

    # ---- running flow statistics (ns_avg_*: one rank)
    _AVG_KEYS = ("u", "v", "p", "T", "uu", "vv", "uv", "pp", "TT", "uT", "vT")   # NS_AVG_U .. NS_AVG_VT

    def enable_averages(self, every: int = 1, second: bool = True, pressure: bool = False, scalar: bool = False) -> None:
        """Running means of u, v (pressure: and P, scalar: and T -- after enable_scalar) and, with second, the
        Reynolds stresses uu, vv, uv (and pp / TT, uT, vT), accumulated on the device: step k since here (or
        reset_averages) with k % every == 0 samples the state it starts from.  Once per solver.  Pressure
        statistics cost one extra derived-field pass per sample."""
        flags = ((L.NS_AVG_SECOND if second else 0) | (L.NS_AVG_PRESSURE if pressure else 0) |
                 (L.NS_AVG_SCALAR if scalar else 0))
        self.enable_averages_flags(every, flags)

    def enable_averages_flags(self, every: int, flags: int) -> None:
        """ns_avg_enable with the raw NS_AVG_* flag bits."""
        desc = L.NsAvgDesc(int(every), int(flags))
        L.check(L.lib().ns_avg_enable(self._h, ctypes.byref(desc)))
        self._avg_flags = int(flags)

    def sample_averages(self) -> None:
        """One sample of the current fields between steps (how a caller adds the final state)."""
        L.check(L.lib().ns_avg_sample(self._h))

    def reset_averages(self) -> None:
        """n = 0, steps = 0, every plane zero: the spin-up cut-off."""
        L.check(L.lib().ns_avg_reset(self._h))
        self._avg_kept = (0.0, 0)

    def average_plane(self, which: int) -> np.ndarray:
        out = np.empty(self.shape, dtype=np.float64)
        L.check(L.lib().ns_avg_get(self._h, int(which), _dptr(out)))
        return out

    def averages(self) -> dict:
        """The planes accumulated, as (nx, ny) arrays (0 outside a polygon) under the keys u, v, p, T (the means)
        and uu, vv, uv, pp, TT, uT, vT (the population covariances), plus n, the number of samples."""
        f = getattr(self, "_avg_flags", None)
        if f is None:
            L.check(L.lib().ns_avg_get(self._h, L.NS_AVG_U, None))   # (raises: not enabled)
        sec, pr, sc = f & L.NS_AVG_SECOND, f & L.NS_AVG_PRESSURE, f & L.NS_AVG_SCALAR
        have = {"u": True, "v": True, "p": pr, "T": sc, "uu": sec, "vv": sec, "uv": sec, "pp": sec and pr,
                "TT": sec and sc, "uT": sec and sc, "vT": sec and sc}
        n = self._average_counts()[0]
        out = {k: self.average_plane(i) for i, k in enumerate(self._AVG_KEYS) if have[k]}
        out["n"] = n
        return out

    def _average_counts(self):
        # (n and steps without ns_avg_last, which hands the kernel time out once: kept for average_stats)
        st = L.NsAvgStats()
        L.check(L.lib().ns_avg_last(self._h, ctypes.byref(st)))
        keep = getattr(self, "_avg_kept", (0.0, 0))
        self._avg_kept = (keep[0] + st.t_kernel_ms, keep[1] + st.n_kernels)
        return st.n, st.steps

    def average_stats(self) -> dict:
        """n, steps since enable / reset and the sample passes' kernel time since the last call (timing on)."""
        n, steps = self._average_counts()
        t, k = self._avg_kept
        self._avg_kept = (0.0, 0)
        return {"n": n, "steps": steps, "t_kernel_ms": t, "n_kernels": k}

    # ---- wall loads (ns_loads_*: one rank)
    _LOAD_KEYS = ("len", "fpx", "fpy", "fvx", "fvy", "q", "heat", "heat_adv")   # NS_LOAD_LEN .. NS_LOAD_HEAT_ADV
    _FACE_KEYS = ("s", "ds", "p", "tx", "ty", "un", "tb", "qn")

    def enable_loads(self, every: int = 1, capacity: int = 4096) -> None:
        """The scheme's boundary fluxes summed per edge on the device: step k since here (or reset_loads) with
        k % every == 0 appends one record of the state it starts from to a ring of `capacity` records.  Once per
        solver."""
        desc = L.NsLoadDesc(int(every), int(capacity))
        L.check(L.lib().ns_loads_enable(self._h, ctypes.byref(desc)))

    def loads(self) -> list:
        """The current fields' sums, one dict per edge: len, fpx, fpy (pressure force on the wall), fvx, fvy (viscous),
        q (flow rate out), heat (conductive heat rate out), heat_adv."""
        n = len(self.grid.edges)
        out = np.empty((n, L.NS_LOAD_NUM), dtype=np.float64)
        L.check(L.lib().ns_loads_edges(self._h, _dptr(out)))
        return [dict(zip(self._LOAD_KEYS, (float(x) for x in row))) for row in out]

    def wall_faces(self, edge: int) -> dict:
        """The boundary faces of one edge in ascending s: arrays s, ds, p, tx, ty, un, tb, qn of the current fields."""
        n = ctypes.c_int64()
        L.check(L.lib().ns_loads_face_count(self._h, int(edge), ctypes.byref(n)))
        arrs = {k: np.empty(n.value, dtype=np.float64) for k in self._FACE_KEYS}
        out = L.NsLoadFaces(*[_dptr(arrs[k]) for k in self._FACE_KEYS])
        L.check(L.lib().ns_loads_faces(self._h, int(edge), ctypes.byref(out)))
        return arrs

    def load_history(self) -> tuple:
        """(steps[held], records[held, n_edges, 8]) of the ring, oldest first; a record's step is the step number
        since enable / reset, -1 for one taken by sample_loads."""
        held = self._load_counts()[1]
        steps = np.empty(held, dtype=np.int64)
        rec = np.empty((held, len(self.grid.edges), L.NS_LOAD_NUM), dtype=np.float64)
        L.check(L.lib().ns_loads_history(self._h, 0, held, steps.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                         _dptr(rec)))
        return steps, rec

    def sample_loads(self) -> None:
        """One record of the current fields between steps, its step -1."""
        L.check(L.lib().ns_loads_sample(self._h))

    def reset_loads(self) -> None:
        L.check(L.lib().ns_loads_reset(self._h))
        self._load_kept = (0.0, 0)

    def _load_counts(self):
        # (the counters without losing ns_loads_last's kernel time, which is handed out once: kept for load_stats)
        st = L.NsLoadStats()
        L.check(L.lib().ns_loads_last(self._h, ctypes.byref(st)))
        keep = getattr(self, "_load_kept", (0.0, 0))
        self._load_kept = (keep[0] + st.t_kernel_ms, keep[1] + st.n_kernels)
        return st.total, st.held, st.steps

    def load_stats(self) -> dict:
        """total, held, steps since enable / reset and the sampling kernels' time since the last call (timing on)."""
        total, held, steps = self._load_counts()
        t, k = self._load_kept
        self._load_kept = (0.0, 0)
        return {"total": total, "held": held, "steps": steps, "t_kernel_ms": t, "n_kernels": k}

    # ---- passive scalar (ns_scalar_*: one rank's rectangle)
    def enable_scalar(self, pe: float, bc) -> None:
        """A scalar T carried by the step, Peclet number pe.  bc: one ("dirichlet", value) or ("zerograd",)
        per grid edge, in the grid's edge order (cavity.rectangle: W, N, E, S).  T = cT0 = 0 afterwards."""
        kinds = {"dirichlet": L.NS_SBC_DIRICHLET, "zerograd": L.NS_SBC_ZEROGRAD}
        rows = []
        for b in bc:
            if not b or b[0] not in kinds:
                raise ValueError(f"scalar boundary condition {b!r}: ('dirichlet', value) or ('zerograd',)")
            rows.append(L.NsScalarBc(kinds[b[0]], float(b[1]) if b[0] == "dirichlet" else 0.0))
        arr = (L.NsScalarBc * len(rows))(*rows)
        desc = L.NsScalarDesc(pe, len(rows), arr)
        L.check(L.lib().ns_scalar_enable(self._h, ctypes.byref(desc)))
        self._scalar = True

    def scalar(self, cT0: bool = False):
        """T as the nx x ny plane (with cT0=True: T and the previous step's convective term)."""
        T = np.empty(self.shape, dtype=np.float64)
        C = np.empty(self.shape, dtype=np.float64) if cT0 else None
        L.check(L.lib().ns_scalar_get(self._h, _dptr(T), _dptr(C) if cT0 else None))
        return (T, C) if cT0 else T

    def set_scalar(self, T, cT0=None) -> None:
        keep = [None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(self.shape))
                for a in (T, cT0)]
        L.check(L.lib().ns_scalar_set(self._h, *[None if a is None else _dptr(a) for a in keep]))

    def scalar_stats(self) -> dict:
        """The latest step's tmin, tmax, it_t, res_t, t_rhs_kernel_ms, n_rhs_kernels (ns_scalar_last)."""
        st = L.NsScalarStats()
        L.check(L.lib().ns_scalar_last(self._h, ctypes.byref(st)))
        return st.as_dict()

    def set_buoyancy(self, by: float, bx: float = 0.0, tref: float = 0.0) -> None:
        """Boussinesq buoyancy: the body force (bx, by) (T - tref) in the momentum equation (ns_scalar_buoyancy).
        After enable_scalar, between steps; all zero switches it off.  While it is on, NS_ARR_CU / NS_ARR_CV hold
        the convective term minus the force."""
        desc = L.NsBuoyancyDesc(float(bx), float(by), float(tref))
        L.check(L.lib().ns_scalar_buoyancy(self._h, ctypes.byref(desc)))

    def scalar_kernel(self, which: int) -> np.ndarray:
        """ns_scalar_kernel (tests): 1 = the right-hand side alone, 2 = the converged solve of the current rT,
        3 = the right-hand side with the buoyancy force applied to RU / RV / CU / CV (three values)."""
        out = np.zeros(3 if which == 3 else 2, dtype=np.float64)
        L.check(L.lib().ns_scalar_kernel(self._h, which, _dptr(out)))
        return out

    def scalar_rhs(self) -> np.ndarray:
        out = np.empty(self.shape, dtype=np.float64)
        L.check(L.lib().ns_scalar_get_rhs(self._h, _dptr(out)))
        return out

    def kernel(self, which: int, iters: int = 1) -> np.ndarray:
        out = np.zeros(8, dtype=np.float64)
        L.check(L.lib().ns_kernel(self._h, which, iters, _dptr(out)))
        return out

    def mg_restrict(self) -> np.ndarray:
        out = np.zeros((self.shape[0] // 2, self.shape[1] // 2))
        L.check(L.lib().ns_mg_transfer(self._h, 0, _dptr(out)))
        return out

    def mg_prolong(self, coarse) -> None:
        c = np.ascontiguousarray(np.asarray(coarse, dtype=np.float64).reshape(self.shape[0] // 2, self.shape[1] // 2))
        L.check(L.lib().ns_mg_transfer(self._h, 1, _dptr(c)))

    def set_timing(self, on: bool) -> None:
        L.check(L.lib().ns_set_timing(self._h, 1 if on else 0))

    def fill_random(self, seed: int = 0x5EED) -> None:
        L.check(L.lib().ns_fill_random(self._h, seed))

    def time_poisson(self, warmup: int, iters: int):
        out = np.zeros(3, dtype=np.float64)
        L.check(L.lib().ns_time_poisson(self._h, warmup, iters, _dptr(out)))
        return {"avg_ms": out[0], "total_ms": out[1], "span_ms": out[2]}

    def time_poisson_fp32(self, warmup: int, iters: int):
        """Jacobi sweeps on fp32 copies of phi, rhs_phi (configs[4]); also the fp64-summed
        residual^2 of the last sweep's input."""
        out = np.zeros(4, dtype=np.float64)
        L.check(L.lib().ns_time_poisson_fp32(self._h, warmup, iters, _dptr(out)))
        return {"avg_ms": out[0], "total_ms": out[1], "span_ms": out[2], "res2": out[3]}
