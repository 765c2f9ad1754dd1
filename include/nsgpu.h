/*
 * nsgpu.h -- C-ABI of libnsgpu.so, the MI355X (gfx950) implementation of the
 * shivams15/navierstokessolver hot path: FluidSolver::Solve's
 * advect / diffuse / project time step and its pressure-Poisson solve.
 *
 * Plain C types only (no torch / HIP types), so the reference-side host code
 * (navierstokessolver_amd/host/FluidSolver.cpp, ctypes in Python, ...) can bind
 * it directly.  Each entry point names the reference interface it replaces
 * (/root/reference/SRC/<file>:<line>).
 *
 * Conventions
 *   - every call returns 0 on success and a negative NS_E* code on failure;
 *     ns_last_error() holds the message (thread-local).  Nothing throws or aborts.
 *   - the caller owns all host buffers; the library copies them.
 *   - one host thread drives one ns_solver (handles are not thread-safe).
 *   - ns_get_fields / ns_set_fields exchange fields in the reference's compact
 *     cell-id order (the PETSc Vec of FluidSolver.h:6-18; ids i outer / x, j inner / y,
 *     cells outside the polygon skipped: Grid.cpp:149-162).  With nranks > 1 each rank
 *     exchanges its own x-slab: the compact ids ns_local_cells() names, i.e. the
 *     domain's cells in global rows ns_slab_range().  ns_get_array / ns_set_array copy
 *     the slab's nx_local x ny bounding-box plane instead (the same thing for a
 *     rectangle; 0 outside a polygon).
 *   - all state lives in HBM; ns_step() synchronises with the host once per
 *     residual check and once at the end of the step (its ns_stats), mirroring
 *     the reference's per-step printf (FluidSolver.cpp:554-560).
 */
#ifndef NSGPU_H
#define NSGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSGPU_ABI_VERSION 9   /* 2: ns_grid_desc.face_edge (non-rectangular domains);
                                 3: ns_get/set_fields in compact-id order on polygons, ns_local_cells;
                                 4: NS_POISSON_MG is 0, so a zero-initialised ns_params selects the
                                    multigrid (RB-SOR moved to 3; the value 2 is rejected);
                                 5: ns_stats.x_link_bytes appended;
                                 6: ns_stats.t_cycle_kernel_ms / n_cycle_kernels and
                                    t_guess_kernel_ms / n_guess_kernels appended (the finest
                                    level's V-cycle-boundary and guess-forming passes);
                                 7: ns_stats.t_rhs_kernel_ms / n_rhs_kernels (K1) and the direct
                                    Poisson solve's kernel times t_fps_dct_ms / t_fps_tri_ms /
                                    t_fps_idct_ms / n_fps_solves appended;
                                 8: ns_stats.phi_checked appended (res_phi is -1 on a direct solve
                                    whose residual was not computed);
                                 9: ns_stats.t_k5_kernel_ms / n_k5_kernels (K5), t_band_kernel_ms /
                                    n_band_kernels (the Helmholtz wall bands) and k5_deferred appended */

typedef struct ns_solver ns_solver;  /* opaque: device memory, stream, RCCL comm */

/* status codes */
#define NS_OK        0
#define NS_EINVAL   -1  /* bad argument / unsupported configuration */
#define NS_EHIP     -2  /* HIP runtime failure */
#define NS_ERCCL    -3  /* RCCL failure */
#define NS_ENOMEM   -4
#define NS_EDIVERGE -5  /* non-finite values / solver did not converge */

/* boundary-condition types: bcTypes, Grid.h:6 */
#define NS_BC_INLET_UNI       0
#define NS_BC_INLET_PARABOLIC 1  /* rejected by ns_create: empty ghost constant in the reference (FluidSolver.cpp:86-87,
                                    171).  A developed inflow is an INLET_UNI edge carrying ns_parabolic_profile's
                                    values as its ns_edge_profile */
#define NS_BC_WALL            2
#define NS_BC_PRESSURE        3  /* rejected: no ghost stencil in the reference (FluidSolver.cpp:150,168) */
#define NS_BC_NEUMANN         4  /* outflow: velocity ghost q, phi ghost 2.5 phi_0 - 2 phi_1 + 0.5 phi_2
                                    (FluidSolver.cpp:98-101); needs NS_POISSON_MG, whose hierarchy then
                                    preconditions a BiCGStab solve of the true Poisson matrix */

/* Poisson solvers */
#define NS_POISSON_MG     0  /* the default (0): on a rectangle without outflow sides, uniform spacings and
                                ny = 2^p (16 .. 8192) the direct solve -- DCT along y, tridiagonal
                                recurrences along x, inverse DCT: one "iteration", residual ~1e-13,
                                checked periodically and refined by V-cycles if above rtol; elsewhere
                                (NSGPU_FPS=0 everywhere) geometric multigrid V-cycles, RB Gauss-Seidel
                                smoother */
#define NS_POISSON_JACOBI 1  /* weighted Jacobi sweeps (ping-pong) to rtol: O(n^2) sweeps per solve */
#define NS_POISSON_RBSOR  3  /* fused red-black SOR sweeps to rtol: O(n) sweeps per solve */

/* One boundary edge of the polygon (Edge, Grid.h:20-26). */
typedef struct ns_edge {
    int32_t nx, ny;   /* outward normal, one of (+-1,0),(0,+-1) */
    int32_t type;     /* NS_BC_* */
    double  info;     /* bcInfo: wall tangential speed / inlet speed */
} ns_edge;

/* Grid geometry (replaces the Grid object FluidSolver reads, Grid.h:42-69).
 * Rectangle: cell_id == face_edge == NULL and the four sides W,E,S,N each covered by
 * exactly one edge (found by its normal) -- the streaming / multigrid fast path.
 * Any other polygon (steps, holes, split sides; Grid.cpp:131-185): cell_id and
 * face_edge describe it cell by cell over the nx*ny bounding box; the time step then
 * runs the masked kernels, a Jacobi-preconditioned BiCGStab Helmholtz solve and a BiCGStab
 * Poisson solve preconditioned by one V-cycle of the bounding box's multigrid. */
typedef struct ns_grid_desc {
    int32_t nx, ny;           /* cells in x and y (Grid::hx.size(), hy.size()) */
    const double* hx;         /* nx spacings (Grid::hx) */
    const double* hy;         /* ny spacings (Grid::hy) */
    int32_t n_edges;
    const ns_edge* edges;     /* Grid::edges, in vertex order */
    const int32_t* cell_id;   /* nx*ny ids or -1 (outside); NULL = full rectangle */
    const int32_t* face_edge; /* nx*ny*4: boundary edge on the W,E,S,N face or -1 (Cell::edges, Grid.h:33);
                                 required with cell_id */
} ns_grid_desc;

/* Optional host-side transport for the x-slab exchanges (tests, or clusters without
 * RCCL): the library stages ghost rows through pinned host memory and calls these.
 * exchange: send_lo goes to rank-1, send_hi to rank+1; recv_lo is filled from rank-1,
 *           recv_hi from rank+1 (NULL where there is no neighbour); count doubles each.
 * allreduce: in place over n doubles, op 0 = sum, 1 = min.  Both return 0 on success. */
typedef struct ns_host_transport {
    void* user;
    int (*exchange)(void* user, const double* send_lo, const double* send_hi, double* recv_lo, double* recv_hi,
                    int64_t count);
    int (*allreduce)(void* user, double* buf, int32_t n, int32_t op);
} ns_host_transport;

typedef struct ns_params {
    double  dt;               /* FluidSolver::dt */
    double  re;               /* FluidSolver::re */
    int32_t poisson;          /* NS_POISSON_* */
    double  rtol;             /* relative residual tolerance of each solve (reference: 1e-8, FluidSolver.cpp:68,80) */
    int32_t max_iters;        /* sweep cap per solve (0 = 200000) */
    double  omega;            /* Poisson SOR/Jacobi weight (0 = automatic) */
    double  omega_v;          /* Helmholtz SOR weight (0 = 1.0) */
    int32_t check_every;      /* sweeps between residual checks (0 = automatic) */
    int32_t device;           /* HIP device ordinal (-1 = current / LOCAL_RANK) */
    int32_t timing;           /* 1 = time every Poisson sweep kernel with HIP events */
    /* x-slab decomposition over ranks (one process per GPU) */
    int32_t rank, nranks;
    const void* nccl_id;      /* 128-byte ncclUniqueId from rank 0 (NULL if nranks == 1) */
    /* multigrid (NS_POISSON_MG): smoothing sweeps per level before / after the coarse
     * correction, and sweeps of the coarsest solve (0 = defaults 2 / 2 / automatic) */
    int32_t mg_pre, mg_post, mg_coarse_iters;
    const ns_host_transport* host_transport;  /* NULL = RCCL (nranks > 1) */
    double mg_omega;          /* over-relaxation of the red-black smoother (0 = default 1.1:
                               * 4.1 vs 4.6 V-cycles per step at 4096^2, tools/mg_params_sweep.py) */
} ns_params;

/* Per-step result (the reference prints iter, umin, umax, vmin, vmax: FluidSolver.cpp:559-560). */
typedef struct ns_stats {
    double  umin, umax, vmin, vmax;
    int32_t it_u, it_v, it_phi;      /* sweeps of the Helmholtz solves; Poisson sweeps (RB-SOR / Jacobi) or V-cycles (MG) */
    double  res_u, res_v, res_phi;   /* final relative residuals (of the input of the last sweep); res_phi = -1
                                      * when this step's Poisson residual was not computed (phi_checked 0) */
    double  t_poisson_kernel_ms;     /* sum of Poisson sweep-kernel durations (timing == 1; multigrid: the
                                      * finest level's sweeps and prolongation passes) */
    int32_t n_poisson_kernels;       /* number of Poisson sweep kernels timed */
    int32_t n_checks;                /* residual checks (host syncs) in the step */
    double  t_restrict_kernel_ms;    /* multigrid: sum of the finest level's restriction-pass durations (timing == 1) */
    int32_t n_restrict_kernels;      /* number of those passes timed */
    double  t_helm_kernel_ms;        /* single rank: sum of the timed Helmholtz pass durations (one velocity
                                        component each, K2: the two-sweep passes and the 3-sweep passes
                                        with the residual stage -- 24 B/cell either; timing == 1) */
    int32_t n_helm_kernels;          /* number of those passes timed */
    int32_t n_exchanges;             /* ghost-row exchange groups of the step (multi-rank / loopback) */
    int32_t n_allreduces;            /* all-reduces of the step (multi-rank / loopback) */
    double  x_link_bytes;            /* bytes this rank sends over its busiest peer link in the step
                                      * (one side's ghost rows of every exchange + its slab of every
                                      * agglomeration gather; multi-rank / loopback) */
    double  t_cycle_kernel_ms;       /* multigrid, one rank: sum of the finest level's V-cycle-boundary
                                      * pass durations (k_sweep4: cycle c's prolongation + 2 sweeps and
                                      * cycle c+1's 2 sweeps + restriction in one pass; timing == 1) */
    int32_t n_cycle_kernels;         /* number of those passes timed */
    double  t_guess_kernel_ms;       /* multigrid, one rank: sum of the durations of the solves' first
                                      * finest restriction passes that form the phi extrapolation on the
                                      * fly (k_sweep2_gin; timing == 1) */
    int32_t n_guess_kernels;         /* number of those passes timed */
    double  t_rhs_kernel_ms;         /* sum of K1's durations (ConstructRHS_V, k_rhs_s; timing == 1; multi-rank:
                                      * the split launch between marker events) */
    int32_t n_rhs_kernels;           /* number of K1 launches timed */
    double  t_fps_dct_ms;            /* direct Poisson solve (timing == 1): the rows' DCT (k_fps_dct) */
    double  t_fps_tri_ms;            /*   the tridiagonal recurrences along x (k_fps_t1, scan, t2, scan, t3;
                                      *   one interval, allgathers included on slabs) */
    double  t_fps_idct_ms;           /*   the inverse DCT (k_fps_idct) */
    int32_t n_fps_solves;            /* number of direct solves timed */
    int32_t phi_checked;             /* 1: res_phi is this step's Poisson residual, computed and tested against
                                      * rtol (every multigrid / Krylov / sweep solve; the direct solve on its
                                      * first solve, every 16th after it, and on every solve once a checked
                                      * residual came within 1/100 of rtol); 0: a direct solve not checked on
                                      * this step (res_phi = -1) -- a fixed arithmetic sequence whose residual
                                      * the last check measured */
    double  t_k5_kernel_ms;          /* (ABI 9) K5's duration (CorrectVelocities, k_cell_s<5>; timing == 1).  K5 is the
                                      * step's last launch: ns_step reports its own step's, ns_step_async the
                                      * previous step's (read at this step's first host sync, like the monitor) */
    int32_t n_k5_kernels;            /* number of K5 launches timed (0 or 1) */
    double  t_band_kernel_ms;        /* (ABI 9) the Helmholtz wall-band launches (k_helm_band; timing == 1) */
    int32_t n_band_kernels;          /* number of band launches timed */
    int32_t k5_deferred;             /* (ABI 9) 1: this step's K1 applied the previous ns_step_async step's
                                      * CorrectVelocities on the fly (k_rhs_sc: K5 folded into K1, 88 B/cell;
                                      * the async step ends after its Poisson solve) */
} ns_stats;

/* device arrays addressable by ns_get_array / ns_set_array */
#define NS_ARR_U     0  /* u (u* between K2 and K5) */
#define NS_ARR_V     1
#define NS_ARR_PHI   2
#define NS_ARR_CU    3  /* convective derivative of the previous step (convectiveDer_u0) */
#define NS_ARR_CV    4
#define NS_ARR_RU    5  /* RHS_u */
#define NS_ARR_RV    6
#define NS_ARR_RPHI  7  /* RHS_phi (div u* / dt, before mean removal) */
#define NS_ARR_TMP   8  /* Poisson sweep ping-pong partner */
#define NS_ARR_TMPU  9  /* Helmholtz sweep ping-pong partners */
#define NS_ARR_TMPV 10
#define NS_NUM_ARR  11

/* kernels addressable by ns_kernel */
#define NS_K_RHS        1  /* K1 rhs_velocity            (ConstructRHS_V, FluidSolver.cpp:327-363) */
#define NS_K_HELMHOLTZ  2  /* K2 helmholtz sweep x iters  (KSPSolve(uSolver) x2, :547-548) */
#define NS_K_DIV        3  /* K3 divergence + sums        (ConstructRHS_phi, :365-378) */
#define NS_K_POISSON    4  /* K4 Poisson sweep x iters    (KSPSolve(phiSolver), :551) */
#define NS_K_CORRECT    5  /* K5 correct + min/max        (CorrectVelocities, :512-534) */
#define NS_K_HELM_SOLVE 6  /* converged Helmholtz solve   (:547-548) */
#define NS_K_POIS_SOLVE 7  /* converged Poisson solve incl. null-space removal (:550-551) */
#define NS_K_RESIDUAL   8  /* Poisson residual ||rhs - mean - L phi||^2 -> out[0] (no update) */
#define NS_K_POISSON32  9  /* K4 Jacobi x iters on fp32 copies of phi, rhs_phi (fp64 arithmetic and residual,
                              SURVEY.md 8(d) C5); phi <- the fp32 result widened */
#define NS_K_HELM_BAND 10  /* the Helmholtz solve's wall-band relaxation of u, v (k_helm_band: 6 RB-SOR sweeps,
                              two launches of 3, on the cells within max(32, min(nx, ny) / 32) of a wall,
                              the rest held); no output */

/* ---- lifecycle: FluidSolver(char*, Grid*) = SolverInitialize + SolverSetup (FluidSolver.cpp:8-58) ---- */
int  ns_create(const ns_grid_desc* grid, const ns_params* params, ns_solver** out);
void ns_destroy(ns_solver* s);

/* ---- one full time step: the body of FluidSolver::Solve's loop (FluidSolver.cpp:546-560) ---- */
int  ns_step(ns_solver* s, ns_stats* out);
/* the same step without its closing host sync: out's umin..vmax are the PREVIOUS
 * ns_step_async's min/max (NaN on the first), so a caller printing them per step prints the
 * reference's monitor sequence one step late; ns_monitor waits for the latest step's.
 * The host can enqueue the next step while this one's last kernels run. */
int  ns_step_async(ns_solver* s, ns_stats* out);
int  ns_monitor(ns_solver* s, double* mm /* [4]: umin, umax, vmin, vmax */);

/* per-kernel HIP-event timing (ns_params.timing) switched on / off between steps */
int  ns_set_timing(ns_solver* s, int on);

/* ---- state access (host buffers, local slab) ----
 * ns_get_fields / ns_set_fields: compact-id order (prevField->u, v, phi and
 * convectiveDer_u0 / _v0, FluidSolver.h:6-18 / FluidSolver.cpp:40-43), `count` doubles each
 * as ns_local_cells reports; element k is the cell with compact id first_id + k.
 * ns_get_array / ns_set_array: the slab's nx_local x ny bounding-box plane of any NS_ARR_*. */
int  ns_get_fields(ns_solver* s, double* u, double* v, double* phi);
int  ns_set_fields(ns_solver* s, const double* u, const double* v, const double* phi,
                   const double* cu0, const double* cv0);
int  ns_local_cells(ns_solver* s, int64_t* first_id, int64_t* count);
int  ns_get_array(ns_solver* s, int which, double* host);
int  ns_set_array(ns_solver* s, int which, const double* host);

/* ---- individual kernels (tests and bench) ----
 * out (may be NULL) receives kernel-specific scalars:
 *   NS_K_HELMHOLTZ / NS_K_POISSON: out[0] = residual^2 of the last sweep's input
 *   NS_K_DIV:     out[0] = sum rhs, out[1] = sum rhs^2
 *   NS_K_CORRECT: out[0..3] = umin, umax, vmin, vmax
 *   NS_K_*_SOLVE: out[0] = sweeps used, out[1] = final relative residual
 *   NS_K_RESIDUAL: out[0] = residual^2 */
int  ns_kernel(ns_solver* s, int which, int iters, double* out);

/* Multigrid transfers alone (tests): op 0 = restriction of the current residual
 * rhs_phi - mean - L phi into `coarse` (nx/2 x ny/2, host, the slab's coarse rows);
 * op 1 = prolongation: phi += bilinear(`coarse`).  Needs NS_POISSON_MG with >= 2 levels. */
int  ns_mg_transfer(ns_solver* s, int op, double* coarse);

/* Fill phi and rhs_phi with reproducible uniform [-1,1) values generated on the
 * device (splitmix64 of (seed, global cell)), rhs mean-removed: the sweep benchmark input. */
int  ns_fill_random(ns_solver* s, uint64_t seed);

/* Time `iters` Poisson sweep kernels (after `warmup`) with HIP events on the
 * solver's stream: out[0] = average kernel ms, out[1] = total ms. */
int  ns_time_poisson(ns_solver* s, int warmup, int iters, double* out);

/* The same for the fp32-field Jacobi sweep (12 B/cell; configs[4]: "fp32 fields + fp64
 * Poisson residual"): phi and rhs_phi are copied to fp32 planes first (allocated on first
 * use, 3 x 4 B/cell); out[0..2] as above, out[3] = residual^2 of the last sweep's input. */
int  ns_time_poisson_fp32(ns_solver* s, int warmup, int iters, double* out);

/* ---- passive scalar (temperature / dye / concentration) carried by the time step ----
 * An optional field T advanced inside ns_step / ns_step_async by the velocities' scheme: AB2 on the MUSCL /
 * Rusanov convective term div(u T), Crank-Nicolson diffusion with the Peclet number pe in re's place, no
 * pressure term, no coupling back into momentum unless ns_scalar_buoyancy asks for it ("Passive scalar").  A solver without a scalar
 * runs exactly the launches it ran before.  Additive to ABI 9: no struct above changes, the scalar's planes
 * are allocated by ns_scalar_enable (not counted by ns_device_bytes).  One rank's rectangle only
 * (INTEGRATION.md 4): a masked polygon (cell_id != NULL) and nranks > 1 are refused. */
#define NS_SBC_DIRICHLET 0   /* T = value on the edge */
#define NS_SBC_ZEROGRAD  1   /* adiabatic wall / outflow */
typedef struct ns_scalar_bc   { int32_t type; double value; } ns_scalar_bc;
typedef struct ns_scalar_desc { double pe; int32_t n_edges; const ns_scalar_bc* bc; } ns_scalar_desc; /* bc[k] for grid edge k */
typedef struct ns_scalar_stats {
    double  tmin, tmax;          /* of T after the step */
    int32_t it_t;                /* sweeps of the scalar's Helmholtz solve */
    double  res_t;               /* its final relative residual */
    double  t_rhs_kernel_ms;     /* the right-hand side kernel's duration (k_rhs_t; timing == 1) */
    int32_t n_rhs_kernels;       /* launches timed (0 or 1) */
} ns_scalar_stats;
int  ns_scalar_enable(ns_solver* s, const ns_scalar_desc* d);            /* T = 0, cT0 = 0; once per solver */
int  ns_scalar_set(ns_solver* s, const double* T, const double* cT0);    /* compact-id order, either may be NULL */
int  ns_scalar_get(ns_solver* s, double* T, double* cT0);
int  ns_scalar_last(ns_solver* s, ns_scalar_stats* out);                 /* the latest completed step's */
/* tests: which = 1 the right-hand side alone (cT0 <- cT, rT readable by ns_scalar_get_rhs; out[0] = ||rT||^2),
 * 2 = the converged solve of the current rT from the current T (out[0] = sweeps, out[1] = relative residual),
 * 3 = the right-hand side with the buoyancy force (below) applied to the NS_ARR_RU / RV / CU / CV planes as they
 *     stand (out[0] = ||rT||^2, out[1] = ||ru||^2, out[2] = ||rv||^2 of the planes after the call) */
int  ns_scalar_kernel(ns_solver* s, int which, double* out);
int  ns_scalar_get_rhs(ns_solver* s, double* rT);

/* ---- Boussinesq buoyancy: the carried scalar drives the flow ----
 * The body force f = (bx, by) (T - tref) in the momentum equation, AB2 in time like the convective term:
 * dt (1.5 f^n - 0.5 f^{n-1}) joins RHS_u / RHS_v ("Buoyancy").  The force is folded into the stored
 * explicit term: while buoyancy is on, NS_ARR_CU / NS_ARR_CV (and ns_set_fields' cu0 / cv0) hold the convective
 * term MINUS the force, so a restart that carries them over carries the force history too.  Call after
 * ns_scalar_enable, between steps; all-zero coefficients (the state after ns_scalar_enable) switch it off, and the
 * step then runs exactly the launches of a passive scalar.  NS_EINVAL for a solver without a scalar, a NULL
 * descriptor or a coefficient that is not finite.  Additive to ABI 9. */
typedef struct ns_buoyancy_desc { double bx, by, tref; } ns_buoyancy_desc;   /* f = (bx, by) (T - tref) */
int  ns_scalar_buoyancy(ns_solver* s, const ns_buoyancy_desc* d);

/* ---- boundary values that vary along an edge: inlet profiles, shaped lids ----
 * per-face bcInfo of one WALL / INLET_UNI edge: info[k], k = j (x-normal edge, n == ny) or global i (y-normal
 * edge, n == nx of the whole grid, on every rank); entries where the edge has no face are ignored.  The ghost
 * constant of face k is 2 info[k] in the component the edge's own info goes to (an inlet's normal velocity, a
 * wall's tangential one); K1, the implicit half's wall terms, K3 (fused into the direct solve or not) and the
 * scalar's right-hand side read it ("Edge profiles").
 * info == NULL: back to the edge's own value (its ns_edge.info).
 * Between steps, any number of times (time-dependent inflow); ordered on the solver's stream like ns_scalar_set.
 * NS_EINVAL (the message names the edge) for a bad edge index, a NEUMANN edge, n different from the box's extent
 * along the edge, or a value that is not finite.  Flux compatibility of the inlets stays the caller's business.
 * Additive to ABI 9. */
int  ns_edge_profile(ns_solver* s, int32_t edge, const double* info, int32_t n);

/* ---- derived fields on the device: pressure, vorticity, divergence, stream function ----
 * From the current u, v, phi, between steps ("Derived fields"; the normative statement is
 * tests/derived_ref.py).  Face values are Div_V's: r-weighted toward a neighbour in the domain, 0.5 (q + ghost) on a
 * boundary face with that edge's velocity ghost (its profile entry where ns_edge_profile set one).
 *   div  = (u_E - u_W) / hx + (v_N - v_S) / hy          what the approximate projection leaves (K3 without 1 / dt)
 *   vort = (v_E - v_W) / hx - (u_N - u_S) / hy
 *   p    = phi - dt / (2 re) L phi                       ExportData's pressure (L: LHS_phi with its NEUMANN rows)
 *   psi  at the (nx + 1) x (ny + 1) cell vertices, i outer: the volume flux through the vertical line from the box's
 *        bottom to the vertex -- psi(0, 0) = 0, psi(i + 1, 0) = psi(i, 0) - v_S(i, 0) hx[i], psi(i, j + 1) =
 *        psi(i, j) + u_face(i, j) hy[j].  A flux function, not a Poisson solve: path-independent only up to the
 *        column's accumulated div * area.
 * ns_derived: host buffers, NULL = not wanted (and not stored on the device); p, vort, div are nx_local x ny
 * bounding-box planes as ns_get_array's, exactly 0 outside a polygon.  With all four NULL (or out == NULL) the call
 * is a stats-only pass.  A deferred correction (ns_step_async) is settled first, as by ns_get_array; the call runs
 * on the solver's stream, writes no NS_ARR_* plane and none of the step's partial / scalar slots, and keeps the
 * Poisson guess history.  Its device planes are allocated on first use, only those ever asked for (not counted by
 * ns_device_bytes).  NS_EINVAL for a null solver, out and st both NULL, and nranks > 1.  Additive to ABI 9. */
typedef struct ns_derived {
    double* p; double* vort; double* div;
    double* psi;
} ns_derived;
typedef struct ns_derived_stats {
    double  ke, enstrophy;       /* 1/2 sum A (u^2 + v^2), 1/2 sum A vort^2 over the domain's cells, A = hx hy */
    double  div_l2, div_max;     /* sqrt(sum A div^2), max |div| */
    double  cfl;                 /* dt max(|u| / hx + |v| / hy) */
    double  vort_min, vort_max, p_min, p_max;
    double  psi_min, psi_max;    /* NaN when psi was not asked for */
    double  t_kernel_ms;         /* the cell pass (timing == 1) */
    int32_t n_kernels;
} ns_derived_stats;
int  ns_derive(ns_solver* s, const ns_derived* out, ns_derived_stats* st);   /* either may be NULL, not both */

/* ---- Lagrangian tracer particles carried by the time step ----
 * Massless particles that follow the flow on the device ("Tracers"; the normative statement is
 * tests/tracer_ref.py).  Positions are physical coordinates relative to the bounding box's lower-left corner
 * (ns_grid_desc carries no origin: a caller whose grid starts elsewhere subtracts it).  Once enabled and holding
 * particles, every ns_step / ns_step_async advances them by the solver's dt in u^n, v^n, right after K1 -- no host
 * sync is added to the step; a solver that never enables them runs exactly the launches it ran before.
 *   sampling: bilinear between cell centres; where a neighbour is not in the domain, the boundary value 0.5 (q + ghost)
 *             at the boundary face (the edge's velocity ghost, its ns_edge_profile entry where one is set).  Continuous
 *             across interior faces, exact for a field linear in x and y away from boundary faces, discontinuous only
 *             at re-entrant corners.
 *   advance:  AB2, x += dt (1.5 w^n - 0.5 w^{n-1}), an Euler step on a particle's first; age += dt.
 *   fate:     a particle whose new position is in no domain cell does not move: it is EXITED if it left through a
 *             NEUMANN or INLET_UNI face, STUCK at a wall, at a jump past a corner, or on a non-finite value.  A particle
 *             that is not LIVE keeps its position, sample and age and is never touched again.  Keeping the CFL number
 *             below 1 is the caller's business: a jump over a thin divider into another part of the domain lands LIVE.
 * Particle indices are stable (no compaction): a caller follows individuals, and re-injects for streaklines by
 * adding between steps.
 * ns_tracers_enable: once per solver; its planes (44 B per particle of capacity) are not counted by ns_device_bytes.
 * ns_tracers_add:    appends at [n, n + count), all or nothing; new particles are fresh with age 0.
 * ns_tracers_get:    particles [first, first + n); any pointer may be NULL; synchronises.
 * ns_tracers_sample: w at the current positions, n doubles each (a particle that is not LIVE: the sample it froze with).
 * ns_tracers_advance: `steps` advances of dt in the current u, v held fixed (tests; pathlines of a steady field).
 * ns_tracers_reset:  n = 0.
 * ns_tracers_last:   the counts after the latest advance (of a step, or of ns_tracers_advance: seeds added since are
 *                    in n, not yet in live) and that advance's kernel time, handed out once; synchronises.
 * ns_tracers_sample / _advance settle a deferred correction (ns_step_async) first, as ns_get_array does.
 * NS_EINVAL (the message names the cause): a null solver, not enabled, enabled twice, capacity <= 0, nranks > 1
 * (particles would migrate between slabs), an add past the capacity, a seed that is not finite or not in a domain cell
 * (the message gives its index), dt not finite, steps < 0, a get range outside [0, n).  Additive to ABI 9. */
#define NS_TRACER_LIVE   0
#define NS_TRACER_EXITED 1
#define NS_TRACER_STUCK  2
typedef struct ns_tracer_stats {
    int64_t n, live, exited, stuck;
    double  age_max;             /* of the live ones, 0 if none */
    double  t_kernel_ms;         /* the latest advance's particle kernels (timing == 1) */
    int32_t n_kernels;
} ns_tracer_stats;
int  ns_tracers_enable(ns_solver* s, int64_t capacity);
int  ns_tracers_add(ns_solver* s, const double* x, const double* y, int64_t n);
int  ns_tracers_get(ns_solver* s, int64_t first, int64_t n, double* x, double* y, double* age, int32_t* state);
int  ns_tracers_sample(ns_solver* s, double* u, double* v);
int  ns_tracers_advance(ns_solver* s, double dt, int32_t steps);
int  ns_tracers_reset(ns_solver* s);
int  ns_tracers_last(ns_solver* s, ns_tracer_stats* out);

/* ---- running flow statistics: time means and Reynolds stresses accumulated by the time step ----
 * Optional running means of u, v (and on request the pressure P and the carried scalar T) and their central
 * co-moment sums, kept on the device ("Flow statistics"; the normative statement is tests/stats_ref.py).
 * Sample number n + 1 of a source plane x updates, with w = 1.0 / (n + 1) formed on the host in double:
 *   dx = x - xm     xm' = xm + w dx     Sxx' = Sxx + dx (x - xm')     Sxy' = Sxy + dx (y - ym')
 * (dx from x's old mean, ym' y's new one).  Handed out: the means as they stand and S * (1.0 / n), the population
 * covariances <x'y'>.  Co-moments kept with NS_AVG_SECOND: uu, vv, uv; pp with NS_AVG_PRESSURE; TT, uT, vT with
 * NS_AVG_SCALAR; no others.
 *   in the step:   step k since enable / reset (k = 0, 1, ..) with k % every == 0 samples the state the step starts
 *                  from -- u^n, v^n, phi^n, T^n -- on the solver's stream right behind K1, in ns_step and ns_step_async
 *                  alike; no host sync is added.  N steps at every = 1 sample the states 0 .. N - 1.
 *   ns_avg_sample: samples the current fields between steps (a deferred correction is settled first, as by
 *                  ns_get_array): how a caller adds the final state.
 *   ns_avg_reset:  n = 0, steps = 0, every plane zero: the spin-up cut-off.
 *   P:             ns_derive's pressure phi - dt / (2 re) L phi, written by that cell pass into a plane of the
 *                  statistics' own: pressure statistics cost one extra pass of 24 + 8 B/cell per sample.
 * A solver that never enables them runs exactly the launches it ran before.  The planes are allocated by
 * ns_avg_enable (not counted by ns_device_bytes).
 * ns_avg_get:  the nx_local x ny bounding-box plane as ns_get_array's, exactly 0 outside a polygon; all 0 while
 *              n == 0; synchronises.
 * ns_avg_last: n, the steps since enable / reset and the sample passes' kernel time since the last call
 *              (timing == 1; handed out once); synchronises.
 * NS_EINVAL (the message names the cause): a null solver or descriptor, every < 1, unknown flag bits, enabling twice,
 * any other ns_avg_* call before ns_avg_enable, NS_AVG_SCALAR without a scalar, nranks > 1, an unknown `which`, a
 * `which` whose plane this solver does not accumulate.  Additive to ABI 9. */
#define NS_AVG_SECOND   1   /* + uu, vv, uv (and pp / TT, uT, vT of the sources asked for) */
#define NS_AVG_PRESSURE 2   /* + P */
#define NS_AVG_SCALAR   4   /* + T: needs ns_scalar_enable before ns_avg_enable */
typedef struct ns_avg_desc  { int32_t every; int32_t flags; } ns_avg_desc;
typedef struct ns_avg_stats {
    int64_t n;                   /* samples taken since enable / reset */
    int64_t steps;               /* steps since enable / reset */
    double  t_kernel_ms;         /* the sample passes' kernels since the last ns_avg_last (timing == 1) */
    int32_t n_kernels;           /* one per sample, two with NS_AVG_PRESSURE (the derived pass) */
} ns_avg_stats;
#define NS_AVG_U   0   /* the means */
#define NS_AVG_V   1
#define NS_AVG_P   2
#define NS_AVG_T   3
#define NS_AVG_UU  4   /* the covariances <x'y'> */
#define NS_AVG_VV  5
#define NS_AVG_UV  6
#define NS_AVG_PP  7
#define NS_AVG_TT  8
#define NS_AVG_UT  9
#define NS_AVG_VT 10
#define NS_AVG_NUM 11
int  ns_avg_enable(ns_solver* s, const ns_avg_desc* d);   /* once per solver */
int  ns_avg_reset(ns_solver* s);
int  ns_avg_sample(ns_solver* s);
int  ns_avg_get(ns_solver* s, int which, double* plane);
int  ns_avg_last(ns_solver* s, ns_avg_stats* out);

/* ---- wall loads: pressure, shear and heat flux per boundary edge, on the device ----
 * The scheme's own boundary fluxes on every boundary face of the domain and their sums per edge ("Wall
 * loads"; the normative statement is tests/loads_ref.py).  A boundary face is face k (0 W, 1 E, 2 S, 3 N) of a domain
 * cell whose neighbour there is not in the domain; it belongs to the grid edge e that ns_edge_profile and ns_scalar_bc
 * index by.  n = the face's outward normal, h the cell's spacing along n, ds the other one, s the face centre's
 * coordinate along the edge from the box's lower-left corner.  Per face:
 *   p   ns_derive's pressure P of the adjacent cell, on every face type (first order on a NEUMANN face: nothing is
 *       extrapolated to the face)
 *   tx  (ghost(u) - u) / (re h), ty likewise with v: the diffusive momentum flux the scheme passes through the face,
 *       the traction on the fluid; the ghost is the step's own velocity ghost, an edge profile's entry included
 *   un  face(u) n_x + face(v) n_y with the divergence's face values 0.5 (q + ghost)
 *   tb  0.5 (T + ghost(T)), qn = -(ghost(T) - T) / (pe h): the scalar on the face and the conductive heat flux leaving
 *       the fluid; ghost(T) = T on a zero-gradient edge, -T + 2 value on a Dirichlet one.  Exactly 0 without a scalar
 * Per edge the NS_LOAD_NUM sums over its faces, below.  The force of the fluid on the wall is (fpx + fvx, fpy + fvy).
 * The sums are reproducible bit for bit: their order is a function of the face list alone (no floating-point atomics).
 *   in the step:     step k since enable / reset (k = 0, 1, ..) with k % every == 0 appends one record -- k and the
 *                    n_edges x NS_LOAD_NUM sums of the state the step starts from, u^n, v^n, phi^n, T^n -- to a device
 *                    ring of `capacity` records, right behind K1, in ns_step and ns_step_async alike; a full ring
 *                    overwrites its oldest record.  No host sync, wait or readback is added
 *   ns_loads_sample: appends a record of the current fields between steps, its step -1 (a deferred correction is
 *                    settled first, as by ns_get_array)
 *   ns_loads_edges:  the current fields' n_edges x NS_LOAD_NUM sums; no record; synchronises
 *   ns_loads_faces:  the current fields' per-face arrays of one edge in ascending s, ns_loads_face_count entries each;
 *                    any pointer may be NULL; synchronises
 *   ns_loads_history: records [first, first + n) of those held, oldest first: step[n], rec[n][n_edges][NS_LOAD_NUM]
 *                    (either may be NULL); synchronises
 *   ns_loads_reset:  total = held = steps = 0
 *   ns_loads_last:   the counters and the sampling kernels' time since the last call (timing == 1; two launches per
 *                    sample); synchronises
 * A solver that never enables them runs exactly the launches it ran before.  The buffers are allocated by
 * ns_loads_enable (not counted by ns_device_bytes).  The scalar columns exist wherever a scalar does.
 * NS_EINVAL (the message names the cause): a null solver or descriptor, every < 1, capacity < 1, enabling twice, any
 * other ns_loads_* call before ns_loads_enable, a bad edge index, a history range outside [0, held), nranks > 1 (P is
 * the one-rank derived pass's).  Additive to ABI 9. */
#define NS_LOAD_LEN      0   /* sum ds */
#define NS_LOAD_FPX      1   /* sum p n_x ds */
#define NS_LOAD_FPY      2
#define NS_LOAD_FVX      3   /* -sum tx ds */
#define NS_LOAD_FVY      4
#define NS_LOAD_Q        5   /* sum un ds: the flow rate out of the domain */
#define NS_LOAD_HEAT     6   /* sum qn ds */
#define NS_LOAD_HEAT_ADV 7   /* sum un tb ds */
#define NS_LOAD_NUM      8
typedef struct ns_load_desc  { int32_t every; int32_t capacity; } ns_load_desc;
typedef struct ns_load_faces { double *s, *ds, *p, *tx, *ty, *un, *tb, *qn; } ns_load_faces;
typedef struct ns_load_stats {
    int64_t total;               /* samples taken since enable / reset */
    int64_t held;                /* records in the ring: min(total, capacity) */
    int64_t steps;               /* steps since enable / reset */
    double  t_kernel_ms;         /* the sampling kernels since the last ns_loads_last (timing == 1) */
    int32_t n_kernels;           /* two per sample: the face kernel and the edge sums */
} ns_load_stats;
int  ns_loads_enable(ns_solver* s, const ns_load_desc* d);   /* once per solver */
int  ns_loads_sample(ns_solver* s);
int  ns_loads_edges(ns_solver* s, double* out);
int  ns_loads_face_count(ns_solver* s, int32_t edge, int64_t* n);
int  ns_loads_faces(ns_solver* s, int32_t edge, const ns_load_faces* out);
int  ns_loads_history(ns_solver* s, int64_t first, int64_t n, int64_t* step, double* rec);
int  ns_loads_reset(ns_solver* s);
int  ns_loads_last(ns_solver* s, ns_load_stats* out);

/* ---- host-side helpers (no GPU needed) ---- */
/* the face averages of the parabola 6 s (1 - s) * mean over the faces k0 <= k < k1 of spacings h[0..n) (s runs 0..1
 * from face k0's lower end to face k1-1's upper end), 0 elsewhere: the average over [sa, sb] is
 * mean (3 (sa + sb) - 2 (sa^2 + sa sb + sb^2)), and sum out[k] h[k] = mean * (the faces' length) up to round-off
 * on any spacing -- a parabolic and a uniform inlet of the same info carry the same discrete flux */
int  ns_parabolic_profile(const double* h, int32_t n, int32_t k0, int32_t k1, double mean, double* out);
/* the x-slab [i0, i1) of `rank` out of `nranks` for nx cells */
int  ns_slab_range(int32_t nx, int32_t nranks, int32_t rank, int32_t* i0, int32_t* i1);
/* size in bytes of an ncclUniqueId, and produce one (rank 0 only; needs RCCL, no GPU) */
int  ns_nccl_id_size(void);
int  ns_nccl_get_id(void* out128);
/* device bytes one solver allocates for this grid */
int64_t ns_device_bytes(int32_t nx_local, int32_t ny);
/* version / last error */
int  ns_abi_version(void);
const char* ns_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* NSGPU_H */
