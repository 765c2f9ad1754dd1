// ns_knobs.h -- every NSGPU_* environment knob of libnsgpu.so, read ONCE per solver (ns_create stores the
// result in ns_solver::k; the launchers take it as an argument).  Host-only: no HIP include.
//
// Most knobs are the equivalence oracles of the GPU tests (the A/B partner of a default path) or measurement
// hooks.  A field's initialiser is its default; a knob whose default depends on the grid or the decomposition
// keeps an "unset" value here and the decision stays where it is made (ns_solver.cpp choose_paths).
// A new knob: one field, one line in from_env().
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace nsg {

struct Knobs {
    enum { RHS_STREAM = 0, RHS_LDS = 1, RHS_GLOBAL = 2 };

    // ---- kernel variants of the time step (A/B partners of the default launches)
    int rhs = RHS_STREAM;      // NSGPU_RHS: K1 as k_rhs_s strips (unset), =global the global-load k_rhs, any other value (lds) k_rhs_lds + k_rhs_bc
    int k1s = 0;               // NSGPU_K1S=3 / 24 / 32 / 33: the streaming K1's builds (waves, rows in flight, hy tables in SGPRs)
    int k1_l = 0;              // NSGPU_K1_L=n (>= 4): K1's rows per strip (0: one resident round)
    int cell_grid = 0;         // NSGPU_CELL=grid: the thread-per-cell K3 / K5 / apply instead of the k_cell_s strips (and k_rhs_t_grid for k_rhs_t)
    int mask_cell = 1;         // NSGPU_MASK_CELL=0: a masked domain's K3 / K5 as thread-per-cell k_div / k_correct<TopoMask>
    int apply_grid = 0;        // NSGPU_APPLY=grid: the Poisson operator by k_apply only
    int sd3 = 0;               // NSGPU_SD3=2 / 3: rows in flight of the residual 3-sweep pass (0: 2 for two fields, 3 for one)
    int cv_blk = 1;            // NSGPU_CV_BLK=0: the LDS coarse V-cycle's cell-loop smoother instead of the 2 x 2 blocks
    int strip_rows = 0;        // NSGPU_STRIP_ROWS=n: rows per streaming strip (even, 4..64; 0 = adaptive)
    int tiled = 0;             // NSGPU_SWEEP=tiled: the first (LDS-tiled) single-sweep kernels
    int sweep3 = 1;            // NSGPU_SWEEP3=0: Helmholtz batches as pairs only (no k_sweep3 pass)
    int sweep3_res = 1;        // NSGPU_SWEEP3_RES=0: Helmholtz batches end on pairs, not on a 3-sweep pass with its residual
    int helm_uv = 1;           // NSGPU_HELM_UV=0: one rank's 3-sweep batch as two one-field launches
    int helm_band = 1;         // NSGPU_HELM_BAND=0: no wall-band relaxation before the global Helmholtz passes
    int band6 = 0;             // NSGPU_BAND6=1: 6 band sweeps as one k_helm_band6 launch + copy-back (measured slower)
    int band_w = -1;           // NSGPU_BAND_W=n (>= 1): the wall bands' width in cells (-1: from the grid)
    int band_sweeps = -1;      // NSGPU_BAND_SWEEPS=n: their RB-SOR sweeps, a multiple of 3, >= 3 (-1: from the grid)
    int ext_timing = 1;        // NSGPU_EXT_TIMING=0: marker events around timed launches instead of dispatch stamps
    int speculate = 1;         // NSGPU_SPECULATE=0: no speculative K5 / K3 behind a residual check
    int k5_guess = 0;          // NSGPU_K5_GUESS=1: K5 forms the next step's Poisson guess (k_cell_s<6>; measured no gain)
    int k5_defer = 1;          // NSGPU_K5_DEFER=0: K5 at every async step's end instead of inside the next step's K1

    // ---- multigrid Poisson solve
    int fuse_restrict = 1;     // NSGPU_FUSED_RESTRICT=0: a separate k_restrict pass
    int fuse_prolong = 1;      // NSGPU_FUSED_PROLONG=0: a separate k_prolong pass
    int tile_small = 1;        // NSGPU_TILE_SMALL=0: no LDS-tiled fused passes on small levels
    int fuse4 = 1;             // NSGPU_FUSE4=0: no k_sweep4 V-cycle boundary (the two passes)
    int gin = 0;               // NSGPU_GIN=1: the phi extrapolation inside the first restriction pass (measured slower)
    int mg_predict = 1;        // NSGPU_MG_PREDICT=0: a residual check (host sync) after every V-cycle
    int phi_extrap = -1;       // NSGPU_PHI_EXTRAP=0..4: the Poisson guess's order (-1: cubic, or none on a direct solve)
    double mg_omega = 0.0;     // NSGPU_MG_OMEGA=w: the smoother's over-relaxation, if mg_omega_set (else ns_params' or 1.1)
    int mg_omega_set = 0;
    long pair_min_cells = 2048L * 2048L;   // NSGPU_PAIR_MIN_CELLS: smallest level smoothed in streamed 2-sweep passes
    long direct_cells = 128L * 128L;       // NSGPU_DIRECT_CELLS: largest coarsest level solved exactly (0: the LDS V-cycle)
    long agg_cells = 1024L * 1024L;        // NSGPU_AGG_CELLS: multi-rank, levels below this many cells live whole on every rank
    int outflow_pc_wall = 0;   // NSGPU_OUTFLOW_PC=wall: round 1's wall closure instead of the outflow side's line solve

    // ---- direct Poisson solve (ns_fps.hip)
    int fps = 1;               // NSGPU_FPS=0: the multigrid where the direct solve applies
    int fps_dense = 1;         // NSGPU_FPS_DENSE=0: the multigrid where the dense y transforms apply
    int fps_outflow = 1;       // NSGPU_FPS_OUTFLOW=0: the channel's BiCGStab path instead of its direct solve
    int fps_check = 16;        // NSGPU_FPS_CHECK=n: the solve's residual on every n-th in-step solve (1 = every solve)
    int fps_passes = 0;        // NSGPU_FPS_PASSES=3: the recurrences' three-pass form (0: unset, two passes)
    int fps_fuse = -1;         // NSGPU_FPS_FUSE=0: K3 and the DCT as two launches (-1: fused where a fused form exists)
    int fps_real = 1;          // NSGPU_FPS_REAL=0: the row-pair transforms where the one-row real-input ones apply
    int fps_grid = 0;          // NSGPU_FPS_GRID=n: the pair transforms' workgroup cap (0: one workgroup per row pair)
    int fps_ptab = 2;          // NSGPU_FPS_PTAB=0 / 1 / 2: pivots by division / from a table / per-block fixed point
    int fps_onegather = 1;     // NSGPU_FPS_ONEGATHER=0: multi-rank, two allgathers per solve
    int fps_defer = 1;         // NSGPU_FPS_DEFER=0: multi-rank, the mean's all-reduce before the solve
    int fps_pc = 1;            // NSGPU_FPS_PC=0: a masked domain's box V-cycle preconditioner instead of the box's direct solve
    int cap = 1;               // NSGPU_CAP=0: a masked domain's BiCGStab instead of the capacitance solve
    long cap_max = 4096;       // NSGPU_CAP_MAX=n: most interface faces of a capacitance matrix
    int cap_outflow = 1;       // NSGPU_CAP_OUTFLOW=0: no box solve for a masked domain whose box has the E outflow

    // ---- masked domains' Helmholtz solve
    int mask_rb = 1;           // NSGPU_MASK_HELM=krylov: BiCGStab instead of red-black SOR
    int mask_rbt = 1;          // NSGPU_MASK_RBT=0: red-black half-sweep launches only (no LDS-tiled whole sweep)
    int mask_mt = 1;           // NSGPU_MASK_MT=0: one sweep per launch (no k_helm_mt_mask temporal blocking)
    int mask_band = 6;         // NSGPU_MASK_BAND=n: wall-band sweeps before the global ones, a multiple of 6 (0: none)
    int mask_band_w = -1;      // NSGPU_MASK_BAND_W=n (>= 1): those bands' width (-1: from the grid)

    // ---- multi-rank
    int overlap = -1;          // NSGPU_OVERLAP=0: exchange, then the whole pass (-1: exchanges overlap the interior strips)
    int comm_cus = 0;          // NSGPU_COMM_CUS=n: CUs reserved for the comm stream (0: no CU masks)
    int bus = 1;               // NSGPU_BUS=0: per-reduction all-reduces instead of the scalar bus
    int deep = 1;              // NSGPU_DEEP=0: no deep ghost rows (one exchange group per launch as in r4)

    // ---- test / measurement hooks
    int loopback = 0;          // NSGPU_RCCL_LOOPBACK=1: a 1-rank RCCL communicator whose every peer is this process
    char virtual_iters[4096] = "";   // NSGPU_VIRTUAL_ITERS="h:c,h:c,...": a virtual slab's replayed sweeps / V-cycles per step
    int virtual_iters_len = 0;       // its length in the environment: a list that does not fit stays empty (ns_create refuses it)
    int virtual_copy = 0;      // NSGPU_VIRTUAL_COPY=1: a virtual slab's allgather slot by a device copy
    int time_pairs = 0;        // NSGPU_TIME_PAIRS (set): ns_time_poisson times the two-sweep pass
    int verbose = 0;           // NSGPU_VERBOSE=1: the chosen paths and residual histories on stderr

    static Knobs from_env() {
        Knobs k;
        const auto env = [](const char* name) { return std::getenv(name); };
        // 0 / 1 switches, plain integers, and strings with one recognised value
        const auto flag = [&](const char* name, int& v) { if (const char* e = env(name)) v = std::atoi(e) != 0; };
        const auto num = [&](const char* name, int& v) { if (const char* e = env(name)) v = std::atoi(e); };
        const auto lnum = [&](const char* name, long& v) { if (const char* e = env(name)) v = std::atol(e); };
        const auto is = [&](const char* name, const char* val) { const char* e = env(name); return e && !std::strcmp(e, val); };

        if (const char* e = env("NSGPU_RHS")) k.rhs = std::strcmp(e, "global") ? RHS_LDS : RHS_GLOBAL;
        num("NSGPU_K1S", k.k1s);
        num("NSGPU_K1_L", k.k1_l);
        k.cell_grid = is("NSGPU_CELL", "grid");
        flag("NSGPU_MASK_CELL", k.mask_cell);
        k.apply_grid = is("NSGPU_APPLY", "grid");
        num("NSGPU_SD3", k.sd3);
        num("NSGPU_CV_BLK", k.cv_blk);
        num("NSGPU_STRIP_ROWS", k.strip_rows);
        k.strip_rows = k.strip_rows >= 4 ? (std::min(k.strip_rows, 64) & ~1) : 0;
        k.tiled = is("NSGPU_SWEEP", "tiled");
        flag("NSGPU_SWEEP3", k.sweep3);
        flag("NSGPU_SWEEP3_RES", k.sweep3_res);
        num("NSGPU_HELM_UV", k.helm_uv);
        flag("NSGPU_HELM_BAND", k.helm_band);
        flag("NSGPU_BAND6", k.band6);
        if (const char* e = env("NSGPU_BAND_W")) k.band_w = std::max(1, std::atoi(e));
        if (const char* e = env("NSGPU_BAND_SWEEPS")) k.band_sweeps = std::max(3, std::atoi(e) / 3 * 3);
        flag("NSGPU_EXT_TIMING", k.ext_timing);
        flag("NSGPU_SPECULATE", k.speculate);
        flag("NSGPU_K5_GUESS", k.k5_guess);
        flag("NSGPU_K5_DEFER", k.k5_defer);

        flag("NSGPU_FUSED_RESTRICT", k.fuse_restrict);
        flag("NSGPU_FUSED_PROLONG", k.fuse_prolong);
        flag("NSGPU_TILE_SMALL", k.tile_small);
        flag("NSGPU_FUSE4", k.fuse4);
        flag("NSGPU_GIN", k.gin);
        flag("NSGPU_MG_PREDICT", k.mg_predict);
        if (const char* e = env("NSGPU_PHI_EXTRAP")) k.phi_extrap = std::max(0, std::min(4, std::atoi(e)));
        if (const char* e = env("NSGPU_MG_OMEGA")) { k.mg_omega = std::atof(e); k.mg_omega_set = 1; }
        lnum("NSGPU_PAIR_MIN_CELLS", k.pair_min_cells);
        lnum("NSGPU_DIRECT_CELLS", k.direct_cells);
        k.direct_cells = std::max(0L, k.direct_cells);
        lnum("NSGPU_AGG_CELLS", k.agg_cells);
        k.outflow_pc_wall = is("NSGPU_OUTFLOW_PC", "wall");

        flag("NSGPU_FPS", k.fps);
        flag("NSGPU_FPS_DENSE", k.fps_dense);
        flag("NSGPU_FPS_OUTFLOW", k.fps_outflow);
        if (const char* e = env("NSGPU_FPS_CHECK")) k.fps_check = std::max(0, std::atoi(e));
        if (const char* e = env("NSGPU_FPS_PASSES")) k.fps_passes = std::atoi(e) == 3 ? 3 : 2;
        flag("NSGPU_FPS_FUSE", k.fps_fuse);
        flag("NSGPU_FPS_REAL", k.fps_real);
        num("NSGPU_FPS_GRID", k.fps_grid);
        num("NSGPU_FPS_PTAB", k.fps_ptab);
        flag("NSGPU_FPS_ONEGATHER", k.fps_onegather);
        flag("NSGPU_FPS_DEFER", k.fps_defer);
        flag("NSGPU_FPS_PC", k.fps_pc);
        flag("NSGPU_CAP", k.cap);
        lnum("NSGPU_CAP_MAX", k.cap_max);
        flag("NSGPU_CAP_OUTFLOW", k.cap_outflow);

        k.mask_rb = !is("NSGPU_MASK_HELM", "krylov");
        flag("NSGPU_MASK_RBT", k.mask_rbt);
        flag("NSGPU_MASK_MT", k.mask_mt);
        if (const char* e = env("NSGPU_MASK_BAND")) k.mask_band = std::max(0, std::atoi(e) / 6 * 6);
        if (const char* e = env("NSGPU_MASK_BAND_W")) k.mask_band_w = std::max(1, std::atoi(e));

        flag("NSGPU_OVERLAP", k.overlap);
        if (const char* e = env("NSGPU_COMM_CUS")) k.comm_cus = std::max(0, std::atoi(e));
        flag("NSGPU_BUS", k.bus);
        flag("NSGPU_DEEP", k.deep);

        flag("NSGPU_RCCL_LOOPBACK", k.loopback);
        if (const char* e = env("NSGPU_VIRTUAL_ITERS")) {
            k.virtual_iters_len = (int)std::strlen(e);
            if ((size_t)k.virtual_iters_len < sizeof k.virtual_iters) std::strcpy(k.virtual_iters, e);
        }
        flag("NSGPU_VIRTUAL_COPY", k.virtual_copy);
        k.time_pairs = env("NSGPU_TIME_PAIRS") != nullptr;
        flag("NSGPU_VERBOSE", k.verbose);
        return k;
    }
};

}  // namespace nsg
