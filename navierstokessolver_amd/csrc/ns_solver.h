// ns_solver.h -- what ns_solver.cpp (the step: Helmholtz and Poisson orchestration, the passive scalar) and
// ns_observe.cpp (the observers of the flow: derived fields, tracers, flow statistics, wall loads) share: the error
// macros, the solver's state and a few helpers.  Private to those two files; no .hip file includes it.
//
// A new observer touches: its kernels' .hip, its state struct here (owned buffers: dev_ptr / pinned_ptr, so that
// observers_free and a failed *_enable need no list), its entry points and step hook in ns_observe.cpp and, if it is
// timed, one trows<> table in ns_timing.h.
#pragma once
#include <rccl/rccl.h>
#include <rocblas/rocblas.h>

#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/nsgpu.h"
#include "ns_internal.h"
#include "ns_timing.h"

namespace nss {

void set_err(const char* fmt, ...);   // the calling thread's ns_last_error text (ns_solver.cpp)

#define HIPCHK(x)                                                                        \
    do {                                                                                 \
        hipError_t e_ = (x);                                                             \
        if (e_ != hipSuccess) {                                                          \
            nss::set_err("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return NS_EHIP;                                                              \
        }                                                                                \
    } while (0)

#define NCCLCHK(x)                                                                          \
    do {                                                                                    \
        ncclResult_t r_ = (x);                                                              \
        if (r_ != ncclSuccess) {                                                            \
            nss::set_err("%s failed: %s (%s:%d)", #x, ncclGetErrorString(r_), __FILE__, __LINE__); \
            return NS_ERCCL;                                                                \
        }                                                                                   \
    } while (0)

#define CHK(x)                 \
    do {                       \
        int rc_ = (x);         \
        if (rc_ != 0) return rc_; \
    } while (0)

// device scalar slots
enum {
    S_DIVSUM = 0,   // 2: sum rhs, sum rhs^2
    S_SHIFT = 2,    // 2: mean, ||rhs - mean||^2
    S_HBN = 4,      // 2: ||ru||^2, ||rv||^2
    S_RES = 6,      // 2: residual^2 (u, v) or (phi, -)
    S_MM = 8,       // 4: umin, -umax, vmin, -vmax
    S_AUX = 12,     // 4
    S_KSHIFT = 16,  // 1: the Krylov solves' shift after consistent_rhs (see there)
    // multi-rank scalar bus (r5, bus()): this rank's partial values, gathered from every rank and folded
    // into the global slots above -- K1's ||RHS||^2 (-> S_HBN), the Helmholtz residuals (-> S_RES, S_AUX)
    // and the previous K5's min / max (-> S_MM); contiguous, in this order
    S_HBNL = 18,    // 2
    S_RESL = 20,    // 2
    S_AUXL = 22,    // 2
    S_MML = 24,     // 4
    S_KRY = 28,     // 7: (r5) a BiCGStab batch's verdict for the host (KS_STOP, KS_BRK, KS_IT, KS_R2, r.r, alpha, omega)
    S_OE = 35,      // 1: (r6) slabs with an E outflow: mode 0's projected shift 2 f'_{n-1}, all-reduced
    S_NUM = 36
};
constexpr int BUS_NV = 10, BUS_NSUM = 6;

// the step's kernel timings: the recorder of ns_timing.h over HIP events (nsg::HipTiming)
using Timing = nsg::Timing<nsg::HipTiming>;
#define TCHK(x) HIPCHK(static_cast<hipError_t>(x))

// device and pinned host memory with an owner: freed when the owner goes, or is assigned a fresh state
struct DevFree { void operator()(void* p) const { (void)hipFree(p); } };
struct PinnedFree { void operator()(void* p) const { (void)hipHostFree(p); } };
template <class T> using dev_ptr = std::unique_ptr<T[], DevFree>;
template <class T> using pinned_ptr = std::unique_ptr<T[], PinnedFree>;

}  // namespace nss

// one multigrid level (level 0 = the solver's own PHI / TMP / RPHI arrays)
struct MgLevel {
    nsg::Geo g{};
    nsg::Coef c{};
    double *phi = nullptr, *tmp = nullptr, *b = nullptr;  // current iterate, ping-pong partner, rhs
    double* mem = nullptr;                               // planes (levels >= 1)
    double* coef = nullptr;                              // coefficient tables (levels >= 1)
    std::vector<double> hx, hy;                          // host spacings
    int minrows = 0;                                     // fewest rows any rank holds of this level
    // coarse-level agglomeration (nranks > 1): a replicated level lives WHOLE on every rank
    // (g.i0 = 0, g.nxl = g.nx) and is smoothed with no exchange.  The first replicated level
    // is reached from the last distributed one through this rank's slab of it (gs) and
    // gathered (every rank's rows si0[q] .. si0[q] + sn[q]) after the restriction.
    bool repl = false;
    // multi-rank: the rhs ghost rows are owed -- they travel with the level's next overlapped
    // FUSE_R exchange instead of in an exchange round of their own (flush_b otherwise)
    bool b_pend = false;
    // the level's iterate is identically zero but not stored (the restriction from the level
    // above skipped its phi := 0 writes): its first pass -- the fused restriction pass or the LDS
    // coarse V-cycle -- takes it as zero without reading it or its ghost rows; any other consumer
    // materialises the zeros first (zero_phi)
    bool zero = false;
    // multi-rank: the iterate's 5 ghost rows were sent right after this level's fused restriction
    // pass (riding on the next exchange group down the V-cycle): the prolongation pass needs no
    // exchange of its own for them -- phi is not written in between
    bool phi_ghost = false;
    nsg::Geo gs{};
    std::vector<int> si0, sn;
};

struct ns_solver {
    nsg::Knobs k;                // the NSGPU_* environment at ns_create (ns_knobs.h): fixed for the solver's life
    nsg::Geo g{};
    nsg::Coef c{};
    int device = 0;
    hipStream_t st = nullptr;
    double dt = 0, re = 0, rtol = 1e-8, omega = 0, omega_v = 1.0;
    int poisson = NS_POISSON_MG, max_iters = 200000, check_every = 0, timing = 0;
    double* base = nullptr;      // all fields
    size_t plane = 0;            // doubles per field plane
    double* arr[NS_NUM_ARR] = {};  // pointer to local row 0 of each field
    double* coef = nullptr;      // device coefficient tables
    double* part = nullptr;      // per-block partials
    double* scal = nullptr;      // device scalars
    double* hs = nullptr;        // pinned host mirror of scal
    int rank = 0, nranks = 1;
    ncclComm_t comm = nullptr;
    double ncells = 0;           // global cell count
    // timed steps (timing == 1): every timed kernel call is an interval of this recorder, by kind (ns_timing.h) --
    // drained where a host sync has passed them: the multigrid's at each residual check, the Helmholtz passes', K1's
    // and the wall bands' after helm_solve, K5's at the next host sync (the next step's, after ns_step_async), the
    // direct solve's after waiting for its own last event, the scalar's in scalar_end
    nss::Timing tm;
    int helm_batch0 = 4, pois_batch0 = 8;
    int helm_next = 4;           // first Helmholtz batch of the next step (adaptive unless check_every)
    int helm_adapt = 1;
    // the Helmholtz wall bands (k.helm_band): their width (cells from a wall: min(nx, ny) / 32) and RB-SOR sweeps (a
    // multiple of 3).  (r6) k.band6, 6 band sweeps as ONE k_helm_band6 launch + copy-back: half the band bytes, but
    // the launches are latency-bound, not HBM-bound -- 100 + 13 us against 2 x 48.5 (profiles/r06/ab/): off
    int band_w = 128, band_sweeps = 6;
    int helm_probe = 0;          // steps since the Helmholtz first-pass residual was last sampled
    int phi_extrap = 3;          // Poisson initial guess: 0 phi^{n-1}, 1 linear, 2 quadratic, 3 (default) cubic while
                                 // the last solve took > 1 V-cycle, else quadratic; 0 on a direct solve (choose_paths)
    double mg_rate2 = 0.0;       // last measured per-cycle contraction of ||r||^2
    int mg_hist[4] = {-1, -1, -1, -1};   // V-cycles the last four solves converged at (first check)
    double* phim = nullptr;      // phi^{n-2} (the extrapolation's second point; rotates with PHI / TMP)
    double* phim2 = nullptr;     // phi^{n-3} (quadratic / cubic extrapolation)
    double* phim3 = nullptr;     // phi^{n-4} (cubic extrapolation)
    double* phim4 = nullptr;     // phi^{n-5} (quartic, NSGPU_PHI_EXTRAP=4: A/B only)
    double* phim_mem = nullptr;  // the extra planes' allocation
    float* f32_mem = nullptr;    // fp32-field sweep planes (configs[4]), allocated on first use
    float* f32[3] = {};          // phi, its ping-pong partner, rhs_phi (rows of g.ld floats)
    int phim_valid = 0;          // history planes holding data (0 after a reset / an injected phi)
    // multi-rank: ghost-row exchanges of the two-sweep passes run on a comm stream while the
    // pass's interior strips run (NSGPU_OVERLAP=0: exchange, then the whole pass)
    int overlap = 1;
    int helm_b_pend = 0;          // RHS_u / RHS_v ghost rows owed to the first Helmholtz pair pass
    // ghost-row requests riding on the NEXT exchange group (halo_reqs / gather_level), e.g. a
    // multigrid level's post-restriction iterate (MgLevel::phi_ghost)
    struct Piggy { const nsg::Geo* g; double* f; int w; };
    Piggy piggy[4];
    int npiggy = 0;
    hipStream_t cst = nullptr;
    // multi-rank: CUs reserved for the comm stream (its RCCL kernels run beside the compute
    // stream's strips instead of queueing behind them; NSGPU_COMM_CUS, 0 = no masks)
    int comm_cus = 0, compute_cus = 0;
    hipEvent_t xev[2] = {nullptr, nullptr};
    hipEvent_t fev = nullptr;     // fetch_begin / fetch_end: the scalars' copy to the host is done
    int k1_red_nb = 0;            // (r7) K1''s partials wait for the Helmholtz check's reduction launch (their count)
    // ns_step_async: the step's min/max travel to mm_host behind the step's last kernel (mev);
    // read by the next ns_step_async (after that step's first host sync) or by ns_monitor
    double* mm_host = nullptr;
    hipEvent_t mev = nullptr;
    int mm_pending = 0;
    int extrap_pending = 0;       // ns_step: the phi extrapolation waits to hide a host sync
    std::vector<MgLevel> lv;     // multigrid hierarchy (NS_POISSON_MG)
    int mg_pre = 2, mg_post = 2, mg_coarse_iters = 0;
    double mg_omega_c = 1.0, mg_omega_s = 1.1;
    bool mg_coarse_lds = false;
    // r4: the coarsest level solved exactly by its separable eigen-decomposition (k_direct, two
    // launches): the first whole coarse level of <= k.direct_cells cells (default 128^2; 0 = the LDS
    // V-cycle below it as in round 3).  dmat: P1 = Vx^-1, Q1 = Vy^-T, E, P2 = Vx,
    // Q2 = Vy^T (direct_setup), padded to multiples of 16
    // r4: a V-cycle boundary on the finest level in one pass (k_sweep4, k.fuse4): cycle c's prolongation
    // pass is deferred when c's output is not checked (p_pending) and runs fused with cycle c+1's
    // restriction pass
    bool p_pending = false;
    // r4: the phi extrapolation formed inside the solve's first restriction pass (k_sweep2_gin) instead
    // of by k_axpby: extrapolate_phi only rotates the planes and leaves the guess's sources here;
    // K3 then runs speculatively behind the Helmholtz check.  Measured (r4, 4096^2 driver form): the
    // pass takes 241 us (184 VGPRs, 2 waves / SIMD, five streams) against FUSE_R 87 + k_axpby 104 us,
    // 9,924-9,961 vs 9,957-10,143 MLUPS -- so opt-in (k.gin); default k_axpby (round 3)
    bool gin_pending = false;
    const double* gin_src[4] = {nullptr, nullptr, nullptr, nullptr};
    double gin_c[4] = {0, 0, 0, 0};
    bool mg_direct = false;
    double* dmat = nullptr;
    const double *dP1 = nullptr, *dQ1 = nullptr, *dE = nullptr, *dP2 = nullptr, *dQ2 = nullptr;
    // NEUMANN outflow (pois_solve_krylov): BiCGStab planes r, r0, p, v, s, t, ph, sh, scratch
    // (null without an outflow side) and the recurrence scalars
    double* kv[9] = {};
    double* kv_mem = nullptr;
    double* lrow = nullptr;      // outflow preconditioner: its line solution (one row, in kv_mem)
    double* cvimg = nullptr;     // the LDS coarse V-cycle's image (nsg::cv_image), cv_n doubles
    int cv_n = 0, cv_dn = 0;
    double* ksc = nullptr;
    bool pc_active = false;      // inside mg_precond: level 0 has no mean shift
    bool krylov_mg = false;      // the Poisson BiCGStab is preconditioned by a V-cycle (else Jacobi)
    // the outflow preconditioner: a rectangle whose only NEUMANN side is W (0) or
    // E (1): the V-cycle's hierarchy closes that side with a Dirichlet-centre ghost whose data,
    // on the finest level, is the side's 1-D line solve (launch_line_solve); -1 = walls
    int out_side = -1;
    bool consist = false;        // stretched grid, no outflow: consistent_rhs() before every Poisson solve
    bool fps_xuni = true;        // (r6) the direct solve's hx is uniform (false: x-stretched, unfused, no pivot fixed points)
    // (r6) the dense y transforms (hy stretched, or an ny no FFT plan takes): Ly's eigenvectors through rocSOLVER's
    // tridiagonal eigensolver at create, the transforms as rocBLAS GEMMs (F: forward, G: inverse, N x N each)
    bool fps_dense = false;
    rocblas_handle rb = nullptr;
    double area = 0.0;           // sum of the domain's cell areas
    double inv_area = 0.0;       // sum of their reciprocals
    int32_t* fc_mem = nullptr;   // masked domain: topology plane (g.fc) and edge table (g.et)
    int32_t* mband_tiles = nullptr;   // (r6) masked, one rank: the (li0, j0) of the mt tiles holding a wall-band cell
    int mband_n = 0;
    int32_t* ecell_mem = nullptr;   // (r5) masked domain: the slab's domain cells that are not FC_DEEP (g.ecell)
    nsg::EdgeDev* et_mem = nullptr;
    std::vector<nsg::EdgeDev> et_host;   // ... and its host copy (re-uploaded when an edge's profile pointer changes)
    // edge profiles (ns_edge_profile): per edge its type and normal, the rectangle side it covers (-1 on a masked
    // domain) and the device table of 2 info(k) with its host copy (ny entries for an x-normal edge, nx for a y-normal
    // one; allocated on first use)
    struct EdgeProf {
        int type = 0, enx = 0, eny = 0, side = -1;
        std::vector<double> host;
        double* tab = nullptr;
    };
    std::vector<EdgeProf> eprof;
    ns_host_transport ht{};      // host transport (ht.exchange != NULL) instead of RCCL
    double* stage = nullptr;     // pinned staging for the host transport
    size_t stage_n = 0;
    // masked domain: this slab's bounding-box cells -> compact cell id - cid0 (-1 outside), so
    // ns_get_fields / ns_set_fields speak the reference's compact Vec order (Grid.cpp:149-162)
    std::vector<int32_t> cid;
    int64_t cid0 = 0, ncid = 0;  // first compact id of the slab and its in-domain cell count
    std::vector<double> hbuf;    // host bounding-box staging for that gather / scatter
    // NSGPU_RCCL_LOOPBACK=1 (test / measurement hook): a 1-rank RCCL communicator whose every
    // peer is this process.  One rank: every exchange point of the step runs its RCCL group with
    // peer == self (both ghost sides from this slab's own edge rows) and every reduction an
    // ncclAllReduce -- the multi-rank call sites on one GPU; ghost rows beyond the walls carry
    // zero weight, so the step is the plain single-rank step.  nranks > 1 with neither an
    // ncclUniqueId nor a host transport: a VIRTUAL slab -- rank `rank`'s slab, hierarchy,
    // launches and RCCL groups (exchanges, the agglomeration gather) with self as every peer,
    // reductions over this slab only: the per-rank time of a multi-GPU step without the other
    // GPUs (tools/slab_projection.py).
    int loopback = 0;
    // virtual slab only (NSGPU_VIRTUAL_ITERS="h:c,h:c,..."): the slab's own residuals are not the
    // global solve's, so each step replays the global run's Helmholtz sweeps h and V-cycles c
    // (cycled over the list), with one residual check (host sync) per solve like a predicted one
    std::vector<std::pair<int, int>> replay;
    size_t replay_k = 0;
    int rp_h = 0, rp_c = -1;        // this step's replayed counts (0 / -1: converge normally)
    int n_xchg = 0, n_allred = 0;   // exchange groups / all-reduces issued in the current step
    double x_link = 0.0;            // bytes over this rank's busiest peer link in the current step
    // speculative CorrectVelocities: inside a time step, the multigrid's residual check that
    // the cycle history predicts to pass enqueues K5 (into the ping-pong partners, with its
    // min/max) BEFORE the host waits for the residual, so the GPU works through the host round
    // trip; k5_spec = 1 after a passing check (the step then only swaps), 0 otherwise (K5 runs
    // again after the last cycle: u* is untouched, K5 writes TMPU / TMPV)
    int in_step = 0, k5_spec = 0, n_spec = 0, n_spec_hit = 0;
    // (k.speculate = 0: no speculative K5 / K3, the equivalence test's reference)
    // r4: K5 may form the next step's Poisson guess (k_cell_s<6>, k.k5_guess; default: k_axpby
    // at the next step as in round 3); guess_ready: TMP holds it (branch guess_branch of extrap_plan) -- any entry
    // point that may write TMP or the phi planes clears it.  K3 then runs speculatively behind the
    // Helmholtz residual check (k3_spec: rhs_phi is this step's), which the extrapolation used to fill
    // Measured (r4, 4096^2 driver form): k_cell_s<6> 242 us against K5 128 + k_axpby 104 us -- no gain
    // (9,819-9,822 vs 9,821-9,863 MLUPS), so it is opt-in
    int guess_ready = 0, guess_branch = 0, k3_spec = 0;
    int cur_cycles = -1;         // V-cycles of the Poisson solve in progress (at its K5)
    int last_cycles = -1;        // V-cycles of the last multigrid solve (-1: none / Krylov)
    // r4: the direct Poisson solve (ns_fps.hip) of a rectangle with zero-flux phi sides and uniform hy
    // (ny a power of two): DCT along y, tridiagonal recurrences along x, inverse DCT -- no iteration,
    // so no initial guess (no phi history planes).  Its output residual (a separate pass: 76 us at
    // 4096^2) is checked on the first solve of a run and every k.fps_check-th after it (default 16;
    // 1 = every solve; a standalone ns_kernel solve always); the check's host sync hides
    // behind a speculative K5, and a residual above rtol continues with multigrid V-cycles from this
    // phi.  The solve is a fixed arithmetic sequence: its residual does not drift between checks
    // (1e-13 .. 1e-12 of ||b|| at 4096^2).  NSGPU_FPS=0: multigrid
    bool fps = false;
    bool fps_pc = false;         // masked domain: the bounding box's direct solve preconditions BiCGStab (NSGPU_FPS_PC=0: V-cycle)
    // (r5) and, with at most NSGPU_CAP_MAX (4096) interface faces, the exact solve by the capacitance matrix
    // (cap_setup / cap_solve; NSGPU_CAP=0: BiCGStab preconditioned by the box's solve, A/B)
    nsg::CapArgs cap{};
    void* cap_mem = nullptr;
    nsg::FpsArgs fa{};
    // what the direct solve reads on the device beside fa (fps_setup; mem: its arena's ONE block, fa's arrays included)
    struct FpsDev {
        double* mem = nullptr;
        const double *tw = nullptr, *wk = nullptr, *tw8 = nullptr;   // (r5) tw8, ny = 16384: the 8192-point halves' twiddles
        // multi-rank: this rank's aggregate of a recurrence (2 x ld), every rank's (nranks x 2 x ld, one
        // allgather per direction and solve) and the carry-in folded from them (ld)
        double *ragg = nullptr, *gath = nullptr;
        size_t n = 0;              // (r5) the allgather's slot: 2 x ld aggregates + (sum b, sum b^2) + padding
        // (r5) ONE allgather per solve (NSGPU_FPS_ONEGATHER=0: two, A/B): the slot also carries the rank's backward
        // aggregate with a zero forward carry-in (2 more ld), which is affine in that carry-in (FpsRank::bq); og_b /
        // og_x1: the host tables B_p (every rank, per mode) and X1_p
        bool og = false;
        const double *og_b = nullptr, *og_x1 = nullptr;
        // the deferred mean's tables of mode 0 (below): every chunk's E / BXl, the groups', the ranks' of the constant 1
        const double *m0e = nullptr, *m0b = nullptr, *m0g = nullptr, *m0a = nullptr;
        double *dense_mem = nullptr, *dF = nullptr, *dG = nullptr;   // the dense transforms (fps_dense): F | G
    } fpd;
    int fps_passes = 2;          // full passes of the tridiagonal recurrences (NSGPU_FPS_PASSES=3: t1 / t2 / t3)
    long fps_solves = 0;
    bool fps_og_mean = false;
    // r5, multi-rank rectangles on the direct solve: the fused K3's sums are not all-reduced -- they ride
    // on the recurrences' forward allgather (at 2 ld of each rank's slot), and the mean comes off mode 0
    // afterwards, as the linear response of its aggregates to the constant ny * mean (fpd.m0*).
    // NSGPU_FPS_DEFER=0: the all-reduce before the solve (A/B).  mean_pend: this step's sums wait there
    bool fps_defer = false, mean_pend = false;
    double fps_res = -1.0;       // the last checked solve's relative residual
    int kpred[3] = {1, 1, 1};    // (r5) the last BiCGStab solve's iterations: Poisson, Helmholtz u, v (bicgstab's batch)
    // (r5) a masked domain's Helmholtz solve on one rank by red-black SOR (k.mask_rb; k.mask_mt: up to 4 sweeps per
    // launch + the residual in the last; k.mask_band wall-band sweeps first): the sweeps the last step needed (the
    // next step's first batch)
    int mask_helm_next = 4, mask_helm_ok = 0;
    // r5, multi-rank rectangles: the Helmholtz check's collective is an allgather of every rank's
    // S_HBNL .. S_MML (bus()): K1's norms and the previous step's K5 min / max ride on it, so neither
    // takes a collective of its own (NSGPU_BUS=0: the per-reduction all-reduces, A/B); bus_mem holds
    // the P gathered slots of BUS_NV values
    bool bus = false;
    double* bus_mem = nullptr;
    // r5, multi-rank rectangles on the direct solve: DEEP ghost rows.  K1 computes its rows and deep_e =
    // 8 + 6 R rows of each neighbour's slab (R: the wall bands' 3-sweep launches), its exchange carrying u,
    // v, phi that deep; the band launches then compute 6 rows fewer each and need no exchange, and the
    // residual 3-sweep pass finds its 7-row cone valid and computes one neighbour row more, which K3 reads --
    // one exchange group (K1's) where r4 had 1 + R + 1 + 1 (deep_geo; NSGPU_DEEP=0: the r4 exchanges, A/B).  hp: the finest planes' ghost rows per side
    // (HALO, or deep_e + HALO + 2); cu_ext / u_ext: ghost rows of cu, cv / of u, v (the Helmholtz
    // iterates) known valid now
    int hp = nsg::HALO;
    bool deep = false;
    int deep_e = 0, cu_ext = 0, u_ext = 0;
    int phi_ext = 0;             // (r5) phi's ghost row valid from the direct solve (deep slabs, k_fps_t2b's ghost rows)
    bool fps_strict = false;     // a check failed or came within 1/100 of rtol: check every solve
    bool hbn_pend = false;       // slabs: K1's ||RHS||^2 partial sums await the Helmholtz check's all-reduce
    // K3 fused into the direct solve's DCT (r4, launch_fps_div; NSGPU_FPS_FUSE=0: K3 + the DCT): inside
    // steps the divergence goes straight into the transformed plane, rhs_phi is stored only for a checked
    // solve; fps_pre: the plane holds this step's coefficients (pois_solve_fps skips its DCT)
    bool fps_fuse = true, fps_pre = false, fps_pre_b = false;
    // (r6) the deferred correction: an ns_step_async step ends after its Poisson solve (U, V = u*, v*, PHI = phi^n)
    // and the next step's K1 applies CorrectVelocities on the fly (k_rhs_sc: K5 folded into K1 -- one HBM pass
    // of 40 B/cell less); any other entry point that reads or writes the fields runs K5 first (materialize)
    bool k5_defer_ok = false;    // one rank, rectangle, no NEUMANN side, the direct solve, hy uniform, streaming K1
    int corr_pend = 0, defer_now = 0, corr_k1 = 0;   // corr_k1: this step's K1 applied a deferred correction
    // a rectangle's edge on each side (W, E, S, N) and the grid's edge count: ns_scalar_enable's bc[k] is per edge
    int side_edge[4] = {-1, -1, -1, -1}, n_edges = 0;
    double inv_h2 = 0.0;         // 1 / min(hx)^2 + 1 / min(hy)^2 (the Helmholtz SOR weights)
    // the passive scalar (ns_scalar_enable; DESIGN.md 4 "Passive scalar"): nothing below exists without one.
    // Planes laid out like the fields: T, its sweep partner, rT, cT0; its ghosts per side (q_g = neu ? q : -q + c);
    // ct: the coefficient tables with the scalar's Dirichlet sides in bx / by (the sweeps' operator I - dt/(2 pe)
    // L_T); partials, device slots and their pinned mirror of its own, so that a step's other reductions see
    // exactly what they see without a scalar
    struct Scalar {
        enum { BN2 = 0, RES2, TMIN, NTMAX, AUX, NSLOT = 8 };   // device slots
        bool on = false;
        double pe = 0.0, omega = 1.0;
        int neu[4] = {0, 0, 0, 0};
        double c[4] = {0, 0, 0, 0};
        nss::dev_ptr<double> mem, bxy, part, scal;
        nss::pinned_ptr<double> hs;
        double *T = nullptr, *TT = nullptr, *R = nullptr, *C = nullptr;   // (in mem)
        nsg::Coef ct{};
        hipEvent_t ev = nullptr;   // (scalar_free destroys it)
        // the step's first batch of sweeps is what the previous step needed; it is enqueued, with its residual and
        // the min / max of its result, before the velocities' Helmholtz solve, whose residual check brings them
        int next = 4, ok_steps = 0, sweeps = 0;
        ns_scalar_stats last{};
        // Boussinesq buoyancy (ns_scalar_buoyancy): f = (bx, by) (T - tref), applied by k_rhs_t's buoyant variant
        double bx = 0.0, by = 0.0, tref = 0.0;
        bool buoyant() const { return on && (bx != 0.0 || by != 0.0); }
    } sc;
    // derived fields (ns_derive; DESIGN.md 4 "Derived fields"): nothing below exists before the first call.  The
    // planes (nxl x ld, no ghost rows) and psi's vertex plane ((nx + 1) rows of ldv) each on first request; partials,
    // result slots and their pinned mirror of its own, so that no slot a later step reads is touched
    struct Derived {
        enum { NSLOT = 16 };   // 3 sums, 4 + 2 minima, psi's (min, -max)
        nss::dev_ptr<double> p, w, d, psi, base, part, ppart, scal;
        nss::pinned_ptr<double> hs;
        int ncap = 0, ldv = 0;
    } dv;
    // tracer particles (ns_tracers_enable; DESIGN.md 4 "Tracers"): nothing below exists without them.  SoA planes of
    // `cap` particles (x, y, wu, wv, age, then the int32 state words), the face tables xf | yf with their host copies
    // (the seed check), partials, four count slots (live, exited, stuck, -max age) and their pinned mirror of its
    // own; su / sv (ns_tracers_sample's output) on first use
    struct Tracers {
        enum { NSLOT = 4 };
        bool on = false;
        int64_t cap = 0, n = 0;
        nss::dev_ptr<double> mem, smp, tab, part, scal;
        nss::pinned_ptr<double> hs;
        std::vector<double> xf, yf;
        nsg::TracerArgs a{};
    } tr;
    // running flow statistics (ns_avg_enable; DESIGN.md 4 "Flow statistics"): nothing below exists without them.
    // mem: the means and co-moment sums accumulated (nxl x ld each, no ghost rows; plane[which], null: not kept) and,
    // with NS_AVG_PRESSURE, the sample's own pressure plane P behind them; ppart: the derived pass's partials, of
    // its own, so that no slot a step or ns_derive reads is touched.  n, steps: host counters
    struct Averages {
        bool on = false;
        int every = 1, flags = 0, nsrc = 2;
        int64_t n = 0, steps = 0;
        size_t nplanes = 0;
        nss::dev_ptr<double> mem, ppart;
        double* P = nullptr;                  // (in mem)
        double* plane[NS_AVG_NUM] = {};
        nsg::MomArgs a{};
        ns_avg_stats acc{};      // the drained sample intervals nobody has asked for yet
    } av;
    // wall loads (ns_loads_enable; DESIGN.md 4 "Wall loads"): nothing below exists without them.  list: the host's
    // boundary-face list (its s and ds tables are handed out from here); tab: its device copy (faces | chunks | chunk
    // offsets); val: the faces' six values; part: the chunks' partials; ring: capacity + 1 records of nrec doubles, the
    // last one ns_loads_edges' own.  The ring's counters and step numbers live on the host: slot = sample % capacity
    struct Loads {
        bool on = false;
        int every = 1, capacity = 0, nrec = 0;
        int64_t total = 0, steps = 0;
        nsg::LoadList list;
        nss::dev_ptr<int32_t> tab;
        nss::dev_ptr<double> val, part, ring;
        std::vector<int64_t> rstep;
        nsg::LoadArgs a{};
        ns_load_stats acc{};     // the drained sample intervals nobody has asked for yet
    } lo;
};

namespace nss {

// `bytes` at *ptr, zeroed on s->st if `zero`; the error text and code otherwise
template <class T>
int dev_alloc(ns_solver* s, T** ptr, size_t bytes, bool zero, const char* what) {
    if (hipMalloc(ptr, bytes) != hipSuccess) { set_err("hipMalloc of %zu bytes (%s) failed", bytes, what); return NS_ENOMEM; }
    if (zero && hipMemsetAsync(*ptr, 0, bytes, s->st) != hipSuccess) { set_err("memset (%s) failed", what); return NS_EHIP; }
    return 0;
}
// ... filled from the host vector v
template <class T>
int dev_upload(ns_solver* s, T** ptr, const std::vector<T>& v, const char* what) {
    CHK(dev_alloc(s, ptr, v.size() * sizeof(T), false, what));
    if (hipMemcpy(*ptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { set_err("%s upload failed", what); return NS_EHIP; }
    return 0;
}
// ... into an owner (which holds the block even where the call fails after allocating it)
template <class T>
int dev_alloc(ns_solver* s, dev_ptr<T>& p, size_t bytes, bool zero, const char* what) {
    T* raw = nullptr;
    const int rc = dev_alloc(s, &raw, bytes, zero, what);
    p.reset(raw);
    return rc;
}
template <class T>
int dev_upload(ns_solver* s, dev_ptr<T>& p, const std::vector<T>& v, const char* what) {
    T* raw = nullptr;
    const int rc = dev_upload(s, &raw, v, what);
    p.reset(raw);
    return rc;
}
inline int pinned_alloc(pinned_ptr<double>& p, size_t n) {
    double* raw = nullptr;
    if (hipHostMalloc(&raw, n * sizeof(double), hipHostMallocDefault) != hipSuccess) { set_err("hipHostMalloc failed"); return NS_ENOMEM; }
    p.reset(raw);
    return 0;
}

// the entry prologue of an observer's (or the scalar's) call `who`: the solver exists and `on` holds -- else "who:
// what (call)", e.g. "ns_avg_get: flow statistics are not enabled (ns_avg_enable)" -- then prepare(flags)
enum { SETTLE = 1, LAUNCH = 2 };
int enter(ns_solver* s, const char* who, bool on = true, const char* what = "", const char* call = "", int flags = 0);
// SETTLE: a deferred correction is applied first (materialize: the call reads or writes the fields); LAUNCH: the
// call launches kernels (the device, the compute stream's CU mask).  On its own where arguments are checked in between
int prepare(ns_solver* s, int flags);
int materialize(ns_solver* s);
// the spacings as the device holds them (s->c.hx, s->c.hy), on the host
int host_spacings(ns_solver* s, std::vector<double>& hx, std::vector<double>& hy);

// the observers' step side (ns_observe.cpp): what step_body_ calls behind K1, and their memory's release
int avg_sample(ns_solver* s);
int loads_sample(ns_solver* s, int64_t step);
int tracer_advance(ns_solver* s, double dt, bool count);
void observers_free(ns_solver* s);

}  // namespace nss
