// ns_cell.h -- what a kernel sees of one cell, shared by the translation units that hold kernels (ns_kernels.hip,
// ns_loads.hip): the velocity ghost, the cell topologies (TopoRect / TopoInner / TopoMask) and the derived fields' cell
// pass (dv_* helpers, derived_cell).  Device code only; every function is inlined into its caller.  Not installed.
#pragma once
#include "ns_internal.h"

namespace nsg {

__device__ __forceinline__ double ldf(const double* f, int ld, int li, int j) {
    return f[(ptrdiff_t)li * ld + j];
}

// velocity ghost, EvaluateGhostStencil_V (FluidSolver.cpp:166-173):
//   walls / inlets: weights {-1} + constant[d];  NEUMANN: weights {1}
// k: the face's index along its side (column j on W / E, global row i on S / N), where an edge profile is read
// (edge_const; PROF false: the side's own constant, no table test -- the unprofiled instantiations of the kernels
// that evaluate a ghost for every cell)
template <bool PROF = true>
__device__ __forceinline__ double ghost_v(const Geo& g, double q, int side, int d, int k) {
    const double cc = PROF ? edge_const(g.c0[side], g.c1[side], g.pt[side], g.pd[side], d, k, side < 2 ? g.ny : g.nx)
                           : (d == 0 ? g.c0[side] : g.c1[side]);
    return g.neu[side] ? q : (-q + cc);
}

// ------------------------------------------------ cell topology: rectangle or masked polygon
// The reference's existence tests (Grid::inDomain, Cell::edges[k] == -1) and ghost stencils
// (EvaluateGhostStencil_V/_P, FluidSolver.cpp:166-181) seen from cell (li, j):
//   in(di, dj)          the cell at that offset is in the domain;
//   gv(di, dj, k, q, d) the velocity ghost across face k of the cell at (di, dj), value q;
//   edge(k)             the edge on face k of this cell (ApplyBoundaryConditions).
// TopoRect folds to bound checks on the compile-time offsets and per-side constants (the
// rectangle kernels compile to what they were); TopoMask reads the int32 topology plane
// (FC_*) and the edge table of a non-rectangular domain.
// PROF false: the sides' own constants only, no edge-profile test (K1's ring in the kernels a solver without profiles
// launches: the code they had before profiles existed)
template <bool PROF>
struct TopoRectT {
    const Geo& g;
    int gi, j;
    __device__ __forceinline__ TopoRectT(const Geo& g_, int li, int j_) : g(g_), gi(g_.i0 + li), j(j_) {}
    __device__ __forceinline__ bool cell() const { return true; }
    __device__ __forceinline__ bool in(int di, int dj) const {
        if (dj == 0) return di < 0 ? gi + di >= 0 : gi + di < g.nx;
        if (di == 0) return dj < 0 ? j + dj >= 0 : j + dj < g.ny;
        return gi + di >= 0 && gi + di < g.nx && j + dj >= 0 && j + dj < g.ny;
    }
    __device__ __forceinline__ double gv(int di, int dj, int k, double q, int d) const {
        return ghost_v<PROF>(g, q, k, d, k < 2 ? j + dj : gi + di);
    }
    // (the constants resolved at this cell's own face: rhs_bc's wall terms)
    __device__ __forceinline__ EdgeDev edge(int k) const {
        if (!PROF) return EdgeDev{g.neu[k], g.enx[k], g.eny[k], g.c0[k], g.c1[k]};
        const int f = k < 2 ? j : gi, n = k < 2 ? g.ny : g.nx;
        return EdgeDev{g.neu[k], g.enx[k], g.eny[k], edge_const(g.c0[k], g.c1[k], g.pt[k], g.pd[k], 0, f, n),
                       edge_const(g.c0[k], g.c1[k], g.pt[k], g.pd[k], 1, f, n)};
    }
};
using TopoRect = TopoRectT<true>;
// a cell at least two cells from every wall (the MUSCL stencil's reach): every neighbour exists,
// no ghost is evaluated -- K1's interior tiles (k_rhs_lds) skip the existence selects
struct TopoInner {
    __device__ __forceinline__ TopoInner(const Geo&, int, int) {}
    __device__ __forceinline__ bool cell() const { return true; }
    __device__ __forceinline__ bool in(int, int) const { return true; }
    __device__ __forceinline__ double gv(int, int, int, double q, int) const { return q; }
    __device__ __forceinline__ EdgeDev edge(int) const { return EdgeDev{}; }   // (never reached)
};
struct TopoMask {
    const Geo& g;
    int li, j, code;
    __device__ __forceinline__ int at(int di, int dj) const {
        const int jj = j + dj;
        return (jj >= 0 && jj < g.ny) ? g.fc[(ptrdiff_t)(li + di) * g.ld + jj] : 0;
    }
    __device__ __forceinline__ TopoMask(const Geo& g_, int li_, int j_) : g(g_), li(li_), j(j_), code(0) { code = at(0, 0); }
    __device__ __forceinline__ bool cell() const { return (code & FC_IN) != 0; }
    __device__ __forceinline__ bool in(int di, int dj) const {
        // (r5) a face neighbour from the cell's own code (its face is FC_INT exactly when the neighbour is in the
        // domain: ns_create checks Grid::inDomain against Cell::edges) -- no load of the neighbour's code
        if (di * di + dj * dj == 1) return fc_edge(code, di < 0 ? 0 : di > 0 ? 1 : dj < 0 ? 2 : 3) == FC_INT;
        return (at(di, dj) & FC_IN) != 0;
    }
    __device__ __forceinline__ double gv(int di, int dj, int k, double q, int d) const {
        const EdgeDev& E = g.et[fc_edge(di == 0 && dj == 0 ? code : at(di, dj), k)];
        return E.neu ? q : (-q + edge_const(E.c0, E.c1, E.pt, E.pd, d, k < 2 ? j + dj : g.i0 + li + di, k < 2 ? g.ny : g.nx));
    }
    __device__ __forceinline__ EdgeDev edge(int k) const {
        const EdgeDev& E = g.et[fc_edge(code, k)];
        const int f = k < 2 ? j : g.i0 + li, n = k < 2 ? g.ny : g.nx;
        return EdgeDev{E.neu, E.enx, E.eny, edge_const(E.c0, E.c1, E.pt, E.pd, 0, f, n),
                       edge_const(E.c0, E.c1, E.pt, E.pd, 1, f, n)};
    }
};

// ------------------------------------------------ derived fields (ns_derive; DESIGN.md 4, "Derived fields")
// Pressure P = phi - alpha L phi (ExportData; L: k_apply<0, Topo>'s rows), vorticity and the divergence the
// approximate projection leaves, all from Div_V's face values (face_val: r-weighted toward a neighbour in the
// domain, 0.5 (q + ghost) with the edge's velocity ghost on a boundary face), and the domain integrals a run is
// watched by.  The products and sums a compiler may contract live in the dv_* helpers with contraction off, and
// every form -- the strips and the thread-per-cell kernel -- goes through them: they agree bit for bit.
__device__ __forceinline__ double dv_face(double q, double qn, double r) {
#pragma clang fp contract(off)
    return qn * r + q * (1 - r);
}
__device__ __forceinline__ double dv_wall(double q, double ghost) {
#pragma clang fp contract(off)
    return 0.5 * (q + ghost);
}
// 1 / h: once per row and per column (dv_rcp), not a division per difference -- the strips are bound by their
// arithmetic, not by HBM, with four fp64 divisions per cell
__device__ __forceinline__ double dv_rcp(double h) {
#pragma clang fp contract(off)
    return 1.0 / h;
}
// (a1 - a0) rhx + sg (b1 - b0) rhy: the divergence (sg = 1) and the vorticity (sg = -1)
__device__ __forceinline__ double dv_diff(double a1, double a0, double rhx, double b1, double b0, double rhy, double sg) {
#pragma clang fp contract(off)
    return (a1 - a0) * rhx + sg * ((b1 - b0) * rhy);
}
__device__ __forceinline__ double dv_lap_nb(double s, double w, double xn, double xc) {
#pragma clang fp contract(off)
    return s + w * (xn - xc);
}
// a NEUMANN face: (ghost - x_c) w2, w2 = (1 / h)^2 (dv_rsq of dv_rcp), with the ghost 2.5 x_c - 2 x_1 + 0.5 x_2 (x_1, x_2 inward)
__device__ __forceinline__ double dv_rsq(double rh) {
#pragma clang fp contract(off)
    return rh * rh;
}
__device__ __forceinline__ double dv_lap_neu(double s, double w2, double xc, double x1, double x2) {
#pragma clang fp contract(off)
    const double gh = 2.5 * xc - 2.0 * x1 + 0.5 * x2;
    return s + (gh - xc) * w2;
}
__device__ __forceinline__ double dv_press(double pc, double alpha, double s) {
#pragma clang fp contract(off)
    return pc - alpha * s;
}
__device__ __forceinline__ double dv_mul(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
// NaN-propagating min (a blown-up field is visible in the stats, as K5's monitor)
__device__ __forceinline__ double dv_min(double a, double x) { return fmin(a, x != x ? -INFINITY : x); }

// one cell's P, vorticity, divergence: U / V / P(di, dj) give u, v, phi at that offset (global loads, or a strip's
// register windows and lane neighbours; P also at +-2 along the normal of a NEUMANN face)
// X(t) / Y(t): table t of the cell's row / column -- 0: h, 1 / 2: the face weight toward the lower / upper neighbour
// (Coef::fwx / fex, fsy / fny), 3 / 4: the Poisson weight toward it (pw / pe, ps / pn), 5: dv_rcp(h) -- global tables
// or a strip's registers
// SEL (the strips: every accessor a register, every ghost arithmetic): both sides of each face are evaluated and
// selected, no branch; otherwise a neighbour or a ghost is read only where the face has one
template <class T, bool SEL, class FU, class FV, class FP, class FX, class FY>
__device__ __forceinline__ void derived_cell(const Geo& g, double alpha, FU&& U, FV&& V, FP&& P, FX&& X, FY&& Y, int li,
                                             int j, double& p_, double& w_, double& d_) {
    const T t(g, li, j);
    const bool hW = t.in(-1, 0), hE = t.in(1, 0), hS = t.in(0, -1), hN = t.in(0, 1);
    const double fw = X(1), fe = X(2), fs = Y(1), fn = Y(2);
    const double uc = U(0, 0), vc = V(0, 0), pc = P(0, 0);
    // the value of component d (q at the cell, Q its accessor) on face k (toward (di, dj), weight r)
    auto face = [&](bool has, double q, auto& Q, int di, int dj, double r, int k, int d) {
        if (SEL) {
            const double a = dv_face(q, Q(di, dj), r), b = dv_wall(q, t.gv(0, 0, k, q, d));
            return has ? a : b;
        }
        return has ? dv_face(q, Q(di, dj), r) : dv_wall(q, t.gv(0, 0, k, q, d));
    };
    // x-faces: u for the divergence (component 0's ghost), v for the vorticity (component 1's); y-faces likewise
    const double uW = face(hW, uc, U, -1, 0, fw, 0, 0), uE = face(hE, uc, U, 1, 0, fe, 1, 0);
    const double vW = face(hW, vc, V, -1, 0, fw, 0, 1), vE = face(hE, vc, V, 1, 0, fe, 1, 1);
    const double uS = face(hS, uc, U, 0, -1, fs, 2, 0), uN = face(hN, uc, U, 0, 1, fn, 3, 0);
    const double vS = face(hS, vc, V, 0, -1, fs, 2, 1), vN = face(hN, vc, V, 0, 1, fn, 3, 1);
    const double rhx = X(5), rhy = Y(5);
    d_ = dv_diff(uE, uW, rhx, vN, vS, rhy, 1.0);
    w_ = dv_diff(vE, vW, rhx, uN, uS, rhy, -1.0);
    // k_apply<0, Topo>'s sum in its order (W, E, S, N): toward (di, dj) with the weight pw, or across a boundary face
    // -- 0 on a wall / inlet, the extrapolated ghost's term on a NEUMANN one (x_1, x_2 inward)
    auto lap = [&](double s, bool has, int di, int dj, double pw, double rh, int k) {
        if (SEL) {
            const double a = dv_lap_nb(s, pw, P(di, dj), pc), b = dv_lap_neu(s, dv_rsq(rh), pc, P(-di, -dj), P(-2 * di, -2 * dj));
            return has ? a : t.edge(k).neu ? b : s;
        }
        if (has) return dv_lap_nb(s, pw, P(di, dj), pc);
        return t.edge(k).neu ? dv_lap_neu(s, dv_rsq(rh), pc, P(-di, -dj), P(-2 * di, -2 * dj)) : s;
    };
    double s = 0.0;
    s = lap(s, hW, -1, 0, X(3), rhx, 0);
    s = lap(s, hE, 1, 0, X(4), rhx, 1);
    s = lap(s, hS, 0, -1, Y(3), rhy, 2);
    s = lap(s, hN, 0, 1, Y(4), rhy, 3);
    p_ = dv_press(pc, alpha, s);
}
}  // namespace nsg
