// ns_fps_tables.h -- the host tables of the direct Poisson solve (ns_fps.hip) from a plain description of the operator.
// Host-only: no HIP include (tests/fps_tables_host_test.cpp builds every table without a GPU).
//
// The pivots p_i(k) of Thomas' recurrence along x depend on the operator only: the host runs it over the global rows
// and keeps what the kernels read (FpsArgs, ns_internal.h: what each table means).  Every table goes through
// fps_piv_next, the ONE host restatement of the device's piv_next: the block fixed points (prowb) and the FIXED chunks
// (cfix) are exact only while host and device pivots are the same bits.  One function per family, in the order to call.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

namespace nsg {

struct FpsOp {
    int nx = 0, ny = 0, ld = 0, i0 = 0, nxl = 0;   // global rows, modes, plane row stride; this slab's rows [i0, i0 + nxl)
    int M = 16, G = 4, outE = 0, pmode = 0;        // FPS_M, FPS_G; a NEUMANN outflow E side; pivot shortcut: 0, 1 ptab, 2 prowb
    std::vector<std::pair<int, int>> ranks;        // every rank's rows [q0, q1), in order (one entry: one rank)
    const double *pw = nullptr, *pe = nullptr;     // x coefficients by global row (nx each)
    double hy0 = 0.0;              // the uniform hy (the FFT's eigenvalues; the dense transforms bring their own mu)
    bool t8 = false;               // the half-size twiddles too (ny = 16384)
    int nch() const { return (nxl + M - 1) / M; }
    int ngrp() const { return (nch() + G - 1) / G; }
    int nchp() const { return ngrp() * G; }   // (the kernels address whole groups' chunks)
};
constexpr int FPS_NEVER = 1 << 30;

struct FpsTables {
    std::vector<double> tw, wk, mu, tw8;   // e^{-2 pi i m / ny}, e^{-i pi m / 2 ny} (interleaved), Ly's eigenvalues
    // rp0 (nchp x ld) | bt (2 x nchp x ld: beta at chunk c, BR at nch + c) in ONE allocation (as two they
    // kept the C library's trim threshold below the heap's top, and every ns_create at 4096^2 paid 40 ms of page faults)
    std::vector<double> ct;
    const double* rp0() const { return ct.data(); } const double* bt() const { return ct.data() + ct.size() / 3; }
    std::vector<double> ptab, pinf;        // pmode 1: prow x ld and ld; pmode 2: pinf only (empty: no shortcut)
    std::vector<int> prowb;                // pmode 2: every 128-mode block's fixed-point row (FPS_NEVER: none)
    std::vector<int> cfix;                 // FIXED chunks: every block's first (FPS_NEVER: none); empty: none at all
    int prow = 0, kfast = FPS_NEVER, clast = -1;
    std::vector<double> r0, m0e, m0b, m0g, m0a;   // slabs, mode 0: 1 / p (nx); of the constant 1: nchp, nchp, ngrp, ranks
    std::vector<double> ogb, ogx1;                // slabs, one allgather per solve: B_p (ranks x ld), X1_p (ranks)
};

// one row of the pivot recurrence, ns_fps.hip's piv_next: the same operands, the same explicit fma, the eliminated
// outflow row (-mu / 2, mu) and mode 0's pinned row, both global row nx - 1.  last: w is that row (w.last, or plainly false
// where a caller's rows end before it).  w: row gi's pw, -(pw + pe), pe_{gi-1}, an outflow side; returns 1 / p_gi, g = g_gi
struct FpsRow { double pw, d, pem; bool oe, last; };
inline FpsRow fps_row(const FpsOp& o, int gi) {
    return {o.pw[gi], -(o.pw[gi] + o.pe[gi]), gi > 0 ? o.pe[gi - 1] : 0.0, o.outE != 0, gi == o.nx - 1};
}
inline double fps_piv_next(const FpsRow& w, bool last, int k, double mu, double rprev, double& g) {
    const bool oe = last && w.oe;
    g = (oe ? -0.5 * mu : w.pw) * rprev;
    const double p = std::fma(-g, w.pem, oe ? mu : w.d + mu);
    return (last && k == 0) ? 0.0 : 1.0 / p;
}

// twiddles, half-twiddles and the eigenvalues -(2 / hy^2)(1 - cos(pi m / ny)) of the uniform Ly
inline void fps_twiddles(const FpsOp& o, FpsTables& T) {
    const int N = o.ny;
    const double pi = 3.14159265358979323846;
    T.tw.assign(2 * (size_t)N, 0.0); T.wk = T.tw;
    T.mu.assign(N, 0.0);
    for (int m = 0; m < N; m++) {
        const double t = 2.0 * pi * ((double)m / N), u = pi * ((double)m / (2.0 * N)), sn = std::sin(u);
        T.tw[2 * m] = std::cos(t); T.tw[2 * m + 1] = -std::sin(t);
        T.wk[2 * m] = std::cos(u); T.wk[2 * m + 1] = -sn;
        T.mu[m] = -4.0 / (o.hy0 * o.hy0) * sn * sn;
    }
    if (o.t8) T.tw8.assign(N, 0.0);   // e^{-2 pi i m / (ny / 2)}: the full table's even entries
    for (int m = 0; o.t8 && m < N / 2 * 2; m++) T.tw8[m] = T.tw[4 * (m / 2) + m % 2];
}

// rp0: 1 / p of the row before each chunk of this slab (0 before global row 0); per chunk beta (over pi) and BR
inline void fps_chunk_tables(const FpsOp& o, FpsTables& T) {
    const int N = o.ny, ld = o.ld, M = o.M, nch = o.nch(), iend = o.i0 + o.nxl;
    T.ct.assign(3 * (size_t)o.nchp() * ld, 0.0); double *rp0 = T.ct.data(), *bt = rp0 + T.ct.size() / 3;
    std::vector<double> r(N, 0.0), crp((size_t)M * N), cpi((size_t)M * N);   // 1 / p of the last row; the chunk's 1/p, pi
    for (int gi = 0; gi < iend; gi++) {
        const int li = gi - o.i0, t = li >= 0 ? li % M : 0;
        if (li >= 0 && t == 0) std::copy(r.begin(), r.end(), rp0 + (size_t)(li / M) * ld);
        const FpsRow w = fps_row(o, gi);
        for (int k = 0; k < N; k++) {
            double gg;
            r[k] = fps_piv_next(w, w.last, k, T.mu[k], r[k], gg);
            if (li >= 0) {
                crp[(size_t)t * N + k] = r[k];
                cpi[(size_t)t * N + k] = -gg * (t ? cpi[(size_t)(t - 1) * N + k] : 1.0);
            }
        }
        if (li < 0 || (t != M - 1 && gi != iend - 1)) continue;
        for (int k = 0; k < N; k++) {   // the chunk's (beta, BR)
            double b = 0.0, R = 1.0;
            for (int u = t; u >= 0; u--) {
                const double rr = crp[(size_t)u * N + k], q = -o.pe[gi - t + u] * rr;
                b = cpi[(size_t)u * N + k] * rr + q * b;
                R = q * R;
            }
            bt[(size_t)(li / M) * ld + k] = b; bt[(size_t)(nch + li / M) * ld + k] = R;
        }
    }
}

// the pivot shortcut of t1b / t2b (piv_pair): every mode's recurrence from global row 0 over uniform interior rows
// reaches its fixed point after c_k rows -- many for the low modes, few for the high ones.  pmode 2: per 128-mode block
// the row from which all its modes return the same bits (prowb: the skipped divisions change nothing); pmode 1 (A/B):
// the modes k >= kfast, whose c_k (to 4 ulp) are all below prow, read 1 / p from ptab there and pinf after it
inline void fps_pivot_shortcut(const FpsOp& o, FpsTables& T) {
    const int N = o.ny, ld = o.ld, mode = o.pmode, PRMAX = std::min(o.nx - 1, mode == 1 ? 1024 : 4096);
    if (mode == 0 || N <= 128 || PRMAX <= 64) return;
    std::vector<double> rr(N, 0.0);
    std::vector<int> conv(N, -1);
    std::vector<char> left(N, 0);
    if (mode == 1) T.ptab.assign((size_t)PRMAX * ld, 0.0);
    for (int gi = 0; gi < PRMAX; gi++) {
        const FpsRow w = fps_row(o, gi);
        for (int k = 0; k < N; k++) {
            double gg;
            const double rn = fps_piv_next(w, false, k, T.mu[k], rr[k], gg);   // (gi < PRMAX <= nx - 1: never row nx - 1)
            const bool fixed = mode == 2 ? rn == rr[k] : std::fabs(rn - rr[k]) <= 4 * 2.220446049250313e-16 * std::fabs(rn);
            if (conv[k] < 0 && !left[k] && gi > 1 && fixed) conv[k] = gi;
            if (mode == 2 && conv[k] >= 0 && rn != rr[k]) { conv[k] = -1; left[k] = 1; }   // (an oscillation: never fast)
            rr[k] = rn;
            if (mode == 1) T.ptab[(size_t)gi * ld + k] = rn;
        }
    }
    // the row after the last of modes [k0, k1) to converge; FPS_NEVER if one did not within PRMAX rows
    auto row = [&](int k0, int k1) {
        int mx = 0;
        for (int k = k0; k < k1; k++) {
            if (conv[k] < 0) return FPS_NEVER;
            mx = std::max(mx, conv[k]);
        }
        return mx + 1;
    };
    bool any = false;
    if (mode == 2) {
        T.prowb.assign((ld + 127) / 128, FPS_NEVER);
        for (int b = 0; b * 128 < N; b++) any |= (T.prowb[b] = row(b * 128, std::min(N, (b + 1) * 128))) != FPS_NEVER;
        if (!any) T.prowb.clear();
    } else {
        for (int kf = 128; kf < N && !any; kf += 128)
            if ((any = row(kf, N) != FPS_NEVER)) {
                T.kfast = kf;
                T.prow = std::min(PRMAX, (row(kf, N) + 15) / 16 * 16);
            }
        T.ptab.resize((size_t)T.prow * ld);
    }
    if (any) T.pinf.assign(ld, 0.0);
    if (any) std::copy(rr.begin(), rr.end(), T.pinf.begin());
}

// the FIXED chunks' candidates (FpsArgs::cfix), each condition compared bit for bit on the tables the device reads:
// from cfix[b] to clast every chunk of block b starts at the fixed point (rp0 = pinf, and past prowb), is whole, does
// not hold global row nx - 1, and shares one (pw, pe) with the row before it.  One rank without an outflow side only
inline void fps_fixed_candidates(const FpsOp& o, FpsTables& T) {
    if (T.prowb.empty() || o.ranks.size() != 1 || o.i0 != 0 || o.nxl != o.nx || o.outE) return;
    const int N = o.ny, ld = o.ld, M = o.M, nb = (int)T.prowb.size();
    auto plain = [&](int c) {   // (the conditions that do not depend on the block)
        const int gi0 = c * M;
        if (gi0 < 1 || gi0 + M > o.nx - 1) return false;
        for (int gi = gi0; gi < gi0 + M; gi++)
            if (std::memcmp(&o.pw[gi], &o.pw[gi0 - 1], sizeof(double)) || std::memcmp(&o.pe[gi], &o.pe[gi0 - 1], sizeof(double)))
                return false;
        return true;
    };
    for (int c = o.nch() - 1; c >= 0 && T.clast < 0; c--)
        if (plain(c)) T.clast = c;
    T.cfix.assign(nb, FPS_NEVER);
    long nfix = 0;
    for (int b = 0; b < nb && T.clast >= 0; b++) {
        if (T.prowb[b] >= o.nx) continue;
        for (int c = T.clast; c >= 0; c--) {
            bool ok = plain(c) && c * M >= T.prowb[b];
            for (int k = b * 128; k < std::min(N, (b + 1) * 128) && ok; k++)
                ok = std::memcmp(&T.rp0()[(size_t)c * ld + k], &T.pinf[k], sizeof(double)) == 0;
            if (!ok) break;
            T.cfix[b] = c;
        }
        if (T.cfix[b] <= T.clast) nfix += T.clast - T.cfix[b] + 1;
    }
    if (nfix == 0) T.cfix.clear();
}

// ... collapsed to one row per block (FpsArgs::fixv, 3 x ld): P (hP: nch x ld, from a run of k_fps_t1b itself), beta and
// BR; a block whose FIXED chunks' rows are not all the same bits has none (cfix[b] <- FPS_NEVER).  Returns the pairs left
inline long fps_fixed_collapse(const FpsOp& o, FpsTables& T, const std::vector<double>& hP, std::vector<double>& fixv) {
    const int N = o.ny, ld = o.ld;
    fixv.assign(3 * (size_t)ld, 0.0);
    const double* tab[3] = {hP.data(), T.bt(), T.bt() + (size_t)o.nch() * ld};
    long nfix = 0;
    for (int b = 0; b < (int)T.cfix.size(); b++) {
        if (T.cfix[b] > T.clast) continue;
        const int k0 = b * 128, nk = std::min(N, k0 + 128) - k0;
        bool ok = true;
        for (int q = 0; q < 3 && ok; q++) {
            const double* row0 = tab[q] + (size_t)T.cfix[b] * ld + k0;
            std::memcpy(&fixv[(size_t)q * ld + k0], row0, nk * sizeof(double));
            for (int c = T.cfix[b] + 1; c <= T.clast && ok; c++)
                ok = std::memcmp(tab[q] + (size_t)c * ld + k0, row0, nk * sizeof(double)) == 0;
        }
        if (ok) nfix += T.clast - T.cfix[b] + 1;
        else T.cfix[b] = FPS_NEVER;
    }
    return nfix;
}

// slabs: mode 0's pivots over the global rows (r0: mu = 0; the last row is pinned, the outflow row too) and its response
// to the constant 1 (the deferred mean) by the kernels' recurrences over f = 1: every local chunk's forward end value
// (m0e) and local back substitution (m0b), the groups' (m0g) and the ranks' (m0a) forward aggregates
inline void fps_mode0_tables(const FpsOp& o, FpsTables& T) {
    const int iend = o.i0 + o.nxl; T.r0.assign(o.nx, 0.0);
    double rp = 0.0, gg, *r0 = T.r0.data();
    for (int gi = 0; gi < o.nx; gi++) rp = r0[gi] = fps_piv_next(fps_row(o, gi), gi == o.nx - 1, 0, 0.0, rp, gg);
    auto step = [&](int gi, double E) { return std::fma(-(o.pw[gi] * (gi > 0 ? r0[gi - 1] : 0.0)), E, 1.0); };
    auto fwd = [&](int ga, int gb) { double E = 0.0; for (int gi = ga; gi < gb; gi++) E = step(gi, E); return E; };
    T.m0e.assign(o.nchp(), 0.0);
    T.m0b = T.m0e;
    std::vector<double> y(o.M);
    for (int c = 0; c < o.nch(); c++) {
        const int gi0 = o.i0 + c * o.M, gi1 = std::min(gi0 + o.M, iend);
        double E = 0.0, xl = 0.0;
        for (int gi = gi0; gi < gi1; gi++) y[gi - gi0] = E = step(gi, E);
        for (int gi = gi1 - 1; gi >= gi0; gi--) xl = std::fma(y[gi - gi0], r0[gi], -o.pe[gi] * r0[gi] * xl);
        T.m0e[c] = E; T.m0b[c] = xl;
    }
    for (int gq = 0; gq < o.ngrp(); gq++)
        T.m0g.push_back(fwd(o.i0 + gq * o.G * o.M, std::min(o.i0 + (gq + 1) * o.G * o.M, iend)));
    for (const auto& q : o.ranks) T.m0a.push_back(fwd(q.first, q.second));
}

// slabs, one allgather per solve (FpsRank::bq / x1): every rank's backward aggregate as a function of its forward
// carry-in Y: with f = 0, y_i = Y prod(-g), x_i = y_i r_i - pe_i r_i x_{i+1}, so B_p(k) = sum_i prod_{m <= i}(-g_m) r_i
// prod_{m < i}(-pe_m r_m) over rank p's rows; X1_p: mode 0's aggregate of f = 1 from zero
inline void fps_rank_aggregates(const FpsOp& o, FpsTables& T) {
    const int N = o.ny; const double* r0 = T.r0.data();
    T.ogb.assign(o.ranks.size() * o.ld, 0.0); T.ogx1.assign(o.ranks.size(), 0.0);
    std::vector<double> rr(N, 0.0), fw(N), bw(N);   // (rr: the pivots run on from rank to rank, from global row 0)
    for (size_t rq = 0; rq < o.ranks.size(); rq++) {
        fw.assign(N, 1.0);
        bw = fw;
        double y1 = 0.0, bw1 = 1.0, gg, *Bq = T.ogb.data() + rq * o.ld;
        for (int gi = o.ranks[rq].first; gi < o.ranks[rq].second; gi++) {
            const FpsRow w = fps_row(o, gi);
            for (int k = 0; k < N; k++) {
                rr[k] = fps_piv_next(w, w.last, k, T.mu[k], rr[k], gg);
                fw[k] *= -gg;
                Bq[k] += fw[k] * rr[k] * bw[k];
                bw[k] *= -o.pe[gi] * rr[k];
            }
            // (mode 0, f = 1: y_i = 1 - g_i y_{i-1}, the same back substitution)
            y1 = std::fma(-(o.pw[gi] * (gi > 0 ? r0[gi - 1] : 0.0)), y1, 1.0);
            T.ogx1[rq] += y1 * r0[gi] * bw1;
            bw1 *= -o.pe[gi] * r0[gi];
        }
    }
}

}   // namespace nsg
