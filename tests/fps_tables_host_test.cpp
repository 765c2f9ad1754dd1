// Host test of the direct Poisson solve's host tables (navierstokessolver_amd/csrc/ns_fps_tables.h): every table for the
// shapes, x spacings, outflow side and rank splits of tests/test_gpu_fps_setup_bits.py that need no GPU (hy = 1 / ny
// throughout: what is checked here does not depend on it), built without one.  tests/test_fps_tables_host.py
// compiles and runs it under the sanitizers (the index arithmetic: ragged last chunks and groups, slabs that start
// mid-chunk).  Slab ranges are passed in as numbers (ns_slab_range: 96 rows on 2 ranks: 48; on 3: 32, 64; 200 on 3:
// 72, 136).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ns_fps_tables.h"

static int fails = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED line %d (%s): %s\n", __LINE__, what, #x); fails++; } } while (0)

// an operator with its coefficient tables (ns_solver.cpp coef_tables: pw / pe from hx)
struct Op {
    std::vector<double> pw, pe;
    nsg::FpsOp o;
    nsg::FpsTables T;
    bool og = false;   // with the ranks' B_p / X1_p (one allgather per solve)
};

// nx x ny cells over lx x 1 (xratio: the geometric spacing, -1 uniform), this rank of the split `edges` (the slabs'
// first rows after 0)
static Op make(int nx, int ny, double lx, double xratio, int outE, int pmode, std::vector<int> edges = {}, int rank = 0,
               bool og = true) {
    Op p;
    std::vector<double> hx(nx, lx / nx);
    if (xratio > 0) {
        const double h = lx * (xratio - 1) / (std::pow(xratio, nx) - 1);
        for (int i = 0; i < nx; i++) hx[i] = h * std::pow(xratio, i);
    }
    p.pw.assign(nx, 0.0);
    p.pe.assign(nx, 0.0);
    for (int i = 0; i < nx; i++) {
        if (i > 0) p.pw[i] = 2.0 / (hx[i] * (hx[i] + hx[i - 1]));
        if (i < nx - 1) p.pe[i] = 2.0 / (hx[i] * (hx[i] + hx[i + 1]));
    }
    nsg::FpsOp& o = p.o;
    o.nx = nx; o.ny = ny; o.ld = (ny + 127) / 128 * 128;
    edges.insert(edges.begin(), 0);
    edges.push_back(nx);
    for (size_t q = 0; q + 1 < edges.size(); q++) o.ranks.push_back({edges[q], edges[q + 1]});
    o.i0 = o.ranks[rank].first;
    o.nxl = o.ranks[rank].second - o.i0;
    o.pw = p.pw.data(); o.pe = p.pe.data(); o.hy0 = 1.0 / ny; o.outE = outE; o.pmode = pmode;
    p.og = og && o.ranks.size() > 1;
    o.t8 = ny == 16384;
    nsg::fps_twiddles(o, p.T);   // (the families in fps_setup's order)
    nsg::fps_chunk_tables(o, p.T);
    nsg::fps_pivot_shortcut(o, p.T);
    nsg::fps_fixed_candidates(o, p.T);
    if (o.ranks.size() > 1) nsg::fps_mode0_tables(o, p.T);
    if (p.og) nsg::fps_rank_aggregates(o, p.T);
    return p;
}

static bool same(const double* a, const double* b, size_t n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }
static bool same(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && (a.empty() || same(a.data(), b.data(), a.size()));
}

// 1. every vector's size is what fps_setup's arena list asks for (the list takes a host table's count from its vector:
// these are the counts the kernels address)
static void check_sizes(const char* what, const Op& p) {
    const nsg::FpsOp& o = p.o;
    const nsg::FpsTables& T = p.T;
    const size_t N = o.ny, ld = o.ld, nchp = o.nchp(), P = o.ranks.size(), nb = (ld + 127) / 128;
    CHECK(o.nch() == (o.nxl + 15) / 16 && o.ngrp() == (o.nch() + 3) / 4 && nchp == (size_t)o.ngrp() * 4);
    CHECK(T.tw.size() == 2 * N && T.wk.size() == 2 * N && T.mu.size() == N && T.tw8.size() == (o.t8 ? N : 0));
    CHECK(T.ct.size() == 3 * nchp * ld && T.bt() == T.rp0() + nchp * ld);   // (rp0 | bt: one block)
    CHECK(T.pinf.size() == (T.ptab.empty() && T.prowb.empty() ? 0 : ld));
    CHECK(T.ptab.size() == (size_t)T.prow * ld && (T.ptab.empty() || T.prowb.empty()));
    CHECK(T.prowb.empty() || (T.prowb.size() == nb && o.pmode == 2));
    CHECK(T.cfix.empty() || (T.cfix.size() == T.prowb.size() && T.clast >= 0 && T.clast < o.nch()));
    CHECK(T.m0e.size() == (P > 1 ? nchp : 0) && T.m0b.size() == T.m0e.size());
    CHECK(T.m0g.size() == (P > 1 ? (size_t)o.ngrp() : 0) && T.m0a.size() == (P > 1 ? P : 0));
    CHECK(T.ogb.size() == (p.og ? P * ld : 0) && T.ogx1.size() == (p.og ? P : 0));
}

// 2. a slab that starts on a chunk boundary: its rp0 rows are the one-rank table's rows at the same global chunks bit
// for bit, and so are beta / BR of the chunks that are whole in both
static void check_slab_rows(const char* what, const Op& slab, const Op& one) {
    const nsg::FpsOp &o = slab.o, &g = one.o;
    const size_t N = o.ny, ld = o.ld;
    CHECK(o.i0 % o.M == 0);
    const int c0 = o.i0 / o.M;
    for (int c = 0; c < o.nch(); c++) {
        CHECK(same(&slab.T.rp0()[c * ld], &one.T.rp0()[(c0 + c) * ld], N));
        if ((c + 1) * o.M > o.nxl || (c0 + c + 1) * o.M > g.nx) continue;   // (ragged in one of them)
        CHECK(same(&slab.T.bt()[c * ld], &one.T.bt()[(c0 + c) * ld], N));
        CHECK(same(&slab.T.bt()[(o.nch() + c) * ld], &one.T.bt()[(g.nch() + c0 + c) * ld], N));
    }
}

// 3. shortcut mode 2: from a block's fixed-point row on, one more row of the recurrence from pinf returns pinf
static void check_fixed_points(const char* what, const Op& p) {
    const nsg::FpsOp& o = p.o;
    for (size_t b = 0; b < p.T.prowb.size(); b++) {
        const int gi = p.T.prowb[b];
        if (gi >= nsg::FPS_NEVER) continue;
        CHECK(gi > 1 && gi <= o.nx - 1);
        if (gi >= o.nx - 1) continue;   // (the last row has no east neighbour: no row of the fixed point)
        for (int k = (int)b * 128; k < std::min(o.ny, ((int)b + 1) * 128); k++) {
            double g;
            const double rn = nsg::fps_piv_next(nsg::fps_row(o, gi), false, k, p.T.mu[k], p.T.pinf[k], g);
            CHECK(same(&rn, &p.T.pinf[k], 1));
        }
    }
}

// 4. outE = 0 against outE = 1: the tables differ only where global row nx - 1 enters -- the last chunk's beta / BR
static void check_outflow(const char* what, const Op& w, const Op& e) {
    const nsg::FpsOp& o = w.o;
    const size_t N = o.ny, ld = o.ld;
    CHECK(same(w.T.rp0(), e.T.rp0(), (size_t)o.nchp() * ld) && same(w.T.mu, e.T.mu) && same(w.T.pinf, e.T.pinf) && same(w.T.ptab, e.T.ptab));
    CHECK(w.T.prowb == e.T.prowb && same(w.T.tw, e.T.tw) && same(w.T.wk, e.T.wk));
    const int last = o.nch() - 1;
    for (int c = 0; c < last; c++) {
        CHECK(same(&w.T.bt()[c * ld], &e.T.bt()[c * ld], N));
        CHECK(same(&w.T.bt()[(o.nch() + c) * ld], &e.T.bt()[(o.nch() + c) * ld], N));
    }
    CHECK(!same(&w.T.bt()[last * ld], &e.T.bt()[last * ld], N));   // (the eliminated row is another row)
    CHECK(e.T.cfix.empty());                                   // (and no FIXED chunks beside it)
}

int main() {
    const char* what = "";
    struct Shape { const char* name; int nx, ny; double lx, xratio; int outE, pmode; };
    const Shape shapes[] = {
        {"33x16", 33, 16, 33.0 / 16, -1, 0, 2},         {"40x96", 40, 96, 40.0 / 96, -1, 0, 2},
        {"64x256", 64, 256, 0.25, -1, 0, 2},            {"200x512", 200, 512, 200.0 / 512, -1, 0, 2},
        {"200x512 ptab0", 200, 512, 200.0 / 512, -1, 0, 0}, {"200x512 ptab1", 200, 512, 200.0 / 512, -1, 0, 1},
        {"520x1024", 520, 1024, 520.0 / 1024, -1, 0, 2}, {"2048x512 lx8", 2048, 512, 8.0, -1, 0, 2},
        {"96x128 xratio", 96, 128, 0.75, 1.02, 0, 0},   {"32x16384", 32, 16384, 32.0 / 16384, -1, 0, 2},
        {"channel 128x256", 128, 256, 4.0, -1, 1, 2},   {"96x256", 96, 256, 1.0, -1, 0, 2},
    };
    for (const Shape& s : shapes) {
        what = s.name;
        const Op p = make(s.nx, s.ny, s.lx, s.xratio, s.outE, s.pmode);
        check_sizes(what, p);
        check_fixed_points(what, p);
        const bool shortcut = !p.T.prowb.empty() || !p.T.ptab.empty();
        if (s.pmode == 0 || s.ny <= 128 || s.nx - 1 <= 64) CHECK(!shortcut && p.T.pinf.empty() && p.T.cfix.empty());
    }
    {   // 5. what test_gpu_fps_fixed.py asserts from the census: 64 x 256 no shortcut, 200 x 512 one -- block 1's
        // fixed-point row is no multiple of 16, so the chunk holding it is general and the next one FIXED
        what = "census";
        const Op a = make(64, 256, 0.25, -1, 0, 2), b = make(200, 512, 200.0 / 512, -1, 0, 2);
        CHECK(a.T.prowb.empty() && a.T.pinf.empty() && a.T.cfix.empty());
        CHECK(b.T.prowb.size() == 4 && b.T.cfix.size() == 4 && b.T.clast == 11);
        if (b.T.cfix.size() == 4) {
            CHECK(b.T.prowb[1] < 200 && b.T.prowb[1] % 16 != 0 && b.T.cfix[1] == b.T.prowb[1] / 16 + 1);
            for (int q = 0; q < 4; q++) CHECK(b.T.cfix[q] > b.T.clast || (b.T.cfix[q] > 0 && b.T.cfix[q] <= b.T.clast));
        }
        const Op t = make(200, 512, 200.0 / 512, -1, 0, 1);   // (the table: whole waves of modes from kfast on)
        CHECK(!t.T.ptab.empty() && t.T.kfast % 128 == 0 && t.T.kfast < 512 && t.T.prow % 16 == 0 && t.T.prowb.empty());
    }
    {   // slabs: 96 rows on 2 and 3 ranks (edges on chunk boundaries), 200 on 3 (72 / 64 / 64: mid-chunk), the channel
        const Op one = make(96, 256, 1.0, -1, 0, 2);
        const std::vector<std::vector<int>> splits = {{48}, {32, 64}};
        for (const auto& e : splits)
            for (int r = 0; r <= (int)e.size(); r++) {
                what = e.size() == 1 ? "96x256 on 2" : "96x256 on 3";
                const Op p = make(96, 256, 1.0, -1, 0, 2, e, r);
                check_sizes(what, p);
                check_slab_rows(what, p, one);
                CHECK(p.T.cfix.empty());   // (FIXED chunks: one rank only)
            }
        for (int r = 0; r < 3; r++)
            for (int og = 0; og < 2; og++) {
                what = "200x512 on 3";
                const Op p = make(200, 512, 1.0, -1, 0, 2, {72, 136}, r, og != 0);
                check_sizes(what, p);
                check_fixed_points(what, p);
            }
        for (int r = 0; r < 2; r++) {
            what = "channel 128x256 on 2";
            check_sizes(what, make(128, 256, 1.0, -1, 1, 2, {64}, r));
        }
        // the ranks' forward aggregates of the constant 1 are every rank's own view of the same numbers
        what = "m0a";
        CHECK(same(make(200, 512, 1.0, -1, 0, 2, {72, 136}, 0).T.m0a, make(200, 512, 1.0, -1, 0, 2, {72, 136}, 2).T.m0a));
    }
    what = "outE";
    check_outflow(what, make(128, 256, 4.0, -1, 0, 2), make(128, 256, 4.0, -1, 1, 2));
    if (fails == 0) std::printf("ok\n");
    return fails != 0;
}
