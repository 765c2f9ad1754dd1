// The wall loads' boundary-face list builder (navierstokessolver_amd/csrc/ns_loads_host.h) on the host, stand-alone:
// a rectangle with an edge of more than one chunk, an L-shaped mask with one-face edges, a bad edge index.  Built and
// run under the sanitizers by tests/test_loads_host.py.  No GPU.
#include <cstdio>
#include <vector>

#include "ns_loads_host.h"

#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                               \
        }                                                           \
    } while (0)

// the list's invariants: sorted by (edge, s), CSR offsets, chunks of <= LOAD_CHUNK faces that never span two edges
static int invariants(const nsg::LoadList& L, int n_edges) {
    const int nf = (int)L.face.size();
    CHECK((int)L.s.size() == nf && (int)L.ds.size() == nf);
    CHECK((int)L.fs.size() == n_edges + 1 && (int)L.cs.size() == n_edges + 1);
    CHECK(L.fs[0] == 0 && L.fs[n_edges] == nf && L.cs[0] == 0 && L.cs[n_edges] == (int)L.chunk.size());
    for (int e = 0; e < n_edges; e++) {
        CHECK(L.fs[e] <= L.fs[e + 1] && L.cs[e] <= L.cs[e + 1]);
        for (int f = L.fs[e]; f < L.fs[e + 1]; f++) {
            CHECK((L.face[f].ke >> 2) == e);
            if (f > L.fs[e]) CHECK(L.s[f - 1] < L.s[f]);
        }
        int next = L.fs[e];
        for (int c = L.cs[e]; c < L.cs[e + 1]; c++) {
            const nsg::LoadChunk& C = L.chunk[c];
            CHECK(C.edge == e && C.first == next && C.count >= 1 && C.count <= nsg::LOAD_CHUNK);
            CHECK(c + 1 == L.cs[e + 1] || C.count == nsg::LOAD_CHUNK);
            next += C.count;
        }
        CHECK(next == L.fs[e + 1]);
    }
    return 0;
}

int main() {
    {   // a 300 x 2 rectangle, sides W, E, S, N on edges 0, 2, 3, 1; hx stretched
        const int nx = 300, ny = 2, ld = 128;
        std::vector<double> hx(nx), hy(ny, 0.5);
        for (int i = 0; i < nx; i++) hx[i] = 1.0 + 0.01 * i;
        const int side_edge[4] = {0, 2, 3, 1};
        auto inside = [](int, int) { return true; };
        auto edge_of = [&](int i, int j, int k) {
            const bool b = k == 0 ? i == 0 : k == 1 ? i == nx - 1 : k == 2 ? j == 0 : j == ny - 1;
            return b ? side_edge[k] : -1;
        };
        nsg::LoadList L;
        CHECK(nsg::build_load_list(nx, ny, ld, 4, hx.data(), hy.data(), inside, edge_of, L));
        CHECK(invariants(L, 4) == 0);
        CHECK((int)L.face.size() == 2 * nx + 2 * ny);
        CHECK(L.fs[1] - L.fs[0] == ny && L.fs[2] - L.fs[1] == nx && L.fs[3] - L.fs[2] == ny && L.fs[4] - L.fs[3] == nx);
        CHECK(L.cs[1] - L.cs[0] == 1 && L.cs[2] - L.cs[1] == 2 && L.cs[4] - L.cs[3] == 2);
        CHECK(L.chunk[L.cs[1] + 1].count == nx - 256);
        // the N edge's first face: cell (0, ny - 1), face 3, s = hx[0] / 2, ds = hx[0]
        const nsg::LoadFace& F = L.face[L.fs[1]];
        CHECK(F.li == 0 && F.j == ny - 1 && (F.ke & 3) == 3 && F.o == ny - 1);
        CHECK(L.s[L.fs[1]] == 0.5 * hx[0] && L.ds[L.fs[1]] == hx[0]);
        CHECK(L.face[L.fs[1] + 7].o == 7 * ld + ny - 1);
        CHECK(L.ds[L.fs[0]] == 0.5 && L.s[L.fs[0] + 1] == 0.75);
    }
    {   // an L: the 3 x 3 box without its upper-right cell; six edges, clockwise from the lower-left corner
        const int nx = 3, ny = 3, ld = 128;
        const std::vector<double> hx(nx, 1.0), hy(ny, 1.0);
        auto inside = [](int i, int j) { return !(i == 2 && j == 2); };
        auto edge_of = [&](int i, int j, int k) {
            const int ii = i + (k == 0 ? -1 : k == 1 ? 1 : 0), jj = j + (k == 2 ? -1 : k == 3 ? 1 : 0);
            if (ii >= 0 && ii < nx && jj >= 0 && jj < ny && inside(ii, jj)) return -1;
            if (k == 0) return 0;                    // W
            if (k == 3) return i == 2 ? 3 : 1;       // N: the notch's floor (one face), or the top
            if (k == 1) return j == 2 ? 2 : 4;       // E: the notch's wall (one face), or the right side
            return 5;                                // S
        };
        nsg::LoadList L;
        CHECK(nsg::build_load_list(nx, ny, ld, 6, hx.data(), hy.data(), inside, edge_of, L));
        CHECK(invariants(L, 6) == 0);
        CHECK((int)L.face.size() == 12 && (int)L.chunk.size() == 6);
        CHECK(L.fs[3] - L.fs[2] == 1 && L.fs[4] - L.fs[3] == 1);
        // the corner cell (1, 2) carries two boundary faces: N on edge 1, E on edge 2
        CHECK(L.face[L.fs[2]].li == 1 && L.face[L.fs[2]].j == 2 && (L.face[L.fs[2]].ke & 3) == 1);
        CHECK(L.face[L.fs[1] + 1].li == 1 && L.face[L.fs[1] + 1].j == 2 && (L.face[L.fs[1] + 1].ke & 3) == 3);
        // an edge without faces keeps empty ranges
        nsg::LoadList M;
        CHECK(nsg::build_load_list(nx, ny, ld, 8, hx.data(), hy.data(), inside, edge_of, M));
        CHECK(invariants(M, 8) == 0 && M.fs[8] == 12 && M.fs[7] == 12 && M.cs[7] == M.cs[8]);
        // an edge index past the table: refused
        nsg::LoadList N;
        CHECK(!nsg::build_load_list(nx, ny, ld, 5, hx.data(), hy.data(), inside, edge_of, N));
    }
    std::printf("ok\n");
    return 0;
}
