// ns_loads_host.h -- the boundary-face list of the wall loads (ns_loads_*; DESIGN.md 4, "Wall loads"), built once on
// the host by ns_loads_enable.  Plain C++ with no HIP in it: tests/loads_host_test.cpp drives it stand-alone under the
// sanitizers.  Not installed.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace nsg {

constexpr int LOAD_CHUNK = 256;   // faces per workgroup of k_load_faces: the unit of the sums' fixed order

// one boundary face: face k (0 W, 1 E, 2 S, 3 N) of the domain cell (li, j) at plane offset o = li * ld + j, on the
// grid's edge e (ke = k | e << 2).  16 bytes: the kernel reads it as one int4
struct LoadFace {
    int32_t o, li, j, ke;
};
// one workgroup's faces: `count` (<= LOAD_CHUNK) of them from `first`, all on `edge`
struct LoadChunk {
    int32_t first, count, edge, pad;
};
// faces sorted by edge, then by s (ties, which a straight edge does not have, by cell and face); fs / cs: the CSR
// offsets of each edge's faces / chunks (n_edges + 1 entries).  s: the face centre's coordinate along its edge from
// the box's lower-left corner; ds: the face's length
struct LoadList {
    std::vector<LoadFace> face;
    std::vector<double> s, ds;
    std::vector<LoadChunk> chunk;
    std::vector<int32_t> fs, cs;
};

// inside(i, j): cell (i, j) of the nx x ny box is in the domain; edge_of(i, j, k): the edge on face k of that domain
// cell, or -1 where the neighbour is in the domain.  An edge index outside [0, n_edges) is an error: false
template <class In, class Edge>
bool build_load_list(int nx, int ny, int ld, int n_edges, const double* hx, const double* hy, In&& inside, Edge&& edge_of,
                     LoadList& L) {
    std::vector<double> xf((size_t)nx + 1, 0.0), yf((size_t)ny + 1, 0.0);   // summed one by one, as the tracers' faces
    for (int i = 0; i < nx; i++) xf[i + 1] = xf[i] + hx[i];
    for (int j = 0; j < ny; j++) yf[j + 1] = yf[j] + hy[j];
    struct Rec {
        LoadFace f;
        double s, ds;
    };
    std::vector<Rec> rec;
    for (int i = 0; i < nx; i++)
        for (int j = 0; j < ny; j++) {
            if (!inside(i, j)) continue;
            for (int k = 0; k < 4; k++) {
                const int e = edge_of(i, j, k);
                if (e == -1) continue;
                if (e < 0 || e >= n_edges) return false;
                Rec r;
                r.f = LoadFace{(int32_t)(i * ld + j), i, j, k | e << 2};
                r.s = k < 2 ? 0.5 * (yf[j] + yf[j + 1]) : 0.5 * (xf[i] + xf[i + 1]);
                r.ds = k < 2 ? hy[j] : hx[i];
                rec.push_back(r);
            }
        }
    std::sort(rec.begin(), rec.end(), [](const Rec& a, const Rec& b) {
        const int ea = a.f.ke >> 2, eb = b.f.ke >> 2;
        if (ea != eb) return ea < eb;
        if (a.s != b.s) return a.s < b.s;
        if (a.f.o != b.f.o) return a.f.o < b.f.o;
        return a.f.ke < b.f.ke;
    });
    L = LoadList{};
    L.fs.assign((size_t)n_edges + 1, 0);
    L.cs.assign((size_t)n_edges + 1, 0);
    for (const Rec& r : rec) {
        L.face.push_back(r.f);
        L.s.push_back(r.s);
        L.ds.push_back(r.ds);
        L.fs[(r.f.ke >> 2) + 1]++;
    }
    for (int e = 0; e < n_edges; e++) {
        const int n = L.fs[e + 1];
        L.fs[e + 1] = L.fs[e] + n;
        for (int a = 0; a < n; a += LOAD_CHUNK)
            L.chunk.push_back(LoadChunk{L.fs[e] + a, std::min(LOAD_CHUNK, n - a), e, 0});
        L.cs[e + 1] = (int32_t)L.chunk.size();
    }
    return true;
}

}  // namespace nsg
