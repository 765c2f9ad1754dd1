// ns_avg.hip -- running flow statistics (ns_avg_*; DESIGN.md 4, "Flow statistics"; the normative statement is
// tests/stats_ref.py): k_moments, one sample of the source planes folded into the running means and the central
// co-moment sums.  A pure pointwise stream: no topology, no Geo tables, no ghost rows -- cells outside a polygon are
// exactly 0 in every source plane, so they stay exactly 0 in every statistics plane.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ns_internal.h"

namespace nsg {

// The update of the statement, contraction off: exactly its sequence of IEEE operations (no FMA), so the planes can
// be compared with the NumPy restatement bit for bit.  d = x - m, m' = m + w d; S' = S + d (y - m_y')
__device__ __forceinline__ void mo_mean(double x, double w, double& m, double& d) {
#pragma clang fp contract(off)
    d = x - m;
    m = m + w * d;
}
__device__ __forceinline__ double mo_co(double S, double d, double y, double my) {
#pragma clang fp contract(off)
    return S + d * (y - my);
}

// W columns of one row at p: a 16-byte access for a lane's two columns, 8 bytes for an odd ny's tail lane
template <int W>
__device__ __forceinline__ void mo_ld(const double* __restrict__ p, double* r) {
    if constexpr (W == 2) {
        const double2 t = *reinterpret_cast<const double2*>(p);
        r[0] = t.x;
        r[1] = t.y;
    } else {
        r[0] = p[0];
    }
}
template <int W>
__device__ __forceinline__ void mo_st(double* __restrict__ p, const double* r) {
    if constexpr (W == 2) *reinterpret_cast<double2*>(p) = make_double2(r[0], r[1]);
    else p[0] = r[0];
}

// the co-moment planes of an instantiation: uu, vv, uv, then TT, uT, vT, then pp
template <int NSRC, bool SECOND, bool HAS_T>
struct MoPlan {
    static constexpr bool HAS_P = NSRC > 2 + (HAS_T ? 1 : 0);
    static constexpr int NS = SECOND ? 3 + (HAS_T ? 3 : 0) + (HAS_P ? 1 : 0) : 0;
};

template <int NSRC, bool SECOND, bool HAS_T, int W>
__device__ __forceinline__ void mo_cells(const MomArgs& A, size_t o) {
    using P = MoPlan<NSRC, SECOND, HAS_T>;
    constexpr int NS = P::NS;
    double x[NSRC][W], m[NSRC][W], d[NSRC][W], S[NS > 0 ? NS : 1][W];
    // every load of the cell pair before the first use: all of them independent
#pragma unroll
    for (int k = 0; k < NSRC; k++) mo_ld<W>(A.src[k] + o, x[k]);
#pragma unroll
    for (int k = 0; k < NSRC; k++) mo_ld<W>(A.mean[k] + o, m[k]);
#pragma unroll
    for (int k = 0; k < NS; k++) mo_ld<W>(A.S[k] + o, S[k]);
#pragma unroll
    for (int k = 0; k < NSRC; k++)
#pragma unroll
        for (int e = 0; e < W; e++) mo_mean(x[k][e], A.w, m[k][e], d[k][e]);
    if constexpr (SECOND) {
#pragma unroll
        for (int e = 0; e < W; e++) {
            S[0][e] = mo_co(S[0][e], d[0][e], x[0][e], m[0][e]);   // uu
            S[1][e] = mo_co(S[1][e], d[1][e], x[1][e], m[1][e]);   // vv
            S[2][e] = mo_co(S[2][e], d[0][e], x[1][e], m[1][e]);   // uv: du of u's old mean, v's new mean
            if constexpr (HAS_T) {
                S[3][e] = mo_co(S[3][e], d[2][e], x[2][e], m[2][e]);   // TT
                S[4][e] = mo_co(S[4][e], d[0][e], x[2][e], m[2][e]);   // uT
                S[5][e] = mo_co(S[5][e], d[1][e], x[2][e], m[2][e]);   // vT
            }
            if constexpr (P::HAS_P)
                S[NS - 1][e] = mo_co(S[NS - 1][e], d[NSRC - 1][e], x[NSRC - 1][e], m[NSRC - 1][e]);   // pp
        }
    }
#pragma unroll
    for (int k = 0; k < NSRC; k++) mo_st<W>(A.mean[k] + o, m[k]);
#pragma unroll
    for (int k = 0; k < NS; k++) mo_st<W>(A.S[k] + o, S[k]);
}

// block (64, 4): a wave takes 128 columns of one row, two per lane; the rows are strided over the grid's y extent.
// A lane whose columns are >= ny neither loads nor stores (the ld padding; of an odd ny's tail lane the second column)
template <int NSRC, bool SECOND, bool HAS_T>
__global__ __launch_bounds__(256) void k_moments(MomArgs A) {
    const int j = 2 * (int)(blockIdx.x * 64 + threadIdx.x);
    if (j >= A.ny) return;
    const bool pair = j + 1 < A.ny;
    for (int i = blockIdx.y * 4 + threadIdx.y; i < A.nxl; i += 4 * gridDim.y) {
        const size_t o = (size_t)i * A.ld + j;
        if (pair) mo_cells<NSRC, SECOND, HAS_T, 2>(A, o);
        else mo_cells<NSRC, SECOND, HAS_T, 1>(A, o);
    }
}

template <int NSRC, bool SECOND, bool HAS_T>
static int moments_go(const MomArgs& A, hipStream_t st) {
    using P = MoPlan<NSRC, SECOND, HAS_T>;
    auto odd = [](const void* p) { return !p || (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
    for (int k = 0; k < NSRC; k++)
        if (odd(A.src[k]) || odd(A.mean[k])) return -1;
    for (int k = 0; k < P::NS; k++)
        if (odd(A.S[k])) return -1;
    if (A.nxl < 1 || A.ny < 1 || A.ld < A.ny || (A.ld & 1)) return -1;
    // memory-bound: about 2048 workgroups, the rows grid-strided over them
    const int gx = (A.ny + 127) / 128, rows4 = (A.nxl + 3) / 4;
    const int gy = std::min(rows4, std::max(1, 2048 / gx));
    const dim3 grid(gx, gy), block(64, 4);
    hipEvent_t a, b;
    if (take_launch_timing(a, b)) hipExtLaunchKernelGGL((k_moments<NSRC, SECOND, HAS_T>), grid, block, 0, st, a, b, 0, A);
    else hipLaunchKernelGGL((k_moments<NSRC, SECOND, HAS_T>), grid, block, 0, st, A);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_moments(const MomArgs& A, int nsrc, bool second, bool has_t, hipStream_t st) {
    const int key = nsrc * 4 + (second ? 2 : 0) + (has_t ? 1 : 0);
    switch (key) {
        case 2 * 4 + 0: return moments_go<2, false, false>(A, st);
        case 2 * 4 + 2: return moments_go<2, true, false>(A, st);
        case 3 * 4 + 0: return moments_go<3, false, false>(A, st);   // u, v, P
        case 3 * 4 + 2: return moments_go<3, true, false>(A, st);
        case 3 * 4 + 1: return moments_go<3, false, true>(A, st);    // u, v, T
        case 3 * 4 + 3: return moments_go<3, true, true>(A, st);
        case 4 * 4 + 1: return moments_go<4, false, true>(A, st);    // u, v, T, P
        case 4 * 4 + 3: return moments_go<4, true, true>(A, st);
        default: return -1;
    }
}

}  // namespace nsg
