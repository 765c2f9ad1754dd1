// ns_loads.hip -- wall loads (ns_loads_*; DESIGN.md 4, "Wall loads"; the normative statement is tests/loads_ref.py):
// the scheme's own boundary fluxes on every boundary face of the domain and their sums per edge.
//   k_load_faces  one workgroup per chunk of the host-built face list (<= 256 faces of ONE edge, in list order), one
//                 thread per face: the face's p, tx, ty, un, tb, qn (stored SoA) and the chunk's partial of the eight
//                 edge sums by a fixed tree
//   k_load_edges  an edge's chunk partials added in ascending order -> the record
// No floating-point atomics anywhere: the order of every sum is a function of the face list alone, so a record is
// reproducible bit for bit.  Faces on x-normal edges are contiguous in j and coalesce; faces on y-normal edges lie ld
// doubles apart and do not (accepted: a 4096^2 box has 16 K faces).
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include "ns_cell.h"
#include "ns_internal.h"

namespace nsg {

// The statement's expressions, contraction off: exactly its IEEE operations
// (ghost - q) / (re h): the diffusive flux of a velocity component through the face (pe for the scalar)
__device__ __forceinline__ double ld_flux(double ghost, double q, double re, double h) {
#pragma clang fp contract(off)
    return (ghost - q) / (re * h);
}
__device__ __forceinline__ double ld_dot(double fu, double nx, double fv, double ny) {
#pragma clang fp contract(off)
    return fu * nx + fv * ny;
}
__device__ __forceinline__ double ld_tghost(double q, double c) {
#pragma clang fp contract(off)
    return -q + c;
}

// 256 threads' x[8] -> out[8]: the wave's xor butterfly (32, 16, .. 1), then the four waves' sums in wave order
__device__ __forceinline__ void ld_block_sum(double (&x)[8], double* __restrict__ out) {
    __shared__ double sh[4][8];
#pragma unroll
    for (int k = 0; k < 8; k++)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x[k] += __shfl_xor(x[k], off, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 8; k++) sh[w][k] = x[k];
    __syncthreads();
    if (threadIdx.x < 8) out[threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

template <class T>
__global__ __launch_bounds__(256) void k_load_faces(LoadArgs A) {
    const Geo& g = A.g;
    const Coef& c = A.c;
    const LoadChunk ch = A.chunk[blockIdx.x];
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if ((int)threadIdx.x < ch.count) {
        const int f = ch.first + threadIdx.x;
        const int4 F = *reinterpret_cast<const int4*>(A.face + f);   // o, li, j, k | e << 2
        const ptrdiff_t o = F.x;
        const int li = F.y, j = F.z, k = F.w & 3, gi = g.i0 + li;
        const T t(g, li, j);
        const double hx = c.hx[gi], hy = c.hy[j];
        const double h = k < 2 ? hx : hy, ds = k < 2 ? hy : hx;
        const double nx = k == 0 ? -1.0 : k == 1 ? 1.0 : 0.0, ny = k == 2 ? -1.0 : k == 3 ? 1.0 : 0.0;
        const double uc = A.u[o], vc = A.v[o];
        // the pressure of the adjacent cell: the derived fields' own cell pass (its vorticity and divergence unused)
        double p, w_, d_;
        {
            auto U = [&](int di, int dj) { return A.u[o + (ptrdiff_t)di * g.ld + dj]; };
            auto V = [&](int di, int dj) { return A.v[o + (ptrdiff_t)di * g.ld + dj]; };
            auto P = [&](int di, int dj) { return A.phi[o + (ptrdiff_t)di * g.ld + dj]; };
            auto X = [&](int q) { return q == 0 ? hx : q == 1 ? c.fwx[gi] : q == 2 ? c.fex[gi] : q == 3 ? c.pw[gi] : q == 4 ? c.pe[gi] : dv_rcp(hx); };
            auto Y = [&](int q) { return q == 0 ? hy : q == 1 ? c.fsy[j] : q == 2 ? c.fny[j] : q == 3 ? c.ps[j] : q == 4 ? c.pn[j] : dv_rcp(hy); };
            derived_cell<T, false>(g, A.alpha, U, V, P, X, Y, li, j, p, w_, d_);
        }
        // the velocity ghosts across this face (edge profiles through the topology), the tractions, Div_V's face values
        const double gu = t.gv(0, 0, k, uc, 0), gv = t.gv(0, 0, k, vc, 1);
        const double tx = ld_flux(gu, uc, A.re, h), ty = ld_flux(gv, vc, A.re, h);
        const double un = ld_dot(dv_wall(uc, gu), nx, dv_wall(vc, gv), ny);
        double tb = 0.0, qn = 0.0;
        if (A.T) {
            const double tc = A.T[o];
            const double gt = A.tneu[k] ? tc : ld_tghost(tc, A.tc[k]);
            tb = dv_wall(tc, gt);
            qn = -ld_flux(gt, tc, A.pe, h);
        }
        double* __restrict__ val = A.val + f;
        const size_t nf = (size_t)A.nf;
        val[0] = p;
        val[nf] = tx;
        val[2 * nf] = ty;
        val[3 * nf] = un;
        val[4 * nf] = tb;
        val[5 * nf] = qn;
        acc[0] = ds;                                   // NS_LOAD_LEN
        acc[1] = dv_mul(dv_mul(p, nx), ds);            // NS_LOAD_FPX
        acc[2] = dv_mul(dv_mul(p, ny), ds);            // NS_LOAD_FPY
        acc[3] = -dv_mul(tx, ds);                      // NS_LOAD_FVX
        acc[4] = -dv_mul(ty, ds);                      // NS_LOAD_FVY
        acc[5] = dv_mul(un, ds);                       // NS_LOAD_Q
        acc[6] = dv_mul(qn, ds);                       // NS_LOAD_HEAT
        acc[7] = dv_mul(dv_mul(un, tb), ds);           // NS_LOAD_HEAT_ADV
    }
    ld_block_sum(acc, A.part + 8 * (size_t)blockIdx.x);
}

// thread 8 e + q: sum q of edge e
__global__ __launch_bounds__(256) void k_load_edges(const double* __restrict__ part, const int32_t* __restrict__ cs,
                                                    int n_edges, double* __restrict__ out) {
    const int t = threadIdx.x;
    if (t >= 8 * n_edges) return;
    const int e = t >> 3, q = t & 7;
    double s = 0.0;
    for (int k = cs[e]; k < cs[e + 1]; k++) s += part[8 * (size_t)k + q];
    out[t] = s;
}

template <class K, class... Args>
static int load_go(K kern, dim3 grid, hipStream_t st, Args... args) {
    hipEvent_t a, b;
    if (take_launch_timing(a, b)) hipExtLaunchKernelGGL(kern, grid, dim3(256), 0, st, a, b, 0, args...);
    else hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, args...);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_load_faces(const LoadArgs& A, hipStream_t st) {
    if (A.nf <= 0 || A.nchunk <= 0 || A.g.nxl != A.g.nx || A.g.i0 != 0) return -1;
    if (A.g.fc) {
        LoadArgs B = A;
        B.T = nullptr;   // (a masked domain carries no scalar: ns_scalar_enable refuses it)
        return load_go(k_load_faces<TopoMask>, dim3(A.nchunk), st, B);
    }
    return load_go(k_load_faces<TopoRect>, dim3(A.nchunk), st, A);
}

int launch_load_edges(const LoadArgs& A, double* out, hipStream_t st) {
    if (A.n_edges < 1 || A.n_edges > MAX_EDGES || !out) return -1;   // (8 x 31 threads: one workgroup)
    return load_go(k_load_edges, dim3(1), st, (const double*)A.part, A.cs, A.n_edges, out);
}

}  // namespace nsg
