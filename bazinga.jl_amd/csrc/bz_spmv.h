// bz_spmv.h — the sparse affine constraint c(x) = A x - b (BZ_C_SPARSE_AFFINE): the two row kernels of its AL gradient.
//
// A and A' are two CSR matrices in HBM (A' is built once, at bz_problem_create, by a stable counting sort).  Both passes
// are the same row kernel: L lanes (compile time, 1..64, chosen at creation from the mean row length) walk one row, lane
// l taking the entries l, l + L, l + 2L, ... in stored order and accumulating in T; the L lane sums are folded by a fixed
// xor tree carried in double.  A row's value is therefore a function of the stored order and of L alone: no atomics,
// nothing that depends on the grid or on timing.
//   k_spmv_yupd      rows of A :  c_i = sum a_ij x_j - b_i, and on that value what k_yupd does with it
//   k_spmv_t_finish  rows of A':  (A' yhat)_j, and on that value what k_gemv_t_finish does with it
// Rows longer than S entries (S fixed at creation from the matrix alone) are cut into segments that run as rows of
// their own ("virtual rows": the row pointers refined at the cuts); a segment leaves its sum in a side buffer and
// k_spmv_fold, one wave per cut row, adds a row's segment sums in a fixed order and runs the row's epilogue.
//
// Kept apart from bz_kernels.h because only bz_solver.hip instantiates these templates: the sixteen family translation
// units do not see (or rebuild for) them.
#pragma once
#include "bz_kernels.h"

namespace bz {

template <class T> struct SpMat {
    const int64_t* ptr;      // [nv + 1] entry offsets of the virtual rows
    const int32_t* col;      // [nnz] 0-based, any order inside a row
    const T* val;            // [nnz]
    const int32_t* vrow;     // cut matrices: [nv] the row a virtual row belongs to; null: virtual row v IS row v
    const int32_t* vpart;    // cut matrices: [nv] -1: a whole row; otherwise where this segment's sum goes in `part`
    double* part;            // cut matrices: the segment sums
    int64_t nv;
};

// what a row's value goes into.  MODE 0 (rows of A): cx (if kept), yupd (if wanted: null = eval!(cx, c, x) alone) and
// the penalty term; MODE 1 (rows of A'): the gradient and the f term.
template <class T> struct SpEpi {
    const T* b;              // MODE 0: b[ny]
    T* cx;                   // MODE 0: c(x) for the caller that keeps it, or null
    T* out;                  // MODE 0: yupd[ny] or null ; MODE 1: grad[n] or null
    const T* x;              // MODE 1: x[n]
    ElemParams<T> P;
};

template <class T, int MODE>
__device__ __forceinline__ double sp_epilogue(const SpEpi<T>& E, int64_t r, double d) {
    const ElemParams<T>& P = E.P;
    if constexpr (MODE == 0) {
        const T c = (T)d - E.b[r];                                  // eval!(cx, c, x)
        if (E.cx) E.cx[r] = c;
        if (!E.out) return 0.0;
        // t = cx + muy ; s = proj_D(t) ; t -= s ; sum t^2/mu ; yupd = t/mu      (k_yupd)
        const T mu = P.uni >= 1 ? P.mu_uniform : P.mu[r];
        const T muy = P.uni >= 2 ? T(0) : P.muy[r];
        const T lo = P.D_lo_vec ? P.D_lo_vec[r] : P.D_lo;
        const T hi = P.D_hi_vec ? P.D_hi_vec[r] : P.D_hi;
        T t = c + muy;
        const T sv = proj_D(P.D_kind, t, lo, hi);
        t = t - sv;
        const T pterm = (t * t) / mu;
        E.out[r] = t / mu;
        return (double)pterm;
    } else {
        // dlx = dfx + jtv ; f element-wise (Zero | DiagQuadratic)               (k_gemv_t_finish)
        T dfx = T(0), fterm = T(0);
        if (P.f_kind == BZ_F_DIAG_QUADRATIC) {
            const T xv = E.x[r];
            const T qx = P.q[r] * xv;
            dfx = qx - P.b[r];
            fterm = xv * (T(0.5) * qx - P.b[r]);
        }
        if (E.out) E.out[r] = dfx + (T)d;
        return (double)fterm;
    }
}

template <class V, bool NT> __device__ __forceinline__ V sp_ld(const V* p) {
    if constexpr (NT) return __builtin_nontemporal_load(p); else return *p;
}

// the entries [s, e) of one row, this lane being number `sub` of the row's L: four entries per lane in flight, every
// load unconditional (an index past the row's end is clamped to its last entry and the product dropped).  Every lane
// of the row's group returns the folded sum.
template <class T, int L, bool NT>
__device__ __forceinline__ double spmv_row(const SpMat<T>& M, const T* __restrict__ g, int64_t s, int64_t e, int sub) {
    constexpr int U = 4;
    const int64_t last = e > 0 ? e - 1 : 0;      // (an empty matrix: entry 0 of the zero-filled slack behind the arrays)
    T acc = T(0);
    for (int64_t k = s + sub; k < e; k += (int64_t)U * L) {
        int32_t c[U];
        T a[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t kk = k + (int64_t)u * L;
            const int64_t kc = kk < e ? kk : last;
            c[u] = sp_ld<int32_t, NT>(M.col + kc);
            a[u] = sp_ld<T, NT>(M.val + kc);
        }
        T xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) xv[u] = g[c[u]];      // default policy: the gathered vector is what the caches are for
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const T p = a[u] * xv[u];
            acc += (k + (int64_t)u * L < e) ? p : T(0);
        }
    }
    double d = (double)acc;
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, 64);
    return d;
}

// the row loop shared by the two passes: virtual row v belongs to the L lanes (blockIdx.x * BLOCK + threadIdx.x) / L,
// then grid-strides.  Returns this thread's share of the pass's scalar (the row's first lane carries the row's term).
template <class T, int L, bool NT, int MODE>
__device__ __forceinline__ double spmv_rows(const SpMat<T>& M, const T* __restrict__ g, const SpEpi<T>& E) {
    constexpr int RPB = BLOCK / L;
    const int sub = threadIdx.x % L;
    double acc = 0.0;
    for (int64_t v = (int64_t)blockIdx.x * RPB + threadIdx.x / L; v < M.nv; v += (int64_t)gridDim.x * RPB) {
        const int64_t s = M.ptr[v], e = M.ptr[v + 1];
        const double d = spmv_row<T, L, NT>(M, g, s, e, sub);
        if (sub == 0) {
            int64_t r = v;
            int pi = -1;
            if (M.vrow) { pi = M.vpart[v]; r = M.vrow[v]; }
            if (pi >= 0) M.part[pi] = d;      // a segment of a cut row: k_spmv_fold finishes the row
            else acc += sp_epilogue<T, MODE>(E, r, d);
        }
    }
    return acc;
}

template <class T, int L, bool NT>
__global__ void __launch_bounds__(BLOCK)
k_spmv_yupd(SpMat<T> M, const T* __restrict__ x, SpEpi<T> E, double* __restrict__ parts, int slot0) {
    double acc[1] = {spmv_rows<T, L, NT, 0>(M, x, E)};
    block_reduce_store<1>(acc, 0u, parts, slot0);
}

template <class T, int L, bool NT>
__global__ void __launch_bounds__(BLOCK)
k_spmv_t_finish(SpMat<T> M, const T* __restrict__ yupd, SpEpi<T> E, double* __restrict__ parts, int slot0) {
    double acc[1] = {spmv_rows<T, L, NT, 1>(M, yupd, E)};
    block_reduce_store<1>(acc, 0u, parts, slot0);
}

// the cut rows: one wave per row adds the row's segment sums (lane l the sums l, l + 64, ... in order, then the fixed
// xor tree) and runs the row's epilogue; its block partials continue the slot behind the row kernel's (vb0).
template <class T, int MODE>
__global__ void __launch_bounds__(BLOCK)
k_spmv_fold(const double* __restrict__ part, const int32_t* __restrict__ crow, const int32_t* __restrict__ cptr, int ncut,
            SpEpi<T> E, double* __restrict__ parts, int slot0, int vb0) {
    const int lane = threadIdx.x & 63;
    double acc[1] = {0.0};
    for (int j = blockIdx.x * WAVES + (threadIdx.x >> 6); j < ncut; j += gridDim.x * WAVES) {
        const int k1 = cptr[j + 1];
        double a = 0.0;
        for (int k = cptr[j] + lane; k < k1; k += 64) a += part[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if (lane == 0) acc[0] += sp_epilogue<T, MODE>(E, crow[j], a);
    }
    block_reduce_store<1>(acc, 0u, parts, slot0, vb0 + (int)blockIdx.x);
}

}  // namespace bz
