// bz_spmm.h — the K-wide CSR row kernels of the sparse multinomial (softmax) f (BZ_F_SPARSE_MULTINOMIAL):
//   f(X) = sum_i w_i (logsumexp_k(t_ik) - t_{i,b_i}),  T = A_f X,  X n_f x K row-major (class fastest: x[j * K + k]),
// and of the sparse multi-response GLM f (BZ_F_SPARSE_MULTI_GLM), the same passes with K independent row losses as the epilogue:
//   f(X) = sum_i w_i sum_k l(b_ik, t_ik),  B m x K row-major  (k_spmm_glm_r<LOSS> in k_spmm_softmax_r's place).
//
// The passes are those of the sparse least-squares f (bz_spmv.h) with K values behind every gathered index:
//   k_spmm_softmax_r  rows of A_f :  t_ik = sum_j a_ij x_jk, and on the K sums of a row the softmax: r_ik = w_i (p_ik - [k = b_i])
//                     -> R[i * K + k] (if kept) and the row's loss w_i ((mx - t_{i,b_i}) + log S)
//   k_spmm_glm_r<LOSS>  rows of A_f, the multi-response GLM f:  the same sums, and on each of them by itself the row loss of
//                     bz_spmv.h's k_spmv_glm_r<LOSS>: r_ik = w_i l'(b_ik, t_ik) -> R[i * K + k] (if kept) and the term w_i l(b_ik, t_ik)
//   k_spmm_t_algrad  rows of A_f', c = Identity:  (A_f' R)_jk, and on element j * K + k what k_algrad_elem does in its mode 1
//                     (sp_epilogue's SP_LS_T_ALGRAD on every class lane): the whole AL gradient in two launches, grad f never in HBM
//   k_spmm_t          rows of A_f':  A_f' R -> DFX (SP_T) for the forms that finish element-wise or in k_spmv_t_finish
//
// The lane map.  A (virtual) row is walked by a group of KP * L <= 64 lanes, KP the power of two >= K.  The CLASS is the fastest
// lane index (k = lane % KP, l = lane / KP): the gather of one entry's K values is one contiguous access of K elements (a full
// 64-byte line at K = 8 in fp64), and the loads of `col` / `val` have one address across the K class lanes, so the 12 bytes of
// an entry are read once for K products.  Lane (l, k) takes the entries l, l + L, ... in stored order and accumulates in T, four
// entries in flight, every load unconditional (an index past the row's end is clamped and the product dropped; a lane with
// k >= K is clamped to class K - 1 and its result dropped).  The L partial sums of a class are folded by a fixed xor tree in
// double over the lane offsets KP * L / 2 .. KP, as spmv_row's are; the max and the sum over a row's K classes are fixed xor
// trees over the offsets KP / 2 .. 1.  A row's value is a function of the stored order, K and L alone: no atomics, nothing that
// depends on the grid.
//
// Cut rows (sp_build's segments).  A segment leaves its K sums in `part` (K times the scalar kernels' side buffer:
// part[slot * K + k]); k_spmm_fold, one wave per cut row with the same class-fastest lane map (64 / KP lanes per class), adds a
// row's segment sums per class in a fixed order (lane l the segments l, l + 64 / KP, ..., then the xor tree) and runs the row's
// epilogue — for A_f the softmax across the K classes, or the multi-response GLM f's loss arm on each response lane.
//
// Included by bz_solver.hip alone, as bz_spmv.h is.
#pragma once
#include "bz_spmv.h"

namespace bz {

__device__ __forceinline__ float sp_log(float v) { return logf(v); }
__device__ __forceinline__ double sp_log(double v) { return log(v); }

// what a row's K sums go into: SPMM_SOFTMAX or SPMM_GLM_MODE0 + BZ_LOSS_* (rows of A_f), or sp_epilogue's SP_LS_T_ALGRAD / SP_T
// per element j * K + k (rows of A_f')
constexpr int SPMM_SOFTMAX = 100;
constexpr int SPMM_GLM_MODE0 = 101;  // the multi-response GLM f: K independent row losses, SPMM_GLM_MODE0 + BZ_LOSS_* (101 least
                                     // squares .. 105 Poisson), each sp_epilogue's loss arm on element i * K + k with row i's weight
constexpr bool spmm_glm_mode(int MODE) { return MODE >= SPMM_GLM_MODE0 && MODE <= SPMM_GLM_MODE0 + BZ_LOSS_POISSON; }

// the entries [s, e) of one row for class kc, this lane being entry lane l of the row's L: spmv_row with K values behind
// every column index.  Every lane of the row's group returns its class's folded sum.
template <class T, int KP, int L, bool NT>
__device__ __forceinline__ double spmm_row(const SpMat<T>& M, const T* __restrict__ g, int K, int64_t s, int64_t e, int l, int kc) {
    constexpr int U = 4;
    const int64_t last = e > 0 ? e - 1 : 0;
    T acc = T(0);
    for (int64_t i = s + l; i < e; i += (int64_t)U * L) {
        int32_t c[U];
        T a[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t ii = i + (int64_t)u * L;
            const int64_t ic = ii < e ? ii : last;
            c[u] = sp_ld<int32_t, NT>(M.col + ic);      // (one address across the row's class lanes)
            a[u] = sp_ld<T, NT>(M.val + ic);
        }
        T xv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) xv[u] = g[(int64_t)c[u] * K + kc];      // default policy; contiguous across the class lanes
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const T p = a[u] * xv[u];
            acc += (i + (int64_t)u * L < e) ? p : T(0);
        }
    }
    double d = (double)acc;
#pragma unroll
    for (int o = KP * L / 2; o >= KP; o >>= 1) d += __shfl_xor(d, o, 64);
    return d;
}

// The epilogue of row r on its K class sums; called by ALL lanes of the row's group (the softmax exchanges values between the
// class lanes), `lead` marking the one lane per class that writes (entry lane 0), k the lane's class (k >= K: an idle lane,
// which holds class K - 1's sum again).
//   SPMM_SOFTMAX: t_k = (T)d ; mx = max_k t_k and S = sum_k exp(t_k - mx) by xor trees over the class lanes (an idle lane's
//   copy of t_{K-1} cannot change the max; its e is dropped from S).  The max is an ordered compare, which drops a NaN — the
//   lanes may then disagree on mx — but the NaN lane's own e = exp(NaN - .) is NaN and the sum gives it to every lane: p, r and
//   the loss of the whole row are NaN.  The lane of class b_i adds the row's loss.
//   SPMM_GLM_MODE0 + LOSS: the K sums are K responses of their own.  The lead lane of response k < K runs sp_epilogue's loss arm
//   (its weighted mode SP_GLM_MODE0 + LOSS: the same operations in the same order, NaN kept by the ordered compares) on element
//   r * K + k of b and out, with the ROW's weight w[r]: out[r * K + k] = w l' (if kept), and w l goes to its acc[0].  Nothing is
//   exchanged between the response lanes; an idle lane (k >= K) writes nothing and adds nothing.
//   SP_LS_T_ALGRAD / SP_T: sp_epilogue on element r * K + k.
template <class T, int KP, int MODE>
__device__ __forceinline__ void spmm_epilogue(const SpEpi<T>& E, int K, int64_t r, double d, int k, bool lead, double (&acc)[1]) {
    if constexpr (MODE == SPMM_SOFTMAX) {
        const T t = (T)d;
        T mx = t;
#pragma unroll
        for (int o = KP / 2; o > 0; o >>= 1) {
            const T other = __shfl_xor(mx, o, 64);
            mx = other > mx ? other : mx;
        }
        const T ev = sp_exp(t - mx);
        T S = k < K ? ev : T(0);
#pragma unroll
        for (int o = KP / 2; o > 0; o >>= 1) S += __shfl_xor(S, o, 64);
        if (lead && k < K) {
            const T wv = E.w ? E.w[r] : E.w_uniform;
            const int bi = (int)E.b[r];                                  // (finite, integral and in [0, K): checked at creation)
            const bool mine = k == bi;
            if (E.out) E.out[r * K + k] = wv * (ev / S - (mine ? T(1) : T(0)));
            if (mine) acc[0] += (double)(wv * ((mx - t) + sp_log(S)));
        }
    } else if constexpr (spmm_glm_mode(MODE)) {
        if (lead && k < K) sp_epilogue<T, SP_GLM_MODE0 + (MODE - SPMM_GLM_MODE0)>(E, r * K + k, d, acc, r);
    } else {
        if (lead && k < K) sp_epilogue<T, MODE>(E, r * K + k, d, acc);
    }
}

// the row loop of the three passes: virtual row v belongs to the KP * L lanes (blockIdx.x * BLOCK + threadIdx.x) / (KP * L),
// then grid-strides
template <class T, int KP, int L, bool NT, int MODE>
__device__ __forceinline__ void spmm_rows(const SpMat<T>& M, const T* __restrict__ g, int K, const SpEpi<T>& E, double (&acc)[1]) {
    static_assert(KP >= 2 && KP * L <= 64 && (KP & (KP - 1)) == 0 && (L & (L - 1)) == 0, "a group of KP * L <= 64 lanes");
    constexpr int G = KP * L, RPB = BLOCK / G;
    const int sub = threadIdx.x % G;
    const int k = sub % KP, l = sub / KP;                // the class is the fastest lane index
    const int kc = k < K ? k : K - 1;
    for (int64_t v = (int64_t)blockIdx.x * RPB + threadIdx.x / G; v < M.nv; v += (int64_t)gridDim.x * RPB) {
        const int64_t s = M.ptr[v], e = M.ptr[v + 1];
        const double d = spmm_row<T, KP, L, NT>(M, g, K, s, e, l, kc);
        int64_t r = v;
        int pi = -1;
        if (M.vrow) { pi = M.vpart[v]; r = M.vrow[v]; }
        if (pi >= 0) {                                   // a segment of a cut row: k_spmm_fold finishes the row
            if (l == 0 && k < K) M.part[(int64_t)pi * K + k] = d;
        } else {
            spmm_epilogue<T, KP, MODE>(E, K, r, d, k, l == 0, acc);
        }
    }
}

// rows of A_f: R = w (softmax(A_f X) - onehot(b)) -> E.out (if kept) ; partials: slot0 the rows' losses
template <class T, int KP, int L, bool NT>
__global__ void __launch_bounds__(BLOCK)
k_spmm_softmax_r(SpMat<T> M, const T* __restrict__ x, int K, SpEpi<T> E, double* __restrict__ parts, int slot0) {
    double acc[1] = {0.0};
    spmm_rows<T, KP, L, NT, SPMM_SOFTMAX>(M, x, K, E, acc);
    block_reduce_store<1>(acc, 0u, parts, slot0);
}

// rows of A_f, the multi-response GLM f with the loss MODE - SPMM_GLM_MODE0: r_ik = w_i l'(b_ik, t_ik) -> E.out (if kept) ;
// partials: slot0 the terms w_i l(b_ik, t_ik)
template <class T, int KP, int L, bool NT, int MODE>
__global__ void __launch_bounds__(BLOCK)
k_spmm_glm_r(SpMat<T> M, const T* __restrict__ x, int K, SpEpi<T> E, double* __restrict__ parts, int slot0) {
    static_assert(spmm_glm_mode(MODE), "a K-wide GLM mode");
    double acc[1] = {0.0};
    spmm_rows<T, KP, L, NT, MODE>(M, x, K, E, acc);
    block_reduce_store<1>(acc, 0u, parts, slot0);
}

// rows of A_f', c = Identity: grad = A_f' R + yhat ; partials: slot0 the penalty terms
template <class T, int KP, int L, bool NT>
__global__ void __launch_bounds__(BLOCK)
k_spmm_t_algrad(SpMat<T> M, const T* __restrict__ r, int K, SpEpi<T> E, double* __restrict__ parts, int slot0) {
    double acc[1] = {0.0};
    spmm_rows<T, KP, L, NT, SP_LS_T_ALGRAD>(M, r, K, E, acc);
    block_reduce_store<1>(acc, 0u, parts, slot0);
}

// rows of A_f': E.out = A_f' R ; partials: slot0 zeros
template <class T, int KP, int L, bool NT>
__global__ void __launch_bounds__(BLOCK)
k_spmm_t(SpMat<T> M, const T* __restrict__ r, int K, SpEpi<T> E, double* __restrict__ parts, int slot0) {
    double acc[1] = {0.0};
    spmm_rows<T, KP, L, NT, SP_T>(M, r, K, E, acc);
    block_reduce_store<1>(acc, 0u, parts, slot0);
}

// the cut rows: one wave per row, lane (l, k) adds class k's segment sums l, l + 64 / KP, ... in order, the xor tree over the
// offsets 32 .. KP folds them, and the wave's first KP lanes run the row's epilogue; the block partials continue the slot
// behind the row kernel's (vb0).
template <class T, int KP, int MODE>
__global__ void __launch_bounds__(BLOCK)
k_spmm_fold(const double* __restrict__ part, const int32_t* __restrict__ crow, const int32_t* __restrict__ cptr, int ncut, int K,
            SpEpi<T> E, double* __restrict__ parts, int slot0, int vb0) {
    constexpr int LF = 64 / KP;
    const int lane = threadIdx.x & 63;
    const int k = lane % KP, l = lane / KP;
    const int kc = k < K ? k : K - 1;
    double acc[1] = {0.0};
    for (int j = blockIdx.x * WAVES + (threadIdx.x >> 6); j < ncut; j += gridDim.x * WAVES) {
        const int k1 = cptr[j + 1];
        double a = 0.0;
        for (int q = cptr[j] + l; q < k1; q += LF) a += part[(int64_t)q * K + kc];
#pragma unroll
        for (int o = 32; o >= KP; o >>= 1) a += __shfl_xor(a, o, 64);
        spmm_epilogue<T, KP, MODE>(E, K, (int64_t)crow[j], a, k, l == 0, acc);
    }
    block_reduce_store<1>(acc, 0u, parts, slot0, vb0 + (int)blockIdx.x);
}

// MODE -> the K-wide row kernel's entry point and its name, as sp_kernel and sp_kernel_name
template <class T, int KP, int L, bool NT, int MODE> constexpr auto spmm_kernel() {
    static_assert(MODE == SPMM_SOFTMAX || spmm_glm_mode(MODE) || MODE == SP_LS_T_ALGRAD || MODE == SP_T, "a mode of the K-wide row loop");
    if constexpr (MODE == SPMM_SOFTMAX) return &k_spmm_softmax_r<T, KP, L, NT>;
    else if constexpr (spmm_glm_mode(MODE)) return &k_spmm_glm_r<T, KP, L, NT, MODE>;
    else if constexpr (MODE == SP_LS_T_ALGRAD) return &k_spmm_t_algrad<T, KP, L, NT>;
    else return &k_spmm_t<T, KP, L, NT>;
}
constexpr const char* spmm_kernel_name(int MODE) {
    return MODE == SPMM_SOFTMAX ? "k_spmm_softmax_r" : spmm_glm_mode(MODE) ? "k_spmm_glm_r" : MODE == SP_LS_T_ALGRAD ? "k_spmm_t_algrad" : "k_spmm_t";
}

}  // namespace bz
