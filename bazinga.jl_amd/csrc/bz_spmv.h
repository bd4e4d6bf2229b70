// bz_spmv.h — the CSR row kernels: the sparse affine constraint c(x) = A x - b (BZ_C_SPARSE_AFFINE), the two passes of its AL
// gradient, the sparse quadratic f(x) = 0.5 x'Qx + q'x (BZ_F_SPARSE_QUADRATIC), the pass over Q, and the sparse least squares
// f(x) = 0.5 ||A_f x - b||^2 (BZ_F_SPARSE_LEAST_SQUARES), the passes over A_f and A_f', and the sparse logistic
// f(x) = sum_i log(1 + exp(-b_i a_i'x)) (BZ_F_SPARSE_LOGISTIC), the same two passes with another epilogue on the rows of A_f,
// and the sparse GLM f(x) = sum_i w_i l(b_i, a_i'x) (BZ_F_SPARSE_GLM): a row loss l with its derivative as r_i and a weight
// per row, one more epilogue per loss (weighted least squares and logistic, Huber, squared hinge, Poisson).
//
// A and A' are two CSR matrices in HBM (A' is built once, at bz_problem_create, by a stable counting sort).  Both passes
// are the same row kernel: L lanes (compile time, 1..64, chosen at creation from the mean row length) walk one row, lane
// l taking the entries l, l + L, l + 2L, ... in stored order and accumulating in T; the L lane sums are folded by a fixed
// xor tree carried in double.  A row's value is therefore a function of the stored order and of L alone: no atomics,
// nothing that depends on the grid or on timing.
//   k_spmv_yupd      rows of A :  c_i = sum a_ij x_j - b_i, and on that value what k_yupd does with it
//   k_spmv_t_finish  rows of A':  (A' yhat)_j, and on that value what k_gemv_t_finish does with it
//   k_spmv_q_algrad  rows of Q, c = Identity:  (Q x)_i, and on that value what k_algrad_elem does in its mode 2 — the whole
//                    AL gradient in one launch, on k_algrad_elem's grid and with its summation tree; Q x never goes to HBM
//   k_spmv_q         rows of Q:  Q x -> FR (and / or the f terms) for the forms that finish element-wise or in k_spmv_t_finish
// (Q is symmetric by the caller's contract: no transpose is built.)
//   k_spmv_ls_r         rows of A_f :  r_i = sum a_ij x_j - b_i -> R (if kept) and the terms r_i^2 (halved on the host)
//   k_spmv_ls_t_algrad  rows of A_f', c = Identity:  (A_f' r)_j = grad f_j, and on that value what k_algrad_elem does in its
//                       mode 1 — with k_spmv_ls_r the whole AL gradient in two launches; grad f never goes to HBM
//   k_spmv_ls_t         rows of A_f':  A_f' r -> DFX for the forms that finish element-wise or in k_spmv_t_finish
//   k_spmv_logit_r      rows of A_f, the logistic f:  r_i = -b_i sigma(-b_i a_i'x) -> R (if kept) and the terms
//                       softplus(-b_i a_i'x); the two kernels over A_f' then run on that r as they do on a residual
//   k_spmv_glm_r<LOSS>  rows of A_f, the GLM f:  r_i = w_i l'(b_i, a_i'x) -> R (if kept) and the terms w_i l(b_i, a_i'x), the
//                       loss a template argument (MODE SP_GLM_MODE0 + BZ_LOSS_*); the same two kernels over A_f' behind it
// Rows longer than S entries (S fixed at creation from the matrix alone) are cut into segments that run as rows of
// their own ("virtual rows": the row pointers refined at the cuts); a segment leaves its sum in a side buffer and
// k_spmv_fold, one wave per cut row, adds a row's segment sums in a fixed order and runs the row's epilogue.
// What a row's value goes into is the epilogue's MODE (SP_YUPD .. SP_GLM_MODE0 + BZ_LOSS_POISSON): sp_epilogue is its one body,
// with one arm for the row losses of every kind over A_f; sp_kernel / sp_kernel_name are the one map from a MODE to its entry
// point and its label.
//
// Kept apart from bz_kernels.h because only bz_solver.hip instantiates these templates: the sixteen family translation
// units do not see (or rebuild for) them.
#pragma once
#include <limits>
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

// what a row's value goes into: the epilogue's MODE.  (Plain ints, not an enum: a MODE is a template argument of k_spmv_fold,
// k_spmv_glm_r and k_spmm_fold, so its type is part of those kernels' names.)
constexpr int SP_YUPD = 0;           // rows of A: cx (if kept), yupd (if wanted: null = eval!(cx, c, x) alone) and the penalty term
constexpr int SP_T_FINISH = 1;       // rows of A': the gradient and the f term
constexpr int SP_Q_ALGRAD = 2;       // rows of Q, c = Identity: the gradient, the f term and the penalty term
constexpr int SP_Q = 3;              // rows of Q: Q x (if kept) and the f term (if x is given)
constexpr int SP_LS_R = 4;           // rows of A_f: the residual (if kept) and its square
constexpr int SP_LS_T_ALGRAD = 5;    // rows of A_f', c = Identity: the gradient and the penalty term
constexpr int SP_T = 6;              // rows of A_f': the product alone
constexpr int SP_LOGIT_R = 7;        // rows of A_f, logistic: the derivative of the row's loss (if kept) and the loss
constexpr int SP_GLM_MODE0 = 8;      // rows of A_f, the GLM f: the same for the weighted loss SP_GLM_MODE0 + BZ_LOSS_* (8 least
                                     // squares, 9 logistic, 10 Huber, 11 squared hinge, 12 Poisson)
constexpr int SP_NMODES = SP_GLM_MODE0 + BZ_LOSS_POISSON + 1;
template <class T> struct SpEpi {
    const T* b;              // SP_YUPD: b[ny] ; SP_LS_R and the GLM modes: b[m] of f ; SP_LOGIT_R: the labels b[m] of f
    T* cx;                   // SP_YUPD: c(x) for the caller that keeps it, or null
    T* out;                  // SP_YUPD: yupd[ny] or null ; SP_T_FINISH, SP_Q_ALGRAD, SP_LS_T_ALGRAD: grad[n] or null ;
                             // SP_Q: (Q x)[n] or null ; the modes over A_f: r[m] or null ; SP_T: (A_f' r)[n]
    const T* x;              // SP_T_FINISH, SP_Q_ALGRAD, SP_LS_T_ALGRAD: x[n] ; SP_Q: x[n], or null for the product alone
    ElemParams<T> P;
    const T* ext;            // SP_T_FINISH with the sparse quadratic f: (Q x)[n], left by k_spmv_q ; with a row-wise sparse
                             // f: (A_f' r)[n], left by k_spmv_ls_t
    const T* w;              // the GLM modes: the row weights w[m] (scale folded in), or null: w_uniform for every row
    T w_uniform;
    T delta;                 // SP_GLM_MODE0 + BZ_LOSS_HUBER: Huber's delta
};

// scalars a mode leaves per row: SP_Q_ALGRAD the f term and the penalty term, the others (over A_f: the loss) one
template <int MODE> constexpr int sp_nacc() { return MODE == SP_Q_ALGRAD ? 2 : 1; }

// exp and log1p in T: an fp32 problem takes the fp32 functions
__device__ __forceinline__ float sp_exp(float v) { return expf(v); }
__device__ __forceinline__ double sp_exp(double v) { return exp(v); }
__device__ __forceinline__ float sp_log1p(float v) { return log1pf(v); }
__device__ __forceinline__ double sp_log1p(double v) { return log1p(v); }

// (called by the row's first lane alone; every arm is written into this one body and none behind a call: the inlined form of a
// helper gives the same instructions in another order, and the kernels are kept instruction for instruction.  The per-row
// parameters are loaded once per row.  `rw`: the row the weight is taken from where it is not r — the K-wide loss modes of
// bz_spmm.h, whose element r = i * K + k of b and out shares row i's weight; every other caller leaves it out.)
template <class T, int MODE>
__device__ __forceinline__ void sp_epilogue(const SpEpi<T>& E, int64_t r, double d, double (&acc)[sp_nacc<MODE>()], int64_t rw = -1) {
    const ElemParams<T>& P = E.P;
    if constexpr (MODE == SP_YUPD) {
        const T c = (T)d - E.b[r];                                  // eval!(cx, c, x)
        if (E.cx) E.cx[r] = c;
        if (!E.out) return;
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
        acc[0] += (double)pterm;
    } else if constexpr (MODE == SP_T_FINISH) {
        // dlx = dfx + jtv ; f element-wise (Zero | DiagQuadratic)               (k_gemv_t_finish)
        // or the sparse quadratic from ext = Q x, P.b = q                      (k_gemv_t_finish_ext, fext 2)
        T dfx = T(0), fterm = T(0);
        if (P.f_kind == BZ_F_DIAG_QUADRATIC) {
            const T xv = E.x[r];
            const T qx = P.q[r] * xv;
            dfx = qx - P.b[r];
            fterm = xv * (T(0.5) * qx - P.b[r]);
        } else if (P.f_kind == BZ_F_SPARSE_QUADRATIC) {
            const T xv = E.x[r], e = E.ext[r], qv = P.b[r];
            dfx = e + qv;
            fterm = xv * (T(0.5) * e + qv);
        } else if (P.f_kind == BZ_F_SPARSE_LEAST_SQUARES || P.f_kind == BZ_F_SPARSE_LOGISTIC || P.f_kind == BZ_F_SPARSE_GLM ||
                   P.f_kind == BZ_F_SPARSE_MULTINOMIAL || P.f_kind == BZ_F_SPARSE_MULTI_GLM) {
            dfx = E.ext[r];                                             // (k_gemv_t_finish_ext, fext 1: f's value comes from k_spmv_ls_r / k_spmv_logit_r / k_spmv_glm_r / k_spmm_softmax_r / k_spmm_glm_r)
        }
        if (E.out) E.out[r] = dfx + (T)d;
        acc[0] += (double)fterm;
    } else if constexpr (MODE == SP_Q_ALGRAD || MODE == SP_LS_T_ALGRAD) {
        // element r of k_algrad_elem with ext[r] = d, in its mode 2 (rows of Q: with the f term from q = P.b) or its mode 1 (rows
        // of A_f': without): the same operations in the same order (never launched with a pairwise D, whose projection needs
        // the partner element)
        const T xv = E.x[r];
        [[maybe_unused]] T qv = T(0);
        if constexpr (MODE == SP_Q_ALGRAD) qv = P.b[r];
        const T e = (T)d;
        const T mu = P.uni >= 1 ? P.mu_uniform : P.mu[r];
        const T muy = P.uni >= 2 ? T(0) : P.muy[r];
        const T lo = P.D_lo_vec ? P.D_lo_vec[r] : P.D_lo;
        const T hi = P.D_hi_vec ? P.D_hi_vec[r] : P.D_hi;
        const ALOut<T> o = al_elem(BZ_F_ZERO, P.D_kind, xv, T(0), T(0), mu, muy, lo, hi);
        if constexpr (MODE == SP_Q_ALGRAD) {
            const T dfx = e + qv;
            const T fterm = xv * (T(0.5) * e + qv);
            if (E.out) E.out[r] = dfx + o.grad;
            acc[0] += (double)fterm;
            acc[1] += (double)o.pterm;
        } else {
            if (E.out) E.out[r] = e + o.grad;
            acc[0] += (double)o.pterm;
        }
    } else if constexpr (MODE == SP_Q) {
        const T e = (T)d;
        if (E.out) E.out[r] = e;
        if (E.x) acc[0] += (double)(E.x[r] * (T(0.5) * e + P.b[r]));            // k_fvalue_elem with ext
    } else if constexpr (MODE == SP_LS_R || MODE == SP_LOGIT_R || MODE >= SP_GLM_MODE0) {
        // rows of A_f: the row's term w l(b, t) and r = w l'(b, t), t = a_i'x, the loss fixed at compile time.  The plain
        // least-squares and logistic kinds (W false) are the same losses without the weight: no load and no product for it.
        // The weight: one pointer test and one load, as mu has it; every branch below is a select on values already at hand.
        // Ordered compares and arithmetic alone (no fmax / fmin, which drop a NaN): a NaN in t makes every compare false and
        // reaches both the loss and r.
        constexpr bool W = MODE >= SP_GLM_MODE0;
        constexpr int LOSS = W ? MODE - SP_GLM_MODE0 : MODE == SP_LS_R ? BZ_LOSS_LEAST_SQUARES : BZ_LOSS_LOGISTIC;
        [[maybe_unused]] T wv = T(1);
        if constexpr (W) wv = E.w ? E.w[rw >= 0 ? rw : r] : E.w_uniform;
        const T bv = E.b[r];
        const T t = (T)d;
        T loss, dl;
        if constexpr (LOSS == BZ_LOSS_LEAST_SQUARES) {
            const T v = t - bv;                                     // r = A_f x - b ; sum w v^2, halved on the host (fscale)
            loss = v * v;
            dl = v;
        } else if constexpr (LOSS == BZ_LOSS_LOGISTIC) {
            // u = b_i a_i'x ; loss = softplus(-u), dl = -b_i sigma(-u), both from e = exp(-|u|) in [0, 1]: nothing overflows and
            // nothing cancels
            const T u = bv * t;
            const T e = sp_exp(u < T(0) ? u : -u);
            loss = (u < T(0) ? -u : T(0)) + sp_log1p(e);
            const T s = u >= T(0) ? e / (T(1) + e) : T(1) / (T(1) + e);
            dl = -bv * s;
        } else if constexpr (LOSS == BZ_LOSS_HUBER) {
            const T v = t - bv, dlt = E.delta;
            const T a = v < T(0) ? -v : v;
            const bool inside = a <= dlt;
            loss = inside ? T(0.5) * v * v : dlt * (a - T(0.5) * dlt);
            dl = inside ? v : (v > T(0) ? dlt : (v < T(0) ? -dlt : v));      // (only a NaN takes the last arm)
        } else if constexpr (LOSS == BZ_LOSS_SQUARED_HINGE) {
            const T h = T(1) - bv * t;
            const bool off = h <= T(0);
            loss = off ? T(0) : T(0.5) * h * h;
            dl = off ? T(0) : -bv * h;
        } else {
            // Poisson, log link: e - b t without the constant log b!.  Where e has overflowed (fp32: t beyond 88.7) the loss is
            // +inf, not inf - inf; b = 0 drops the product, so that t = -inf gives 0 and not 0 * inf.
            const T e = sp_exp(t);
            const T bt = bv == T(0) ? T(0) : bv * t;
            loss = e < std::numeric_limits<T>::infinity() ? e - bt : e;
            dl = e - bv;
        }
        if constexpr (W) {
            if (E.out) E.out[r] = wv * dl;
            acc[0] += (double)(wv * loss);
        } else {
            if (E.out) E.out[r] = dl;
            acc[0] += (double)loss;
        }
    } else {
        if (E.out) E.out[r] = (T)d;
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
// then grid-strides.  Adds this thread's share of the pass's scalars to acc (the row's first lane carries the row's terms).
template <class T, int L, bool NT, int MODE>
__device__ __forceinline__ void spmv_rows(const SpMat<T>& M, const T* __restrict__ g, const SpEpi<T>& E,
                                          double (&acc)[sp_nacc<MODE>()]) {
    constexpr int RPB = BLOCK / L;
    const int sub = threadIdx.x % L;
    for (int64_t v = (int64_t)blockIdx.x * RPB + threadIdx.x / L; v < M.nv; v += (int64_t)gridDim.x * RPB) {
        const int64_t s = M.ptr[v], e = M.ptr[v + 1];
        const double d = spmv_row<T, L, NT>(M, g, s, e, sub);
        if (sub == 0) {
            int64_t r = v;
            int pi = -1;
            if (M.vrow) { pi = M.vpart[v]; r = M.vrow[v]; }
            if (pi >= 0) M.part[pi] = d;      // a segment of a cut row: k_spmv_fold finishes the row
            else sp_epilogue<T, MODE>(E, r, d, acc);
        }
    }
}

template <class T, int L, bool NT>
__global__ void __launch_bounds__(BLOCK)
k_spmv_yupd(SpMat<T> M, const T* __restrict__ x, SpEpi<T> E, double* __restrict__ parts, int slot0) {
    double acc[1] = {0.0};
    spmv_rows<T, L, NT, SP_YUPD>(M, x, E, acc);
    block_reduce_store<1>(acc, 0u, parts, slot0);
}

template <class T, int L, bool NT>
__global__ void __launch_bounds__(BLOCK)
k_spmv_t_finish(SpMat<T> M, const T* __restrict__ yupd, SpEpi<T> E, double* __restrict__ parts, int slot0) {
    double acc[1] = {0.0};
    spmv_rows<T, L, NT, SP_T_FINISH>(M, yupd, E, acc);
    block_reduce_store<1>(acc, 0u, parts, slot0);
}

// what k_spmv_q_algrad needs beside the entries: the rows as the caller gave them (not the virtual rows) and the cut rows
struct SpRows {
    const int64_t* rowptr;   // [n + 1]
    const int32_t* crow;     // [ncut] the cut rows, ascending
    const int32_t* cptr;     // [ncut + 1] where a cut row's segment sums start in `part`
    int ncut;
    int64_t S;               // segment length
    int64_t n;
};

// rows of Q, c = Identity: grad = (Q x + q) + yhat ; partials: slot0 the f terms, slot0 + 1 the penalty terms.
// The gradient AND the two scalars are bit for bit those of k_spmv_q followed by k_algrad_elem in its mode 2, so the
// kernel is launched on k_algrad_elem's grid and keeps that kernel's summation tree: a workgroup owns the elements
// k_algrad_elem's workgroup of the same number owns — tiles of BLOCK packs, tile k of workgroup b starting at pack
// (b + k gridDim.x) BLOCK.  The L-lane groups walk the tile's rows (spmv_row: the row sums of the product kernel), each
// row's first lane runs the row's epilogue and leaves the row's two terms in LDS; then thread t adds the terms of ITS pack
// in element order, as k_algrad_elem's thread t does, and block_reduce_store<2> does the rest.
// A cut row is summed as the product kernel and k_spmv_fold sum it: its segments by the L-lane groups of the whole
// workgroup (spmv_row per segment, the sums into `part`), then one wave adds the segment sums (lane l the sums l, l + 64,
// ..., the fixed xor tree) and runs the epilogue.  No second launch, no exchange between workgroups.
template <class T, int L, bool NT>
__global__ void __launch_bounds__(BLOCK)
k_spmv_q_algrad(SpMat<T> M, SpRows R, const T* __restrict__ x, SpEpi<T> E, double* __restrict__ parts, int slot0) {
    constexpr int N = PackN<T>::N, TILE = BLOCK * N, RPB = BLOCK / L;
    __shared__ double shf[TILE], shp[TILE];
    const int sub = threadIdx.x % L, grp = threadIdx.x / L, lane = threadIdx.x & 63;
    const int64_t n = R.n, npacks = (n + N - 1) / N;
    double acc[2] = {0.0, 0.0};
    for (int64_t c0 = (int64_t)blockIdx.x * BLOCK; c0 < npacks; c0 += (int64_t)gridDim.x * BLOCK) {
        const int64_t i0 = c0 * N;
        const int64_t iend = i0 + TILE < n ? i0 + TILE : n;
        for (int it = 0; it < N * L; ++it) {
            const int lr = it * RPB + grp;
            const int64_t r = i0 + lr;
            const int64_t rc = r < n ? r : n - 1;                 // (unconditional loads; the row is dropped below)
            const int64_t s = R.rowptr[rc];
            int64_t e = R.rowptr[rc + 1];
            const bool whole = r < n && !(R.ncut && e - s > R.S);
            if (!whole) e = s;
            const double d = spmv_row<T, L, NT>(M, x, s, e, sub);
            if (sub == 0 && whole) {
                double t2[2] = {0.0, 0.0};
                sp_epilogue<T, SP_Q_ALGRAD>(E, r, d, t2);
                shf[lr] = t2[0]; shp[lr] = t2[1];
            }
        }
        if (R.ncut) {
            int j = 0;
            for (int hi = R.ncut; j < hi;) {                      // the first cut row at or behind i0
                const int mid = (j + hi) >> 1;
                if ((int64_t)R.crow[mid] < i0) j = mid + 1; else hi = mid;
            }
            for (; j < R.ncut && (int64_t)R.crow[j] < iend; ++j) {
                const int64_t r = R.crow[j];
                const int64_t s = R.rowptr[r], e = R.rowptr[r + 1];
                const int k0 = R.cptr[j], k1 = R.cptr[j + 1];
                for (int k = grp; k < k1 - k0; k += RPB) {
                    const int64_t ss = s + (int64_t)k * R.S;
                    const int64_t ee = ss + R.S < e ? ss + R.S : e;
                    const double d = spmv_row<T, L, NT>(M, x, ss, ee, sub);
                    if (sub == 0) M.part[k0 + k] = d;
                }
                __syncthreads();                                  // (the segment sums of this row are in `part`)
                if (threadIdx.x < 64) {
                    double a = 0.0;
                    for (int k = k0 + lane; k < k1; k += 64) a += M.part[k];
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
                    if (lane == 0) {
                        double t2[2] = {0.0, 0.0};
                        sp_epilogue<T, SP_Q_ALGRAD>(E, r, a, t2);
                        shf[r - i0] = t2[0]; shp[r - i0] = t2[1];
                    }
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const int at = (int)threadIdx.x * N + e;
            if (i0 + at < n) { acc[0] += shf[at]; acc[1] += shp[at]; }
        }
        __syncthreads();
    }
    block_reduce_store<2>(acc, 0u, parts, slot0);
}

// rows of Q: E.out = Q x (if kept) ; partials: slot0 the f terms (zeros when E.x is null)
template <class T, int L, bool NT>
__global__ void __launch_bounds__(BLOCK)
k_spmv_q(SpMat<T> M, const T* __restrict__ x, SpEpi<T> E, double* __restrict__ parts, int slot0) {
    double acc[1] = {0.0};
    spmv_rows<T, L, NT, SP_Q>(M, x, E, acc);
    block_reduce_store<1>(acc, 0u, parts, slot0);
}

// rows of A_f: r = A_f x - b -> E.out (if kept) ; partials: slot0 the terms r_i^2
template <class T, int L, bool NT>
__global__ void __launch_bounds__(BLOCK)
k_spmv_ls_r(SpMat<T> M, const T* __restrict__ x, SpEpi<T> E, double* __restrict__ parts, int slot0) {
    double acc[1] = {0.0};
    spmv_rows<T, L, NT, SP_LS_R>(M, x, E, acc);
    block_reduce_store<1>(acc, 0u, parts, slot0);
}

// rows of A_f, the logistic f: r_i = -b_i sigma(-b_i a_i'x) -> E.out (if kept) ; partials: slot0 the terms softplus(-b_i a_i'x)
template <class T, int L, bool NT>
__global__ void __launch_bounds__(BLOCK)
k_spmv_logit_r(SpMat<T> M, const T* __restrict__ x, SpEpi<T> E, double* __restrict__ parts, int slot0) {
    double acc[1] = {0.0};
    spmv_rows<T, L, NT, SP_LOGIT_R>(M, x, E, acc);
    block_reduce_store<1>(acc, 0u, parts, slot0);
}

// rows of A_f, the GLM f with the loss MODE - SP_GLM_MODE0: r_i = w_i l'(b_i, a_i'x) -> E.out (if kept) ; partials: slot0 the
// terms w_i l(b_i, a_i'x)
template <class T, int L, bool NT, int MODE>
__global__ void __launch_bounds__(BLOCK)
k_spmv_glm_r(SpMat<T> M, const T* __restrict__ x, SpEpi<T> E, double* __restrict__ parts, int slot0) {
    static_assert(MODE >= SP_GLM_MODE0 && MODE <= SP_GLM_MODE0 + BZ_LOSS_POISSON, "a GLM mode");
    double acc[1] = {0.0};
    spmv_rows<T, L, NT, MODE>(M, x, E, acc);
    block_reduce_store<1>(acc, 0u, parts, slot0);
}

// rows of A_f', c = Identity: grad = A_f' r + yhat ; partials: slot0 the penalty terms
template <class T, int L, bool NT>
__global__ void __launch_bounds__(BLOCK)
k_spmv_ls_t_algrad(SpMat<T> M, const T* __restrict__ r, SpEpi<T> E, double* __restrict__ parts, int slot0) {
    double acc[1] = {0.0};
    spmv_rows<T, L, NT, SP_LS_T_ALGRAD>(M, r, E, acc);
    block_reduce_store<1>(acc, 0u, parts, slot0);
}

// rows of A_f': E.out = A_f' r ; partials: slot0 zeros
template <class T, int L, bool NT>
__global__ void __launch_bounds__(BLOCK)
k_spmv_ls_t(SpMat<T> M, const T* __restrict__ r, SpEpi<T> E, double* __restrict__ parts, int slot0) {
    double acc[1] = {0.0};
    spmv_rows<T, L, NT, SP_T>(M, r, E, acc);
    block_reduce_store<1>(acc, 0u, parts, slot0);
}

// the cut rows: one wave per row adds the row's segment sums (lane l the sums l, l + 64, ... in order, then the fixed
// xor tree) and runs the row's epilogue; its block partials continue the slot (SP_Q_ALGRAD: the two slots) behind the row
// kernel's (vb0).
template <class T, int MODE>
__global__ void __launch_bounds__(BLOCK)
k_spmv_fold(const double* __restrict__ part, const int32_t* __restrict__ crow, const int32_t* __restrict__ cptr, int ncut,
            SpEpi<T> E, double* __restrict__ parts, int slot0, int vb0) {
    const int lane = threadIdx.x & 63;
    constexpr int K = sp_nacc<MODE>();
    double acc[K] = {};
    for (int j = blockIdx.x * WAVES + (threadIdx.x >> 6); j < ncut; j += gridDim.x * WAVES) {
        const int k1 = cptr[j + 1];
        double a = 0.0;
        for (int k = cptr[j] + lane; k < k1; k += 64) a += part[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if (lane == 0) sp_epilogue<T, MODE>(E, crow[j], a, acc);
    }
    block_reduce_store<K>(acc, 0u, parts, slot0, vb0 + (int)blockIdx.x);
}

// MODE -> the row kernel's entry point, and its name as the profile labels spell it.  (k_spmv_q_algrad takes the rows as given
// beside the matrix: another signature, launched by name.)
template <class T, int L, bool NT, int MODE> constexpr auto sp_kernel() {
    static_assert(MODE >= 0 && MODE < SP_NMODES && MODE != SP_Q_ALGRAD, "a mode of the row loop");
    if constexpr (MODE == SP_YUPD) return &k_spmv_yupd<T, L, NT>;
    else if constexpr (MODE == SP_T_FINISH) return &k_spmv_t_finish<T, L, NT>;
    else if constexpr (MODE == SP_Q) return &k_spmv_q<T, L, NT>;
    else if constexpr (MODE == SP_LS_R) return &k_spmv_ls_r<T, L, NT>;
    else if constexpr (MODE == SP_LS_T_ALGRAD) return &k_spmv_ls_t_algrad<T, L, NT>;
    else if constexpr (MODE == SP_T) return &k_spmv_ls_t<T, L, NT>;
    else if constexpr (MODE == SP_LOGIT_R) return &k_spmv_logit_r<T, L, NT>;
    else return &k_spmv_glm_r<T, L, NT, MODE>;
}
constexpr const char* sp_kernel_name(int MODE) {
    constexpr const char* names[] = {"k_spmv_yupd", "k_spmv_t_finish", "k_spmv_q_algrad", "k_spmv_q",
                                     "k_spmv_ls_r", "k_spmv_ls_t_algrad", "k_spmv_ls_t", "k_spmv_logit_r"};
    return MODE < SP_GLM_MODE0 ? names[MODE] : "k_spmv_glm_r";
}

}  // namespace bz
