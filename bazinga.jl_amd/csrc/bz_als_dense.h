// bz_als_dense.h — the slack (ALS) form with a dense affine constraint c(x) = A x - b, and a dense f beside a dense c.
//
// With c = Identity the lifted vector xs = [x; s] has two halves of one length and every slack kernel of bz_kernels.h
// walks one index over both.  With c(x) = A x - b the halves have unrelated lengths: x has nx elements (a whole number
// of 16-byte packs, so that s starts aligned), s has ny (any number, the last pack may be ragged).  What indexes which
// half: q, b and g's per-element vectors the x half; mu, mu*y, y and D's vector bounds the s half.
//   k_algrad_slack_rows       the ny-length part of gradient!(dFxs, F::AugLagFunSlack, xs) between the two passes over A
//   k_gemv_t_finish_ext       dFxs[1:nx] = dfx + A' yupd with dfx of a dense f (LeastSquares, Quadratic)
//   k_fbstep_lifted           prox!(z, G::NonsmoothCostFunSlack, xs, gamma) after the forward step, one launch
//   k_dual_update_slack_rows  als.jl:82-87 on c(x) = A x - b
//
// Kept apart from bz_kernels.h because only bz_solver.hip instantiates these templates: the sixteen family translation
// units do not see (or rebuild for) them.
#pragma once
#include "bz_kernels.h"

namespace bz {

// gradient!(dFxs, F::AugLagFunSlack, xs)  (auglagfunslack.jl:78-97), rows of a dense c, cx = A x - b given:
//   w = (cx + muy) - s ; slot +0 sum w^2/mu     (:89, summed then halved on the host)
//   yupd = y + (cx - s)/mu                      (:92)   -> yupd (the operand of A' yupd, :93)
//   dFxs[nx + i] = -yupd                        (:95)   -> gs, in the same pass
// The operations and their order are k_algrad_slack_elem's (c = Identity), with cx read instead of x.
template <class T>
__global__ void __launch_bounds__(BLOCK)
k_algrad_slack_rows(const T* __restrict__ cx, const T* __restrict__ s, const T* __restrict__ mu,
                    const T* __restrict__ muy, const T* __restrict__ yv, T* __restrict__ yupd,
                    T* __restrict__ gs, int64_t ny, double* __restrict__ parts, int slot0) {
    double acc[1] = {0.0};
    bz_for_chunks<T>(ny, [&](const int64_t i0, const auto cnt_) {
        const int cnt = cnt_;      // compile-time PackN in the main loop, run-time only for the ragged last chunk
        Pack<T> pc = ld(cx, i0, cnt), ps = ld(s, i0, cnt), pmu = ld(mu, i0, cnt), pmuy = ld(muy, i0, cnt);
        Pack<T> py = ld(yv, i0, cnt), pu, pg;
#pragma unroll
        for (int e = 0; e < PackN<T>::N; ++e) {
            const T c = pc.v[e], sv = ps.v[e];
            T w = c + pmuy.v[e];
            w = w - sv;
            const T pterm = (w * w) / pmu.v[e];
            const T r = c - sv;
            const T yu = py.v[e] + r / pmu.v[e];
            pu.v[e] = yu;
            pg.v[e] = -yu;
            if (e < cnt) acc[0] += (double)pterm;
        }
        st(yupd, i0, cnt, pu);
        if (gs) st(gs, i0, cnt, pg);
    });
    block_reduce_store<1>(acc, 0u, parts, slot0);
}

// dlx = dfx + jtv with jtv = sum over row chunks (gemv_t_fold, the fold k_gemv_t_finish uses) and dfx of a dense f, which the
// products with f's own matrix have left in `ext` (dense_f_eval) — k_algrad_elem's modes:
//   fext 1 (LeastSquares): dfx = ext[i] = (A_f' r)_i ; the f value <r, r> has its slot already: nothing is written to slot0
//   fext 2 (Quadratic):    ext = Q x ; dfx = ext + q (P.b holds q) ; slot +0: sum x (0.5 ext + q)
template <class T>
__global__ void __launch_bounds__(BLOCK)
k_gemv_t_finish_ext(const T* __restrict__ part, int nchunks, int64_t pstride, const T* __restrict__ x,
                    ElemParams<T> P, int fext, const T* __restrict__ ext, T* __restrict__ grad, int64_t n,
                    double* __restrict__ parts, int slot0) {
    double acc[1] = {0.0};
    bz_for_chunks<T>(n, [&](const int64_t i0, const auto cnt_) {
        const int cnt = cnt_;      // compile-time PackN in the main loop, run-time only for the ragged last chunk
        const Pack<T> j = gemv_t_fold(part, nchunks, pstride, i0, cnt);      // (k_gemv_t_finish's fold: one copy)
        Pack<T> px = ld(x, i0, cnt), pe = ld(ext, i0, cnt), pg;
        Pack<T> pq = (fext == 2) ? ld(P.b, i0, cnt) : splat(T(0));
#pragma unroll
        for (int e = 0; e < PackN<T>::N; ++e) {
            T dfx = pe.v[e], fterm = T(0);
            if (fext == 2) {
                dfx = pe.v[e] + pq.v[e];
                fterm = px.v[e] * (T(0.5) * pe.v[e] + pq.v[e]);
            }
            pg.v[e] = dfx + j.v[e];
            if (e < cnt) acc[0] += (double)fterm;
        }
        if (grad) st(grad, i0, cnt, pg);
    });
    if (fext == 2) block_reduce_store<1>(acc, 0u, parts, slot0);
}

// prox!(z, G::NonsmoothCostFunSlack, xs, gamma)  (auglagfunslack.jl:136-154) after the forward step, on halves of
// unequal length, in one launch: workgroups 0 .. gx - 1 play a grid of gx over the x half,
//   z_x = prox_g(x - gamma g_x)   (:147-148),
// workgroups gx .. gx + gs - 1 a grid of gs over the s half,
//   z_s = proj_D(s - gamma g_s)   (:151-152),
// and res = xs - z on both.  Every workgroup leaves one partial per slot at its own number, so the sums are folded in
// workgroup order; gx and gs are functions of (nx, ny) alone (Solver::lifted_sections): the same bits on every run.
//   slots: +0 sum g terms (x half; the s workgroups leave 0), +1 <g, res>, +2 ||res||^2 (both halves)
//   g == nullptr: the prox of xs itself
template <class T, bool LP = false>
__global__ void __launch_bounds__(BLOCK)
k_fbstep_lifted(const T* __restrict__ xs, const T* __restrict__ g, T gamma, ElemParams<T> P,
                T* __restrict__ z, T* __restrict__ res, int64_t nx, int64_t ny, int gx, int gs,
                double* __restrict__ parts, int slot0) {
    double acc[3] = {0.0, 0.0, 0.0};
    if ((int)blockIdx.x < gx) {
        const T gl = gamma * P.g_lambda;
        bz_for_chunks_v<T>(nx, (int)blockIdx.x, gx, [&](const int64_t i0, const auto cnt_) {
            const int cnt = cnt_;      // (nx is whole packs: always the compile-time PackN)
            ElemLoads<T> L;
            load_params(P, i0, cnt, L, false, false, true);
            Pack<T> px = ld(xs, i0, cnt);
            Pack<T> pg = g ? ld(g, i0, cnt) : splat(T(0));
            Pack<T> pz, pr;
#pragma unroll
            for (int e = 0; e < PackN<T>::N; ++e) {
                T y = px.v[e];
                if (g) { T t = gamma * pg.v[e]; y = px.v[e] - t; }
                T gterm;
                const T a = prox_elem<T, LP>(P.g_kind, y, gl_elem(P, L, e, gamma, gl), L.gu.v[e], L.glo.v[e], L.ghi.v[e], gterm, P.g_p);
                gterm = gterm_elem(P, L, e, gterm);
                const T r = px.v[e] - a;
                pz.v[e] = a; pr.v[e] = r;
                if (e < cnt) {
                    acc[0] += (double)gterm;
                    acc[1] += (double)(pg.v[e] * r);
                    acc[2] += (double)(r * r);
                }
            }
            st(z, i0, cnt, pz);
            if (res) st(res, i0, cnt, pr);
        });
    } else {
        const T* s = xs + nx;
        const T* gsv = g ? g + nx : nullptr;
        T* zs = z + nx;
        T* rs = res ? res + nx : nullptr;
        bz_for_chunks_v<T>(ny, (int)blockIdx.x - gx, gs, [&](const int64_t i0, const auto cnt_) {
            const int cnt = cnt_;      // compile-time PackN in the main loop, run-time only for the ragged last chunk
            Pack<T> dlo = P.D_lo_vec ? ld(P.D_lo_vec, i0, cnt) : splat(P.D_lo);
            Pack<T> dhi = P.D_hi_vec ? ld(P.D_hi_vec, i0, cnt) : splat(P.D_hi);
            Pack<T> ps = ld(s, i0, cnt);
            Pack<T> pg = gsv ? ld(gsv, i0, cnt) : splat(T(0));
            Pack<T> pz, pr;
#pragma unroll
            for (int e = 0; e < PackN<T>::N; ++e) {
                T y = ps.v[e];
                if (gsv) { T u = gamma * pg.v[e]; y = ps.v[e] - u; }
                const T b = proj_D(P.D_kind, y, dlo.v[e], dhi.v[e]);
                const T r = ps.v[e] - b;
                pz.v[e] = b; pr.v[e] = r;
                if (e < cnt) {
                    acc[1] += (double)(pg.v[e] * r);
                    acc[2] += (double)(r * r);
                }
            }
            st(zs, i0, cnt, pz);
            if (rs) st(rs, i0, cnt, pr);
        });
    }
    block_reduce_store<3>(acc, 0u, parts, slot0);
}

// ALS dual update (als.jl:82-87) with cx = A x - b at the subsolver's solution: y += (cx - s)/mu ; slot +0 max |cx - s|
// (k_dual_update_slack's operations, with cx read instead of x)
template <class T>
__global__ void __launch_bounds__(BLOCK)
k_dual_update_slack_rows(const T* __restrict__ cx, const T* __restrict__ s, const T* __restrict__ mu,
                         T* __restrict__ y, int64_t ny, double* __restrict__ parts, int slot0) {
    double acc[1] = {0.0};
    bz_for_chunks<T>(ny, [&](const int64_t i0, const auto cnt_) {
        const int cnt = cnt_;      // compile-time PackN in the main loop, run-time only for the ragged last chunk
        Pack<T> pc = ld(cx, i0, cnt), ps = ld(s, i0, cnt), pm = ld(mu, i0, cnt), py = ld((const T*)y, i0, cnt);
#pragma unroll
        for (int e = 0; e < PackN<T>::N; ++e) {
            const T r = pc.v[e] - ps.v[e];
            py.v[e] = py.v[e] + r / pm.v[e];
            if (e < cnt) acc[0] = nanmax(acc[0], (double)(r < T(0) ? -r : r));
        }
        st(y, i0, cnt, py);
    });
    block_reduce_store<1>(acc, 1u, parts, slot0);
}

}  // namespace bz
