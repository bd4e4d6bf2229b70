// bz_group.h — the forward-backward step of the group Lasso g (BZ_G_NORM_L21):
//   g(x) = sum_j lambda_j ||x[jK : (j+1)K]||_2 over the n / K contiguous groups of K elements, 1 <= K <= 64.
//
// k_fbstep_group has k_fbstep's contract (y = x - gamma * g ; z = prox(y) ; res = x - z ; g == nullptr: the pure prox of x ;
// res may be null ; slots +0 the g terms, +1 <g, res>, +2 ||res||^2), with a prox that couples the K elements of a group:
//   q_k = y_k * y_k ; s = sum_k q_k ; nrm = sqrt(s) ; gl = gamma * lambda_j
//   nrm <= gl: z = 0 (scal = 0) ; nrm > gl: scal = 1 - gl / nrm ; otherwise (a NaN): scal = nrm - gl ; z_k = scal * y_k
//   the group's term of g(z): scal * nrm (times lambda_j here with a vector lambda, on the host with a number)
// all in T.  The sum s is the fixed xor tree over the lane offsets KP / 2 .. 1, KP the power of two >= K, with zeros in the
// lanes k >= K: a function of K alone, which a host loop (`q[:o] + q[o:]` for o = KP / 2 .. 1) reproduces bit for bit.
//
// The lane map is the one of the K-wide row kernels (bz_spmm.h).  A group is walked by KP adjacent lanes, k = lane % KP, one
// element per lane: with K == KP a wave's access is one contiguous run of 64 elements.  A wave holds 64 / KP groups, a
// workgroup BLOCK / KP; the grid strides over the groups.  Every load is unconditional: a lane with k >= K is clamped to
// element K - 1 of its group and a group index past the end to the last group — what such a lane computes is dropped (its
// square, its store, its sums).  One lane per group (k = 0) loads lambda_j and adds the group's g term.
//
// Included by bz_solver.hip alone, as bz_spmm.h is.
#pragma once
#include "bz_kernels.h"

namespace bz {

template <class V, bool NT>
__device__ __forceinline__ V grp_ld(const V* __restrict__ p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// the correctly rounded square root of the problem's type (sqrtf is the refined sequence here; __fsqrt_rn, which sqrt_rn(float) of
// bz_kernels.h calls, is the hardware's approximate v_sqrt_f32 and would not give the host's bits)
__device__ __forceinline__ float grp_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double grp_sqrt(double v) { return sqrt(v); }

// the most workgroups a launch over `ngroups` groups takes (one partial per workgroup and slot: PSTRIDE at the most)
inline int group_grid(int64_t ngroups, int KP) {
    const int64_t gpb = BLOCK / KP;
    return (int)std::min<int64_t>(PSTRIDE, std::max<int64_t>(1, (ngroups + gpb - 1) / gpb));
}

template <class T, int KP, bool NT>
__global__ void __launch_bounds__(BLOCK)
k_fbstep_group(const T* __restrict__ x, const T* __restrict__ g, T gamma, T lam, const T* __restrict__ lamv, int K,
               T* __restrict__ z, T* __restrict__ res, int64_t ngroups, double* __restrict__ parts, int slot0) {
    static_assert(KP >= 1 && KP <= 64 && (KP & (KP - 1)) == 0, "a group of KP <= 64 lanes");
    constexpr int GPB = BLOCK / KP;                       // groups per workgroup and trip
    const int k = threadIdx.x % KP;
    const int kc = k < K ? k : K - 1;
    const bool kon = k < K;
    double acc[3] = {0.0, 0.0, 0.0};
    // (the trip count is the workgroup's: every lane of a wave takes every shuffle)
    for (int64_t j0 = (int64_t)blockIdx.x * GPB; j0 < ngroups; j0 += (int64_t)gridDim.x * GPB) {
        const int64_t j = j0 + threadIdx.x / KP;
        const bool on = kon && j < ngroups;
        const int64_t jc = j < ngroups ? j : ngroups - 1;
        const int64_t i = jc * K + kc;
        const T xv = grp_ld<T, NT>(x + i);
        T gv = T(0);
        if (g) gv = grp_ld<T, NT>(g + i);
        T lj = lam;
        if (lamv) lj = grp_ld<T, NT>(lamv + jc);          // (one address across the group's lanes)
        T y = xv;
        if (g) { const T t = gamma * gv; y = xv - t; }
        const T yy = y * y;
        T s = kon ? yy : T(0);
#pragma unroll
        for (int o = KP / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const T nrm = grp_sqrt(s);
        const T gl = gamma * lj;
        T scal, zz;
        if (nrm <= gl) { scal = T(0); zz = T(0); }
        else {
            if (nrm > gl) { const T w = gl / nrm; scal = T(1) - w; }
            else scal = nrm - gl;
            zz = scal * y;
        }
        const T r = xv - zz;
        if (on) {
            z[i] = zz;
            if (res) res[i] = r;
            if (k == 0) {
                T gterm = scal * nrm;
                if (lamv) gterm = lj * gterm;
                acc[0] += (double)gterm;
            }
            acc[1] += (double)(gv * r);
            acc[2] += (double)(r * r);
        }
    }
    block_reduce_store<3>(acc, 0u, parts, slot0);
}

}  // namespace bz
