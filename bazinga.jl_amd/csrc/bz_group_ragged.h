// bz_group_ragged.h — the forward-backward step of the group Lasso over a group pointer (BZ_G_GROUP_LASSO):
//   g(x) = l1 ||x||_1 + sum_j lambda_j ||x[ptr[j] : ptr[j+1]]||_2 , ptr[0] = 0 < ptr[1] < ... < ptr[ng] = n, any size >= 1.
//
// k_fbstep_ragged has k_fbstep's contract (y = x - gamma * g ; z = prox(y) ; res = x - z ; g == nullptr: the pure prox of x ;
// res may be null ; slots +0 the g terms, +1 <g, res>, +2 ||res||^2).  The prox of one group, all in T:
//   L1:  t = gamma * l1 ; u_k = y_k - t (y_k > t), y_k + t (y_k < -t), y_k (a NaN), otherwise +0      (!L1: u = y, not evaluated)
//   q_k = u_k * u_k ; s = the 64-accumulator sum of q (below) ; nrm = sqrt(s) ; gl = gamma * lambda_j
//   nrm <= gl: z = 0 (scal = 0) ; nrm > gl: scal = 1 - gl / nrm ; otherwise (a NaN): scal = nrm - gl ; z_k = scal * u_k
//   the group's term of g(z): scal * nrm (times lambda_j here with a vector lambda, on the host with a number) ;
//   L1: lambda_j * (scal * nrm) + (l1 * scal) * (the 64-accumulator sum of |u_k|), finished here.
//
// The sum of a group is a function of its size alone: 64 accumulators a[p], a[p] = q[p] + q[p + 64] + q[p + 128] + ... in
// that order (positions past the end absent), then the fixed fold a[:o] + a[o:2o] for o = 32 .. 1.  With L lanes per group
// (l = lane % L) a lane walks the elements k = l + L * t, t = 0, 1, ..., and holds the R = 64 / L accumulators p = l + L * r in
// a[r], r = t % R.  The fold pairs a[r] with a[r + h] in the lane for h = R / 2 .. 1 (the offsets 32 .. L) and then runs the
// xor tree over the lane offsets L / 2 .. 1.  Adding the +0 of an absent position to a square (>= +0, or a NaN) is exact, so
// the trips a lane takes past its group's end change no bit, and for a size <= 64 the sum is the fold of k_fbstep_group
// (bz_group.h) over the power of two >= K.
//
// A wave holds 64 / L groups, a workgroup BLOCK / L; the grid strides over the groups.  Lane 0 of a group loads ptr[j],
// ptr[j + 1] and lambda_j and hands them to its L - 1 neighbours.  A wave takes the trip count of its longest group
// (tmax, a wave-uniform scalar).  Up to RAGGED_HOLD trips, x and g stay in registers and are read once; a wave with a
// longer group (LONG: compiled in only where the pointer has one, since its batches cost the short form its occupancy) sweeps twice, every group of it: once in batches of R trips (64 elements of each group, at most RAGGED_FLIGHT loads in flight) for the sums, once
// trip by trip to re-read x and g (from L2) and store.  Both forms add in the same order: the bits do not depend on which
// ran.  Every load is unconditional inside its batch: an element index past the group's end is clamped to the group's last
// element and a group index past the end to the last group — what such a lane computes is dropped (its square, its store,
// its sums).  A group runs on one wave whatever its length.  No LDS but the final block reduction, no atomics.
//
// Included by bz_solver.hip alone, behind bz_group.h (grp_ld, grp_sqrt, group_grid).
#pragma once
#include "bz_group.h"

namespace bz {

constexpr int RAGGED_HOLD = 4;          // trips of a group held in registers: groups of up to 4 L elements are read once
constexpr int RAGGED_FLIGHT = 8;        // loads of x (and of g) in flight in the swept form's batches
constexpr int64_t RAGGED_MAX_GROUP = (int64_t)1 << 30;      // (element offsets inside a group are ints)

// lanes per group: the power of two >= the mean group size, 64 at the most (uniform groups of K: k_fbstep_group's KP)
inline int ragged_lanes(int64_t n, int64_t ngroups) {
    int L = 1;
    while (L < 64 && (int64_t)L * ngroups < n) L *= 2;
    return L;
}

__device__ __forceinline__ float ragged_abs(float v) { return __builtin_fabsf(v); }
__device__ __forceinline__ double ragged_abs(double v) { return __builtin_fabs(v); }

// u of one element: the forward step, then (L1) the soft threshold at t1 = gamma * l1
template <class T, bool L1>
__device__ __forceinline__ T ragged_u(T xv, T gv, bool has_g, T gamma, T t1) {
    T y = xv;
    if (has_g) { const T t = gamma * gv; y = xv - t; }
    if constexpr (L1) {
        const T zero_or_nan = y != y ? y : T(0);
        return y > t1 ? y - t1 : (y < -t1 ? y + t1 : zero_or_nan);
    } else {
        return y;
    }
}

// the fixed fold of a group's 64 accumulators, R = 64 / L of them in each of its L lanes
template <class T, int L>
__device__ __forceinline__ T ragged_fold(T (&a)[64 / L]) {
    constexpr int R = 64 / L;
#pragma unroll
    for (int h = R / 2; h >= 1; h >>= 1) {
#pragma unroll
        for (int r = 0; r < h; ++r) a[r] = a[r] + a[r + h];
    }
    T s = a[0];
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

template <class T, int L, bool NT, bool L1, bool LONG>
__global__ void __launch_bounds__(BLOCK)
k_fbstep_ragged(const T* __restrict__ x, const T* __restrict__ g, T gamma, T lam, const T* __restrict__ lamv, T l1,
                const int64_t* __restrict__ ptr, T* __restrict__ z, T* __restrict__ res, int64_t ngroups,
                double* __restrict__ parts, int slot0) {
    static_assert(L >= 1 && L <= 64 && (L & (L - 1)) == 0, "a group on L <= 64 lanes");
    static_assert(!(LONG && L == 1), "L = 1 means every group has one element: nothing to sweep twice");
    constexpr int R = 64 / L;                             // accumulators per lane
    constexpr int GPB = BLOCK / L;                        // groups per workgroup and trip of the grid
    constexpr int HT = RAGGED_HOLD;
    const int l = threadIdx.x % L;
    const bool has_g = g != nullptr;
    const T t1 = gamma * l1;
    double acc[3] = {0.0, 0.0, 0.0};
    // lane 0 of a group: ptr[j], ptr[j + 1] and lambda_j (a group index past the end: the last group's)
    auto ld_group = [&](int64_t jj, long long& q0, long long& q1, T& ql) {
        const int64_t jc = jj < ngroups ? jj : ngroups - 1;
        if (l == 0) {
            q0 = ptr[jc];
            q1 = ptr[jc + 1];
            if (lamv) ql = lamv[jc];
        }
    };
    const int64_t stride = (int64_t)gridDim.x * GPB;
    long long n0 = 0, n1 = 1;
    T nl = lam;
    ld_group((int64_t)blockIdx.x * GPB + threadIdx.x / L, n0, n1, nl);
    // (the trip count is the workgroup's: every lane of a wave takes every shuffle)
    for (int64_t j0 = (int64_t)blockIdx.x * GPB; j0 < ngroups; j0 += stride) {
        const int64_t j = j0 + threadIdx.x / L;
        const bool jon = j < ngroups;
        long long p0 = n0, p1 = n1;
        T lj = nl;
        // (the next trip's pointer behind this trip's work: x and g are addressed through it, a dependent load otherwise)
        ld_group(j + stride, n0, n1, nl);
        if constexpr (L > 1) {
            const int src = (threadIdx.x & 63) - l;
            p0 = __shfl(p0, src, 64);
            p1 = __shfl(p1, src, 64);
            lj = __shfl(lj, src, 64);
        }
        const int size = (int)(p1 - p0);                  // >= 1, <= RAGGED_MAX_GROUP (validated at creation)
        const int last = size - 1;
        int tm = jon ? (size + L - 1) / L : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tm = max(tm, __shfl_xor(tm, o, 64));
        const int tmax = __builtin_amdgcn_readfirstlane(tm);
        const T* xg = x + p0;
        const T* gg = has_g ? g + p0 : x + p0;            // (never read without g)

        T a[R], b[R];
#pragma unroll
        for (int r = 0; r < R; ++r) { a[r] = T(0); b[r] = T(0); }
        T nrm, scal, sabs = T(0);
        bool zero;
        bool held = true;
        if constexpr (LONG) held = tmax <= HT;            // (!LONG: the host saw no group of more than HT * L elements)
        if (held) {
            // ---- x and g in registers: one sweep
            T xv[HT], gv[HT];
#pragma unroll
            for (int t = 0; t < HT; ++t) {
                xv[t] = T(0); gv[t] = T(0);
                if (t == 0 || t < tmax) {                 // (wave-uniform)
                    const int k = t * L + l;
                    const int kc = k < size ? k : last;
                    xv[t] = grp_ld<T, NT>(xg + kc);
                    if (has_g) gv[t] = grp_ld<T, NT>(gg + kc);
                }
            }
#pragma unroll
            for (int t = 0; t < HT; ++t) {
                if (t == 0 || t < tmax) {
                    const bool kon = t * L + l < size;
                    const T u = ragged_u<T, L1>(xv[t], gv[t], has_g, gamma, t1);
                    const T q = u * u;
                    a[t % R] = a[t % R] + (kon ? q : T(0));
                    if constexpr (L1) b[t % R] = b[t % R] + (kon ? ragged_abs(u) : T(0));
                }
            }
            nrm = grp_sqrt(ragged_fold<T, L>(a));
            if constexpr (L1) sabs = ragged_fold<T, L>(b);
            const T gl = gamma * lj;
            zero = nrm <= gl;
            if (zero) scal = T(0);
            else if (nrm > gl) { const T w = gl / nrm; scal = T(1) - w; }
            else scal = nrm - gl;
#pragma unroll
            for (int t = 0; t < HT; ++t) {
                if (t == 0 || t < tmax) {
                    const int k = t * L + l;
                    const T u = ragged_u<T, L1>(xv[t], gv[t], has_g, gamma, t1);
                    const T zz = zero ? T(0) : scal * u;
                    const T r = xv[t] - zz;
                    if (jon && k < size) {
                        z[p0 + k] = zz;
                        if (res) res[p0 + k] = r;
                        acc[1] += (double)(gv[t] * r);
                        acc[2] += (double)(r * r);
                    }
                }
            }
        } else if constexpr (LONG) {
            // ---- a group too long to hold: the sums in batches of R trips (64 elements of each group), U loads in flight ...
            constexpr int U = R < RAGGED_FLIGHT ? R : RAGGED_FLIGHT;
            const int nbatch = (tmax + R - 1) / R;
            for (int c = 0; c < nbatch; ++c) {
#pragma unroll
                for (int r0 = 0; r0 < R; r0 += U) {
                    T xv[U], gv[U];
#pragma unroll
                    for (int i = 0; i < U; ++i) {
                        const int k = (c * R + r0 + i) * L + l;
                        const int kc = k < size ? k : last;
                        xv[i] = grp_ld<T, false>(xg + kc);
                        gv[i] = T(0);
                        if (has_g) gv[i] = grp_ld<T, false>(gg + kc);
                    }
#pragma unroll
                    for (int i = 0; i < U; ++i) {
                        const bool kon = (c * R + r0 + i) * L + l < size;
                        const T u = ragged_u<T, L1>(xv[i], gv[i], has_g, gamma, t1);
                        const T q = u * u;
                        a[r0 + i] = a[r0 + i] + (kon ? q : T(0));
                        if constexpr (L1) b[r0 + i] = b[r0 + i] + (kon ? ragged_abs(u) : T(0));
                    }
                    // (keeps the next U loads behind these sums: R loads in flight at once cost L = 2 and 4 their registers)
                    if constexpr (R > U) __builtin_amdgcn_sched_barrier(0);
                }
            }
            nrm = grp_sqrt(ragged_fold<T, L>(a));
            if constexpr (L1) sabs = ragged_fold<T, L>(b);
            const T gl = gamma * lj;
            zero = nrm <= gl;
            if (zero) scal = T(0);
            else if (nrm > gl) { const T w = gl / nrm; scal = T(1) - w; }
            else scal = nrm - gl;
            // ... then x and g again (from L2), trip by trip, and the stores
            for (int t = 0; t < tmax; ++t) {
                const int k = t * L + l;
                const int kc = k < size ? k : last;
                const T xv = grp_ld<T, false>(xg + kc);
                T gv = T(0);
                if (has_g) gv = grp_ld<T, false>(gg + kc);
                const T u = ragged_u<T, L1>(xv, gv, has_g, gamma, t1);
                const T zz = zero ? T(0) : scal * u;
                const T r = xv - zz;
                if (jon && k < size) {
                    z[p0 + k] = zz;
                    if (res) res[p0 + k] = r;
                    acc[1] += (double)(gv * r);
                    acc[2] += (double)(r * r);
                }
            }
        }
        if (jon && l == 0) {
            T gterm = scal * nrm;
            if (lamv || L1) gterm = lj * gterm;
            if constexpr (L1) { const T w = l1 * scal; gterm = gterm + w * sabs; }
            acc[0] += (double)gterm;
        }
    }
    block_reduce_store<3>(acc, 0u, parts, slot0);
}

}  // namespace bz
