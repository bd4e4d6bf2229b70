// bz_lbfgs_host.h — the L-BFGS memory as the host sees it: which slot holds which pair, and the compact form's coefficient
// arithmetic.  No device header: a plain C++ compiler builds it, so the loops are checked against `LBFGSCompactOperator` of
// oracle/bazinga_ref.py without a GPU (tests/test_lbfgs_host.py).  Copyable: the solver snapshots its state by assignment.
#pragma once

#include <algorithm>
#include <cmath>
#include <deque>
#include <vector>

namespace bz {

constexpr int MAX_MEM = 16;
constexpr int CM = 5;            // capacity of the compact L-BFGS form (pairs)

template <class T> struct LbfgsMemory {
    // L-BFGS ring: M+1 physical slots, `order` newest first, `spare` receives the candidate pair
    int M = 5;
    std::deque<int> order;
    std::vector<int> freeslots;
    int spare = 0;
    T ys[MAX_MEM + 1] = {};
    T H = T(1);
    // compact form: Gram products of the stored pairs in logical order (oldest first), CM x CM
    int gm = 0;
    double Gsy[CM * CM] = {}, Gyy[CM * CM] = {};
    // p = S'(-res), w = Y'(-res) at the current state (logical order, oldest first), when the accepted
    // trial delivered them (k_fused_compact): the next application then needs no reduction pass at all
    double p_new = 0.0, w_new = 0.0;        // <s_new, -res>, <y_new, -res> of the candidate pair
    bool pw_valid = false;
    double hp[CM] = {0}, hw[CM] = {0};

    void reset_all(int M_) {
        M = M_;
        gm = 0; pw_valid = false;
        order.clear(); freeslots.clear();
        spare = 0;
        for (int i = M; i >= 1; --i) freeslots.push_back(i);
        H = T(1);
    }
    void reset() {                       // reset!(H): currmem = curridx = 0, H = 1
        gm = 0; pw_valid = false;
        for (int s : order) freeslots.push_back(s);
        order.clear();
        H = T(1);
    }
    // Gram products of the stored pairs after inserting a pair whose products with them are sy[i], yy[i]
    // (i = logical index, oldest first): drop the oldest when the ring is full, append row/column
    void gram_insert(double* sy, double* yy, double ys_new, double yty) {
        int m = gm;
        if (m == M) {                    // the oldest pair is overwritten
            for (int i = 1; i < m; ++i)
                for (int j = 1; j < m; ++j) { Gsy[(i - 1) * CM + (j - 1)] = Gsy[i * CM + j]; Gyy[(i - 1) * CM + (j - 1)] = Gyy[i * CM + j]; }
            for (int i = 1; i < m; ++i) { sy[i - 1] = sy[i]; yy[i - 1] = yy[i]; hp[i - 1] = hp[i]; hw[i - 1] = hw[i]; }
            --m;
        }
        hp[m] = p_new; hw[m] = w_new;
        for (int i = 0; i < m; ++i) {
            Gsy[i * CM + m] = sy[i]; Gsy[m * CM + i] = 0.0;
            Gyy[i * CM + m] = yy[i]; Gyy[m * CM + i] = yy[i];
        }
        Gsy[m * CM + m] = ys_new; Gyy[m * CM + m] = yty;
        gm = m + 1;
    }
    // update!(H, s, y) when <s,y> > 0: the pair sits in slot `spare`; sy, yy: its Gram products with the stored pairs
    void insert(T ys_new, T yty, const double* sy, const double* yy, bool compact, bool anderson) {
        if (M == 0) return;              // NoAcceleration: nothing is stored, H stays 1
        if (compact) {
            double z[CM] = {0};
            double a[CM], b[CM];
            for (int i = 0; i < CM; ++i) { a[i] = sy ? sy[i] : z[i]; b[i] = yy ? yy[i] : z[i]; }
            gram_insert(a, b, (double)ys_new, (double)yty);
        }
        order.push_front(spare);
        ys[spare] = ys_new;
        if ((int)order.size() > M) { spare = order.back(); order.pop_back(); }
        else { spare = freeslots.back(); freeslots.pop_back(); }
        H = anderson ? T(1) : ys_new / yty;
    }
    // M1 = R^-T (D + H0 Y'Y) R^-1 and M2 = R^-1 (same loops as LBFGSCompactOperator.coefficient_matrices)
    void compact_matrices(double H0, double* M1, double* M2) const {
        const int m = gm;
        double Ri[CM * CM] = {0}, B[CM * CM] = {0}, T1[CM * CM] = {0};
        for (int j = 0; j < m; ++j) {
            Ri[j * CM + j] = 1.0 / Gsy[j * CM + j];
            for (int i = j - 1; i >= 0; --i) {
                double acc = 0.0;
                for (int k = i + 1; k <= j; ++k) acc += Gsy[i * CM + k] * Ri[k * CM + j];
                Ri[i * CM + j] = -acc / Gsy[i * CM + i];
            }
        }
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < m; ++j) B[i * CM + j] = H0 * Gyy[i * CM + j] + (i == j ? Gsy[i * CM + i] : 0.0);
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < m; ++j) {
                double acc = 0.0;
                for (int k = 0; k <= j; ++k) acc += B[i * CM + k] * Ri[k * CM + j];
                T1[i * CM + j] = acc;
            }
        for (int i = 0; i < CM * CM; ++i) { M1[i] = 0.0; M2[i] = Ri[i]; }
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < m; ++j) {
                double acc = 0.0;
                for (int k = 0; k <= i; ++k) acc += Ri[k * CM + i] * T1[k * CM + j];
                M1[i * CM + j] = acc;
            }
    }
    // Anderson: a = (Y'Y)^-1 Y'v by elimination with complete pivoting on the Gram matrix (pivots below 1e-14 of the
    // largest are treated as a rank deficiency: their coefficient is zero)
    void anderson_coefficients(int m, const double* w, double* a) const {
        double A[CM * CM], b[CM];
        int perm[CM];
        for (int i = 0; i < m; ++i) { b[i] = w[i]; perm[i] = i; for (int j = 0; j < m; ++j) A[i * CM + j] = Gyy[i * CM + j]; }
        double amax = 0.0;
        for (int i = 0; i < m; ++i) amax = std::max(amax, std::abs(A[i * CM + i]));
        int rank = 0;
        for (int k = 0; k < m; ++k) {
            int pi = k, pj = k;
            double best = 0.0;
            for (int i = k; i < m; ++i)
                for (int j = k; j < m; ++j)
                    if (std::abs(A[i * CM + j]) > best) { best = std::abs(A[i * CM + j]); pi = i; pj = j; }
            if (!(best > 1e-14 * amax)) break;
            if (pi != k) { for (int j = 0; j < m; ++j) std::swap(A[k * CM + j], A[pi * CM + j]); std::swap(b[k], b[pi]); }
            if (pj != k) { for (int i = 0; i < m; ++i) std::swap(A[i * CM + k], A[i * CM + pj]); std::swap(perm[k], perm[pj]); }
            for (int i = k + 1; i < m; ++i) {
                const double f = A[i * CM + k] / A[k * CM + k];
                for (int j = k; j < m; ++j) A[i * CM + j] -= f * A[k * CM + j];
                b[i] -= f * b[k];
            }
            rank = k + 1;
        }
        double z[CM] = {0};
        for (int k = rank - 1; k >= 0; --k) {
            double acc = b[k];
            for (int j = k + 1; j < rank; ++j) acc -= A[k * CM + j] * z[j];
            z[k] = acc / A[k * CM + k];
        }
        for (int i = 0; i < m; ++i) a[i] = 0.0;
        for (int k = 0; k < rank; ++k) a[perm[k]] = z[k];
    }
    // The coefficients of one application of the operator to v = -res, from hp = S'v, hw = Y'v and the Gram matrices:
    // H0, u1 = M1 p - H0 M2' w, u2h = H0 * (-(M2 p)), zero beyond the stored pairs (CompactCoef, bz_kernels.h)
    void coefficients(bool anderson, double& H0, double* u1, double* u2h) const {
        const int m = (int)order.size();
        H0 = (double)H;
        if (anderson) {
            // d = v + (S - Y) a , a = (Y'Y)^-1 Y'v : the compact kernels' linear combination with u1 = a, H0 u2 = -a
            double a[CM] = {0};
            anderson_coefficients(m, hw, a);
            H0 = 1.0;
            for (int i = 0; i < CM; ++i) { u1[i] = i < m ? a[i] : 0.0; u2h[i] = i < m ? -a[i] : 0.0; }
            return;
        }
        double M1[CM * CM], M2[CM * CM];
        compact_matrices(H0, M1, M2);
        // same loops as LBFGSCompactOperator.__call__ (rows/columns beyond m are zero)
        for (int i = 0; i < CM; ++i) {
            double a = 0.0, b = 0.0, c = 0.0;
            for (int j = 0; j < CM; ++j) a += M1[i * CM + j] * (j < m ? hp[j] : 0.0);
            for (int j = 0; j < CM; ++j) b += M2[j * CM + i] * (j < m ? hw[j] : 0.0);
            for (int j = 0; j < CM; ++j) c += M2[i * CM + j] * (j < m ? hp[j] : 0.0);
            u1[i] = i < m ? a - H0 * b : 0.0;
            u2h[i] = i < m ? H0 * (-c) : 0.0;
        }
    }
};

}  // namespace bz
