"""The dense f kinds LeastSquares(A, b) and Quadratic(Q, q) with c = Identity (dense_f_eval: k_gemv_n, k_gemv_t,
k_gemv_t_mfma, gemv_t_fold, k_algrad_elem in its modes 1 and 2), the part that needs no GPU: the table of shapes with the
proof that each reaches the branch it is named for, the generators, the extended-precision twins of the two oracles, the
a-priori forward bound of one AL gradient, and the proof, on the oracle alone, that every 30-state run of
tests/test_gpu_dense_f.py meets the conditions its comparison rests on.

"The oracle's two roundings" are the plain oracle and the oracle with the twin f (matrix products and dots in
np.longdouble, rounded once) under `LongDoubleReducer`: the oracle's matrix products are BLAS calls that no reducer
reaches, so the reducer alone does not show the rounding sensitivity of a run on this path.

A run case is compared over `compared` states: up to the first state where 100 x the distance of the two roundings
exceeds 1e-2 (`by_sens`), and no further than the state before the first step with an unsettled decision (`settled` of
tests/test_linesearch_host.py: a margin of a gamma halving or of the envelope test inside the difference of the two
roundings' margins).  In fp32 the device took such a step the other way at state 27 of q-1030-f32-nonneg-xor: margin
-4.3e-4 under a floor of 3.4e-4.

Conditions, asserted below for every case in every form it runs in, with the seeds and the data pinned in SEEDS and
SLOW: at least 10 compared states; in fp64 at least 15 of the 30 states with the roundings within 1e-11, in fp32 at
least 4 within 5e-7; the cases marked with events show them inside the compared range."""
import warnings
import zlib

import numpy as np
import pytest

from oracle import bazinga_ref as REF
from tests.test_linesearch_host import Case, OracleRun, settled

LD = np.longdouble
F64, F32 = np.float64, np.float32
BLOCK, WAVES = 256, 4          # bz_kernels.h
GEMV_N_MAX_GRID = 65535        # gemv_rows
PERSIST_MIN_N = 300000         # BZ_PERSIST_MIN_N's default
STATES = 30


def tname(dt):
    return "f64" if np.dtype(dt) == np.float64 else "f32"


def _rng(*key):
    return np.random.default_rng(zlib.crc32("-".join(str(k) for k in key).encode()))


# ------------------------------------------------------------------------------------------ the extended-precision twins
class LeastSquaresTwin(REF.LeastSquares):
    """ref.LeastSquares with r = A x - b, A'r and <r, r> carried in np.longdouble and rounded once to x's type"""

    def _r(self, x):
        if not hasattr(self, "_A"):
            self._A, self._b = self.A.astype(LD), self.b.astype(LD)
        return self._A @ x.astype(LD) - self._b

    def __call__(self, x):
        r = self._r(x)
        return x.dtype.type(LD(self.lam) / 2 * np.sum(r * r))

    def gradient(self, y, x):
        r = self._r(x)
        y[...] = (LD(self.lam) * (r @ self._A)).astype(x.dtype)
        return x.dtype.type(LD(self.lam) / 2 * np.sum(r * r))


class QuadraticTwin(REF.Quadratic):
    """ref.Quadratic with Q x, x'Qx and q'x carried in np.longdouble and rounded once to x's type"""

    def _Qx(self, x):
        if not hasattr(self, "_Q"):
            self._Q, self._q = self.Q.astype(LD), self.q.astype(LD)
        xl = x.astype(LD)
        return xl, self._Q @ xl

    def __call__(self, x):
        xl, Qx = self._Qx(x)
        return x.dtype.type(LD(0.5) * np.sum(xl * Qx) + np.sum(xl * self._q))

    def gradient(self, y, x):
        xl, Qx = self._Qx(x)
        y[...] = (Qx + self._q).astype(x.dtype)
        return x.dtype.type(LD(0.5) * np.sum(xl * Qx) + np.sum(xl * self._q))


def twin_of(f):
    return LeastSquaresTwin(f.A, f.b) if isinstance(f, REF.LeastSquares) else QuadraticTwin(f.Q, f.q)


# ------------------------------------------------------------------------------------------------- shapes and their routes
# LeastSquares (m, n) and the types that run it; Quadratic n.  What each is the smallest to reach: test_shapes_reach_*.
REFERENCE_A = [[1.0, -2.0, 3.0, -4.0, 5.0], [2.0, -1.0, 0.0, -1.0, 3.0], [-1.0, 0.0, 4.0, -3.0, 2.0], [-1.0, -1.0, -1.0, 1.0, 3.0]]
REFERENCE_B = [1.0, 2.0, 3.0, 4.0]          # test/problems/test_verbose.jl, as tests/test_gpu_reference_tests.py types it
BOTH = (F64, F32)
LS_SHAPES = [((4, 5), BOTH), ((1, 4), BOTH), ((3, 70), BOTH), ((33, 17), BOTH), ((257, 1031), BOTH), ((257, 1028), BOTH),
             ((7, 64), (F32,)), ((260, 1024), (F32,)), ((5000, 128), BOTH), ((16400, 64), (F32,)), ((70001, 8), BOTH),
             ((8, 300034), (F64,))]
# 512 / 1024: exactly 256 packs, every thread of k_gemv_n one pack in the single-pack loop and none in the two-pack loop
Q_SIZES = [(2, BOTH), (100, BOTH), (514, BOTH), (1030, BOTH), (2052, (F32,)), (512, (F64,)), (1024, (F32,))]
WIDE = (8, 300034)
D_EXACT = ("zero", "free", "box", "box_vec", "vc", "cc", "eitheror", "xor")
PAIRWISE = ("vc", "cc", "eitheror", "xor")


def pack_of(dt):
    return 16 // np.dtype(dt).itemsize


def plan_chunks(rows, cols, dt):
    """plan_chunks of bz_solver.hip restated: (rows per chunk, chunks)"""
    colblocks = max(1, (cols // pack_of(dt) + BLOCK - 1) // BLOCK)
    chunks = max(1, min(rows, (2048 + colblocks - 1) // colblocks))
    rpc = -(-rows // chunks)
    return rpc, -(-rows // rpc)


def route(rows, cols, dt, transposed=True):
    """which branches one product with a rows x cols matrix takes (k_gemv_n; with `transposed` k_gemv_t / k_gemv_t_mfma and
    gemv_t_fold too), from the launch code and the kernels restated"""
    N = pack_of(dt)
    aligned = cols % N == 0
    npk = cols // N if aligned else 0
    two = [t for t in range(BLOCK) if t + BLOCK < npk]                 # threads that enter k_gemv_n's two-pack loop
    after = lambda t: t + 2 * BLOCK * (-(-(npk - BLOCK - t) // (2 * BLOCK))) if t + BLOCK < npk else t
    one = [t for t in range(BLOCK) if after(t) < npk]                  # ... its single-pack loop behind it
    r = dict(aligned=aligned, npk=npk, two_pack_threads=len(two), one_pack_threads=len(one), grid=min(rows, GEMV_N_MAX_GRID),
             row_stride_loop=rows > GEMV_N_MAX_GRID)
    if transposed:
        rpc, nch = plan_chunks(rows, cols, dt)
        last = rows - (nch - 1) * rpc
        r.update(rpc=rpc, nch=nch, last_rows=last, mfma=np.dtype(dt) == np.float32 and cols % 64 == 0,
                 fold8=(nch - 1) // 8, fold_rest=(nch - 1) % 8)
    return r


def gemv_bytes(rows, cols, dt, with_b, transposed):
    """the bytes gemv_rows (and gemv_cols) account for: the matrix once, p, b and the result ; the matrix once, v and the
    row-chunk partials of npadx columns"""
    sz, N = np.dtype(dt).itemsize, pack_of(dt)
    total = (rows * cols + (2 if with_b else 1) * rows + cols) * sz
    if transposed:
        npadx = -(-cols // N) * N
        total += (rows * cols + rows + plan_chunks(rows, cols, dt)[1] * npadx) * sz
    return total


# ------------------------------------------------------------------------------------------------------------ D and g
def d_pair(bz, ref, D, n, dt, rng, integer=False):
    T = np.dtype(dt).type
    if integer:
        lo, hi = rng.integers(-3, 1, n).astype(dt), rng.integers(0, 4, n).astype(dt)
        s_lo, s_hi = -1.0, 2.0
    else:
        lo, hi = (-rng.uniform(0.1, 1.0, n)).astype(dt), rng.uniform(0.1, 1.0, n).astype(dt)
        s_lo, s_hi = -0.5, 0.5
    if D == "zero":
        return bz.ZeroSet(), ref.ZeroSet()
    if D == "free":
        return bz.FreeSet(), ref.FreeSet()
    if D == "box":
        return bz.ClosedSet(bz.IndBox(s_lo, s_hi)), ref.ClosedSet(ref.IndBox(T(s_lo), T(s_hi)))
    if D == "box_vec":
        return bz.ClosedSet(bz.IndBox(lo, hi)), ref.ClosedSet(ref.IndBox(lo, hi))
    return bz.PairwiseSet(D), ref.PairwiseSet(D)


G_KINDS = ("zero", "l1", "l1_vec", "nonneg", "l1box", "l0box", "indbox", "indbox_vec", "lpbox", "l21", "grouplasso")
D_KINDS = ("zero", "free", "box", "box_vec", "xor", "vc")
SUPPORT_G = ("lpbox", "l0box")          # compared on the common support (the rule of test_lp_power_prox)


def g_pair(bz, ref, g, n, dt, rng):
    """(device g, oracle g).  NormL1 with a vector, NormL21 and GroupLasso have no reference class: the package's own
    numpy `prox` is their specification (tests/test_gpu_weighted_l1.py, tests/test_gpu_group_lasso*.py)"""
    T = np.dtype(dt).type
    u = np.where(np.arange(n) % 5 == 0, 0.0, rng.uniform(0.3, 1.0, n)).astype(dt)
    lo, hi = (-rng.uniform(0.2, 1.0, n)).astype(dt), rng.uniform(0.2, 1.0, n).astype(dt)
    lamv = np.where(np.arange(n) % 7 == 0, 0.0, rng.uniform(0.02, 0.2, n))
    if g == "zero":
        return bz.Zero(), ref.Zero()
    if g == "l1":
        return bz.NormL1(0.1), ref.NormL1(T(0.1))
    if g == "l1_vec":
        return bz.NormL1(lamv), bz.NormL1(lamv)
    if g == "nonneg":
        return bz.NormL1Nonneg(0.1), ref.NormL1Nonneg(T(0.1))
    if g == "l1box":
        return bz.NormL1Box(0.1, u=u), ref.NormL1Box(T(0.1), u=u)
    if g == "l0box":
        return bz.NormL0Box(0.1, u=u), ref.NormL0Box(T(0.1), u=u)
    if g == "indbox":
        return bz.IndBox(-0.5, 0.5), ref.IndBox(T(-0.5), T(0.5))
    if g == "indbox_vec":
        return bz.IndBox(lo, hi), ref.IndBox(lo, hi)
    if g == "lpbox":
        return bz.NormLpPowerBox(0.5, 0.1, u=u), ref.NormLpPowerBox(0.5, T(0.1), u=u)
    if g == "l21":
        lam = np.where(np.arange(n // 3) % 6 == 0, 0.0, rng.uniform(0.02, 0.2, n // 3))
        return bz.NormL21(lam, 3), bz.NormL21(lam, 3)
    sizes = []
    while sum(sizes) < n:          # ragged groups of 1 .. 9 elements
        sizes.append(min(int(rng.integers(1, 10)), n - sum(sizes)))
    lam = 0.05 * np.sqrt(np.array(sizes, float))
    gl = bz.GroupLasso.from_sizes(lam, np.array(sizes), 0.02)
    return gl, gl


# ---------------------------------------------------------------------------------------------------- one AL gradient
def smooth_pair(bz, ref, kind, shape, dt, rng, mode):
    """mode "exact": A, Q with entries in {-2 .. 2} (Q symmetric), b, q integers ; "real": standard normal entries scaled by
    1 / sqrt(n) ; "convex": Q = F F' / n + diag(U(0.5, 1.5)) ; "nonconvex": eigenvalues in (-1, 1), as test_nonconvex_qp_small"""
    if kind == "ls":
        m, n = shape
        if mode == "exact":
            A = np.array(REFERENCE_A, dt) if shape == (4, 5) else rng.integers(-2, 3, (m, n)).astype(dt)
            b = np.array(REFERENCE_B, dt) if shape == (4, 5) else rng.integers(-3, 4, m).astype(dt)
        elif mode == "slow":
            # columns scaled over 1.5 decades and b = A x_t: the minimum of f is 0 and is approached slowly, so a step keeps
            # lowering the envelope by far more than its rounding for the whole run
            A = (rng.standard_normal((m, n)) / np.sqrt(n) * 10.0 ** rng.uniform(-1.5, 0, n)).astype(dt)
            b = (A.astype(np.float64) @ (0.3 * rng.standard_normal(n))).astype(dt)
        else:
            A, b = (rng.standard_normal((m, n)) / np.sqrt(n)).astype(dt), rng.standard_normal(m).astype(dt)
        return bz.LeastSquares(A, b), ref.LeastSquares(A, b)
    n = shape
    if mode == "exact":
        U = rng.integers(-2, 3, (n, n))
        Q, q = (np.triu(U) + np.triu(U, 1).T).astype(dt), rng.integers(-3, 4, n).astype(dt)
    elif mode == "nonconvex":
        U, _ = np.linalg.qr(rng.standard_normal((n, n)))
        Q = U @ np.diag(2.0 * rng.random(n) - 1.0) @ U.T
        Q, q = (0.5 * (Q + Q.T)).astype(dt), rng.standard_normal(n).astype(dt)
    elif mode == "slow":          # convex, eigenvalues over three decades
        U, _ = np.linalg.qr(rng.standard_normal((n, n)))
        Q = U @ np.diag(10.0 ** rng.uniform(-3, 0, n)) @ U.T
        Q, q = (0.5 * (Q + Q.T)).astype(dt), rng.standard_normal(n).astype(dt)
    elif mode == "convex":
        F = rng.standard_normal((n, max(1, n // 8)))
        Q = F @ F.T / n + np.diag(rng.uniform(0.5, 1.5, n))
        Q, q = (0.5 * (Q + Q.T)).astype(dt), rng.standard_normal(n).astype(dt)
    else:
        Q = rng.standard_normal((n, n)) / np.sqrt(n)
        Q, q = (0.5 * (Q + Q.T)).astype(dt), rng.standard_normal(n).astype(dt)
    assert np.array_equal(Q, Q.T)
    return bz.Quadratic(Q, q), ref.Quadratic(Q, q)


def n_of(kind, shape):
    return shape[1] if kind == "ls" else shape


def gradient_case(bz, ref, kind, shape, dt, D, mode):
    """(device oracles, reference oracles, mu, y, x) of one AL gradient: integer data and mu = 1/4 ("exact": in fp32 x has six
    non-zeros, one beyond 5000 rows, so that every sum stays below 2^24) or real data and penalties 10^U(-2, 0) ("real").
    The data do not depend on D."""
    n = n_of(kind, shape)
    rng = _rng("gradient", kind, shape, tname(dt), mode)
    fd, fr = smooth_pair(bz, ref, kind, shape, dt, rng, mode)
    if mode == "exact":
        x = rng.integers(-4, 5, n).astype(dt)
        if np.dtype(dt) == np.float32:
            k = min(n, 6 if (kind == "q" or shape[0] <= 5000) else 1)
            x = np.zeros(n, dt)
            x[rng.choice(n, k, replace=False)] = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), k)
        y, mu = rng.integers(-3, 4, n).astype(dt), np.full(n, 0.25, dt)
    else:
        x, y = rng.standard_normal(n).astype(dt), rng.standard_normal(n).astype(dt)
        mu = (10.0 ** rng.uniform(-2, 0, n)).astype(dt)
    Dd, Dr = d_pair(bz, ref, D, n, dt, _rng("gradient-D", kind, shape, tname(dt), mode), integer=mode == "exact")
    return (fd, bz.NormL1(0.3), bz.IdentityFunction(), Dd), (fr, ref.NormL1(0.3), ref.IdentityFunction(), Dr), mu, y, x


def oracle_gradient(ref, orc, mu, y, x, twin=False):
    """(gradient, L, f, the AugLagFun) of the oracle; twin: with the twin f under LongDoubleReducer"""
    from tests.test_gpu_parity import LongDoubleReducer
    f = twin_of(orc[0]) if twin else orc[0]
    ref.set_reducer(LongDoubleReducer() if twin else None)
    try:
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            al = ref.AugLagFun(f, orc[2], orc[3], mu.copy(), y.copy(), x)
            g = np.empty_like(x)
            lx = al.gradient(g, x)
    finally:
        ref.set_reducer(None)
    return g, lx, al.fx, al


def exact_cases():
    """(kind, shape, dtype, D) of the exact table; the pairwise kinds where n is even"""
    out = []
    for kind, shapes in (("ls", LS_SHAPES), ("q", Q_SIZES)):
        for shape, types in shapes:
            for dt in types:
                for D in D_EXACT:
                    if D in PAIRWISE and n_of(kind, shape) % 2:
                        continue
                    out.append((kind, shape, dt, D))
    return out


def case_id(c):
    kind, shape, dt = c[:3]
    s = f"{shape[0]}x{shape[1]}" if kind == "ls" else str(shape)
    return "-".join([kind, s, tname(dt)] + [str(v) for v in c[3:]])


def assert_exact(ref, kind, dt, orc, mu, y, x):
    """every partial sum of magnitudes stays below 2^53 / 2^24 in its finest unit (matrix products: 1 ; c(x) + mu y = x + y / 4:
    1/4 ; the values: 1/8, from mu y^2 / 2 and t^2 / (2 mu)), so no summation order changes a bit — and the oracle in `dt`
    returns the float64 oracle's values"""
    lim = 2.0 ** (24 if np.dtype(dt) == np.float32 else 53)
    x64, y64 = x.astype(F64), y.astype(F64)
    g, lx, fx, al = oracle_gradient(ref, orc, mu, y, x)
    yupd = np.abs(al.yupd.astype(F64))
    t = yupd * 0.25
    if kind == "ls":
        A, b = np.abs(orc[0].A.astype(F64)), np.abs(orc[0].b.astype(F64))
        r = orc[0].A.astype(F64) @ x64 - orc[0].b.astype(F64)
        assert np.max(A @ np.abs(x64) + b) < lim
        assert np.max(np.abs(r) @ A + yupd) < lim
        fmag = 0.5 * np.sum(r * r)
    else:
        Q, q = np.abs(orc[0].Q.astype(F64)), np.abs(orc[0].q.astype(F64))
        Qx = Q @ np.abs(x64)
        assert np.max(Qx + q + yupd) < lim
        fmag = np.sum(np.abs(x64) * (0.5 * Qx + q)) + 0.5 * np.sum(np.abs(x64) * Qx) + np.sum(np.abs(x64) * q)
    assert 4 * np.max(np.abs(x64) + 0.25 * np.abs(y64) + t) < lim
    assert 8 * (fmag + 0.5 * np.sum(t * t / 0.25) + 0.5 * np.sum(0.25 * y64 ** 2)) < lim
    o64 = tuple(type(o)(*[a.astype(F64) for a in ((o.A, o.b) if kind == "ls" else (o.Q, o.q))]) if i == 0 else o for i, o in enumerate(orc))
    if isinstance(orc[3], ref.IndicatorSet):
        o64 = o64[:3] + (ref.ClosedSet(ref.IndBox(np.asarray(orc[3].f.lb, F64), np.asarray(orc[3].f.ub, F64))),)
    g64, lx64, fx64, _ = oracle_gradient(ref, o64, mu.astype(F64), y64, x64)
    assert np.array_equal(g.astype(F64), g64) and float(lx) == float(lx64) and float(fx) == float(fx64)
    return g, lx, fx


def gamma_k(k, dt):
    u = float(np.finfo(dt).eps) / 2
    assert k * u < 0.01
    return k * u / (1 - k * u)


def forward_bound(kind, dt, orc, mu, y, x, g_twin, al_twin):
    """The a-priori bound of |computed - twin| for one AL gradient whose sums are taken in `dt` in ANY order; u = eps / 2,
    gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: a sum of k terms).
      LeastSquares: |r^ - r| <= dr = gamma_{n+1} (|A| |x| + |b|) ;  |A' r^ - A' r| <= E = gamma_{m+nch} |A'| (|r| + dr) + |A'| dr
                    (m products and adds of a column sum, and the nch - 1 adds of the row-chunk partials counted again)
                    f = <r^, r^> / 2: Ef = (sum (2 |r| dr + dr^2) + gamma_{m+2} sum (|r| + dr)^2) / 2
      Quadratic:    |(Q x + q)^ - (Q x + q)| <= E = gamma_{n+1} (|Q| |x| + |q|)
                    f = sum x (Q x / 2 + q): Ef = sum |x| E / 2 + gamma_{n+3} sum |x| (|Q| |x| / 2 + |q|)
    The part of the gradient that comes from D is element-wise and the same operations on both sides; the last addition
    rounds once on each side and the twin's f part is rounded once: bound = 1.01 (E + u |dfx| + 2 u |gradient|), the 1.01
    for the second-order terms.  L = f + pen / 2 - mu y^2 / 2 with two sums of n terms and three roundings:
    EL = 1.01 (Ef + gamma_{n+1} (pen / 2 + musqy) + 3 u (|f| + pen / 2 + musqy)).  Returns (bound per component, EL, Ef)."""
    u = float(np.finfo(dt).eps) / 2
    n = x.shape[0]
    ax = np.abs(x.astype(LD))
    if kind == "ls":
        A, b = orc[0].A.astype(LD), orc[0].b.astype(LD)
        m = A.shape[0]
        nch = plan_chunks(m, n, dt)[1]
        r = np.abs(A @ x.astype(LD) - b)
        dr = gamma_k(n + 1, dt) * (np.abs(A) @ ax + np.abs(b))
        E = gamma_k(m + nch, dt) * ((r + dr) @ np.abs(A)) + dr @ np.abs(A)
        Ef = 0.5 * (np.sum(2 * r * dr + dr * dr) + gamma_k(m + 2, dt) * np.sum((r + dr) ** 2))
    else:
        Q, q = np.abs(orc[0].Q.astype(LD)), np.abs(orc[0].q.astype(LD))
        E = gamma_k(n + 1, dt) * (Q @ ax + q)
        Ef = 0.5 * np.sum(ax * E) + gamma_k(n + 3, dt) * np.sum(ax * (0.5 * (Q @ ax) + q))
    dfx = np.abs(al_twin.dfx.astype(LD))
    bound = 1.01 * (E + u * dfx + 2 * u * np.abs(g_twin.astype(LD)))
    pen = np.sum((al_twin.yupd.astype(LD) * mu.astype(LD)) ** 2 / mu.astype(LD))
    musqy = 0.5 * np.sum(mu.astype(LD) * y.astype(LD) ** 2)
    EL = 1.01 * (Ef + gamma_k(n + 1, dt) * (0.5 * pen + musqy) + 3 * u * (abs(LD(al_twin.fx)) + 0.5 * pen + musqy))
    return bound.astype(F64), float(EL), float(1.01 * (Ef + u * abs(LD(al_twin.fx))))


REAL_SHAPES = [("ls", s, dt) for s, types in LS_SHAPES for dt in types] + [("q", s, dt) for s, types in Q_SIZES for dt in types]
SPECIAL_SHAPES = [("ls", (257, 1031), F64), ("ls", (257, 1031), F32), ("ls", (260, 1024), F32), ("q", 514, F64), ("q", 514, F32)]


def special_case(bz, ref, kind, shape, dt):
    """the real-data gradient case with x scaled by 0.02, and Quadratic's q by 0.2 (test_largest_finite_entry_overflows_no_sum
    says why)"""
    dev, orc, mu, y, x = gradient_case(bz, ref, kind, shape, dt, "box", "real")
    if kind == "q":
        q = (np.dtype(dt).type(0.2) * orc[0].q).astype(dt)
        dev, orc = (bz.Quadratic(orc[0].Q, q),) + tuple(dev[1:]), (ref.Quadratic(orc[0].Q, q),) + tuple(orc[1:])
    return dev, orc, mu, y, (np.dtype(dt).type(0.02) * x).astype(dt)


def overflow_corner(bz, ref, dt):
    """the special-argument case of Quadratic, n = 514, with x_0 the largest finite number and q_0 = -2 sign(Q_00): x_0 q_0
    overflows by itself, against the sign of x_0 Q_00 x_0 (test_quadratic_value_at_the_overflow_corner_is_nan_on_the_oracle)"""
    dev, orc, mu, y, x = special_case(bz, ref, "q", 514, dt)
    T = np.dtype(dt).type
    q = orc[0].q.copy()
    q[0] = T(-2) * np.sign(orc[0].Q[0, 0])
    x[0] = np.finfo(dt).max
    return (bz.Quadratic(orc[0].Q, q),) + tuple(dev[1:]), (ref.Quadratic(orc[0].Q, q),) + tuple(orc[1:]), mu, y, x


def special_positions(n, dt):
    """column 0, both sides of the first pack boundary, the last column"""
    N = pack_of(dt)
    return [0, N - 1, N, n - 1]


def special_values(dt):
    return [np.nan, np.inf, -np.inf, float(np.finfo(dt).max)]


# --------------------------------------------------------------------------------------------------- the run cases
class DenseCase(Case):
    """a Case of tests/test_linesearch_host.py with the form of the L-BFGS operator: compact None (auto), False or True"""

    def __init__(self, name, dt, build, M=20, direction="lbfgs", compact=False, claims="", states=STATES, kind="ls", g="l1"):
        Case.__init__(self, name, "dense_f", dt, M, build, claims, direction, states=states)
        self.compact, self.kind, self.g = compact, kind, g

    def directions(self, m):
        if self.direction == "lbfgs":
            return m.LBFGS(5, compact=self.compact)
        return Case.directions(self, m)

    def with_form(self, compact):
        c = DenseCase(self.name, self.dtype, self.build, self.M, self.direction, compact, self.claims, self.states, self.kind, self.g)
        return c


def run_build(kind, shape, dt, g, D, seed, ys=1.0, xs=0.3, mode=None):
    def build(bz, ref):
        n = n_of(kind, shape)
        rng = _rng("run", kind, shape, tname(dt), g, D, seed)
        fd, fr = smooth_pair(bz, ref, kind, shape, dt, rng, mode or ("real" if kind == "ls" else "convex"))
        gd, gr = g_pair(bz, ref, g, n, dt, rng)
        Dd, Dr = d_pair(bz, ref, D, n, dt, rng)
        mu = (10.0 ** rng.uniform(-2, 0, n)).astype(dt)
        y, x0 = (ys * rng.standard_normal(n)).astype(dt), (xs * rng.standard_normal(n)).astype(dt)
        return (fd, gd, bz.IdentityFunction(), Dd), (fr, gr, ref.IdentityFunction(), Dr), n, n, mu, y, x0
    return build


RUN_SHAPES = {"ls": [(257, 1031), (33, 1024), (5000, 128)], "q": [514, 1030]}
# NormL21(K = 3): 3 divides none of the sizes above; its cases run at the nearest sizes it divides (both unaligned)
L21_SHAPES = {"ls": (33, 1023), "q": 1029}
# the pinned seeds of the run cases (0 where the first seed keeps the conditions): see `python -m tests.test_dense_f_host`
SEEDS = {"ls-33x1024-f32-indbox_vec-box": 1, "q-1030-f32-l1-box": 3, "q-514-f32-l1_vec-box_vec": 4, "q-1030-f32-indbox_vec-box": 2,
         "q-1029-f32-l21-box_vec": 1, "ls-5000x128-f64-l1_vec-box": 5, "ls-5000x128-f64-lpbox-box": 4}
# Five fp32 slots converge within a few steps on the data of the other slots (standard normal A, Q = F F' / n + diag): from
# then on the envelope test's margin is below 10 eps (1 + |FBE|) — |FBE| is some 3e3 at 5000 rows, a step must lower it by 3e-3
# to be told from rounding — and the decisions are settled for 3 to 9 states with every one of 40 seeds, far starts included.
# They run on data that is approached slowly instead (smooth_pair: "slow", and the nonconvex Q inside the box g), which
# keeps 13 to 30 settled states: (mode, seed).
SLOW = {"ls-5000x128-f32-l1_vec-box_vec": ("slow", 2), "ls-5000x128-f32-l0box-zero": ("slow", 0), "ls-5000x128-f32-lpbox-box_vec": ("slow", 0),
        "q-514-f32-zero-free": ("slow", 0), "q-514-f32-indbox-free": ("nonconvex", 4)}


# events of the table's own cases that are asserted (4 tau backtracks and 41 gamma halvings in its 17 compared states)
CLAIMS = {"ls-33x1024-f64-l1box-xor": "bh"}


def table_cases():
    """per f kind and type the eleven g kinds, D and the shape rotated over them (a pairwise D moves on to an even n)"""
    out = []
    for kind in ("ls", "q"):
        for ti, dt in enumerate(BOTH):
            for gi, g in enumerate(G_KINDS):
                D = D_KINDS[(gi + ti) % len(D_KINDS)]
                shapes = RUN_SHAPES[kind]
                shape = shapes[gi % len(shapes)]
                if D in PAIRWISE and n_of(kind, shape) % 2:
                    shape = shapes[(gi + 1) % len(shapes)]
                if g == "l21":
                    shape = L21_SHAPES[kind]
                    if D in PAIRWISE:
                        D = "box_vec"
                name = case_id((kind, shape, dt, g, D))
                mode, seed = SLOW.get(name, (None, SEEDS.get(name, 0)))
                out.append(DenseCase(name, dt, run_build(kind, shape, dt, g, D, seed, mode=mode), claims=CLAIMS.get(name, ""), kind=kind, g=g))
    return out


TABLE = table_cases()
# the event cases: tau backtracks (two or more) and a gamma halving after state 1 inside the compared range, per f kind;
# far starts, the nonconvex Q.  claims: "b" backtracks, "h" a halving after the start
EVENT_CASES = []
# other directions and the line search at its limit (fp64)
OTHER = []


def add_event(name, kind, shape, dt, g, D, seed, claims, **kw):
    M = kw.pop("M", 20)
    direction = kw.pop("direction", "lbfgs")
    lst = kw.pop("into", EVENT_CASES)
    lst.append(DenseCase(name, dt, run_build(kind, shape, dt, g, D, seed, **kw), M=M, direction=direction, claims=claims, kind=kind, g=g))


# (filled from the probe at the foot of this file)
add_event("ev-ls-257x1031-f64", "ls", (257, 1031), F64, "l1", "box", 1, "b")
add_event("ev-ls-33x1024-f64-far", "ls", (33, 1024), F64, "l1", "box", 0, "h", ys=20.0, xs=10.0)
add_event("ev-q-514-f64", "q", 514, F64, "l1", "box", 0, "bh", mode="convex")
add_event("ev-q-1030-f64-nonconvex", "q", 1030, F64, "l1", "box", 2, "bh", mode="nonconvex")
add_event("anderson-ls-257x1031", "ls", (257, 1031), F64, "l1", "box", 0, "", direction="anderson", into=OTHER)
add_event("broyden-ls-33x1024", "ls", (33, 1024), F64, "l1", "box", 0, "", direction="broyden", into=OTHER)
add_event("M2-ls-257x1031-far", "ls", (257, 1031), F64, "l1", "box", 0, "b", M=2, ys=20.0, xs=10.0, into=OTHER)
add_event("anderson-q-514", "q", 514, F64, "l1", "box", 0, "", direction="anderson", into=OTHER)
add_event("broyden-q-1030", "q", 1030, F64, "l1", "box", 0, "", direction="broyden", into=OTHER)
add_event("M2-q-514-nonconvex", "q", 514, F64, "l1", "box", 2, "bh", M=2, mode="nonconvex", into=OTHER)
# the wide case: n over the persistent two-loop's threshold, 15 states, the two-loop form
WIDE_CASE = DenseCase("wide-ls-8x300034-f64", F64, run_build("ls", WIDE, F64, "l1", "box", 0), compact=False, states=15)
# the start of a solve (one state): the oracle's init() under both roundings
START_CASES = [DenseCase("start-" + case_id((k, s, dt)), dt, run_build(k, s, dt, "l1", "box", 0), states=1, kind=k)
               for k, s, types in (("ls", (257, 1031), BOTH), ("ls", (260, 1024), (F32,)), ("ls", (257, 1028), BOTH), ("ls", (5000, 128), BOTH),
                                   ("q", 514, BOTH), ("q", 1030, BOTH)) for dt in types]


def solve_case(bz, ref, which, dt=F64):
    """the whole solves: (device oracles, reference oracles, n, x0).  "lasso": 257 x 1031, lambda = 0.1 max |A'b| and D = free as
    test_verbose.jl sets them ; "qp": n = 514, eigenvalues in (-1, 1), g = D = the box [-1, 1] as test_nonconvex_qp.jl.  The start
    is not zero (A x0 must not vanish whatever the kernel computes) and f(x0) + g(x0) > 1 (so that the initial penalties,
    max(1, d^2 / 2) / max(1, f + g) / 10, carry the f value of the start: test_solve_cases_*)."""
    T = np.dtype(dt).type
    if which == "lasso":
        rng = _rng("solve", which)
        fd, fr = smooth_pair(bz, ref, "ls", (257, 1031), dt, rng, "real")
        lam = float(T(0.1) * np.max(np.abs(fr.A.T @ fr.b)))
        dev = (fd, bz.NormL1(lam), bz.IdentityFunction(), bz.FreeSet())
        orc = (fr, ref.NormL1(T(lam)), ref.IdentityFunction(), ref.FreeSet())
        return dev, orc, 1031, (0.3 * rng.standard_normal(1031)).astype(dt)
    rng = _rng("solve", which, 1)
    fd, fr = smooth_pair(bz, ref, "q", 514, dt, rng, "nonconvex")
    dev = (fd, bz.IndBox(-1.0, 1.0), bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(-1.0, 1.0)))
    orc = (fr, ref.IndBox(T(-1), T(1)), ref.IdentityFunction(), ref.ClosedSet(ref.IndBox(T(-1), T(1))))
    return dev, orc, 514, (0.9 * np.sign(fr.q)).astype(dt)          # (q'x0 = 0.9 |q|_1: f(x0) > 1)


_SOLVES = {}


def ref_solve(bz, ref, which):
    """the oracle's whole solve, computed once and shared (never changed)"""
    if which not in _SOLVES:
        dev, orc, n, x0 = solve_case(bz, ref, which)
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _SOLVES[which] = ref.alps(*orc, x0.copy(), np.zeros(n))
    return _SOLVES[which]


LBFGS_FORMS = TABLE + EVENT_CASES          # run in the two-loop, the compact and the auto form
RUN_CASES = TABLE + EVENT_CASES + OTHER
assert len({c.name for c in RUN_CASES}) == len(RUN_CASES)


def dist(a, b, support=False):
    """max |a - b| relative to the largest entry of b; support: over the entries where both or neither are zero"""
    a, b = a.astype(F64), b.astype(F64)
    if support:
        m = (a != 0) == (b != 0)
        a, b = a[m], b[m]
    scale = float(np.max(np.abs(b), initial=0.0))
    return float(np.max(np.abs(a - b), initial=0.0)) / (scale if scale > 0 else 1.0)


class Pair:
    """the oracle's two roundings over a case's states: `o` plain, `t` the twin f under LongDoubleReducer; sens[j] the
    running distance of x and z through state j + 1; `compared` the number of leading states held to the oracle"""

    def __init__(self, bz, ref, case):
        from tests.test_gpu_parity import LongDoubleReducer
        built = case.build(bz, ref)
        dev, orc, n, ny, mu, y, x0 = built
        tw = (dev, (twin_of(orc[0]),) + tuple(orc[1:]), n, ny, mu, y, x0)
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            self.o, self.t = OracleRun(ref, case, built), OracleRun(ref, case, tw, reducer=LongDoubleReducer())
            for _ in range(case.states - 1):
                self.o.step()
                self.t.step()
        sup = case.g in SUPPORT_G
        self.case, self.sens, self.each = case, [], []
        s = 0.0
        for (xo, zo, _), (xt, zt, _) in zip(self.o.states, self.t.states):
            d = max(dist(xt, xo, sup), dist(zt, zo, sup))
            self.each.append(d)
            s = max(s, d)
            self.sens.append(s)
        self.compared = next((j for j, v in enumerate(self.sens) if 100 * v > 1e-2), case.states)
        # ... and no further than the state before the first step with an unsettled decision (the rule of
        # tests/test_linesearch_host.py: both roundings take the same branches, keep or skip the pair alike, and every
        # margin of a halving or an envelope test exceeds 100 x the difference of the two margins, floored at
        # 10 eps (1 + |FBE|)): from there on the counts have no one value to be held to
        eps = float(np.finfo(case.dtype).eps)
        unsettled = next((j for j, (a, b) in enumerate(zip(self.o.steps, self.t.steps), 1) if not settled(a, b, eps, case.M)), case.states)
        self.by_sens = self.compared
        self.compared = min(self.compared, unsettled) if self.o.start_halvings == self.t.start_halvings else 0
        fp64 = case.dtype == np.float64
        self.tight = sum(1 for v in self.each if v <= (1e-11 if fp64 else 5e-7))

    def tol(self, j):
        return max(1e-9 if self.case.dtype == np.float64 else 5e-5, 100 * self.sens[j])

    def counts(self, j):
        """(tau backtracks, gamma halvings, skipped pairs) of the oracle through state j + 1"""
        s = self.o.steps[:j]
        return (sum(v.nbt for v in s), self.o.start_halvings + sum(v.halvings for v in s), sum(0 if v.kept else 1 for v in s))


_PAIRS = {}


def pair_of(bz, ref, case):
    key = (case.name, case.compact)
    if key not in _PAIRS:
        _PAIRS[key] = Pair(bz, ref, case)
    return _PAIRS[key]


def ids(cases):
    return [c.name for c in cases]


# ------------------------------------------------------------------------------------------------------------ the tests
def test_twins_are_the_oracles_to_rounding_and_exact_on_integers(ref):
    rng = np.random.default_rng(0)
    for dt in BOTH:
        A, b, x = (rng.integers(-2, 3, (7, 12)).astype(dt), rng.integers(-3, 4, 7).astype(dt), rng.integers(-4, 5, 12).astype(dt))
        U = rng.integers(-2, 3, (12, 12))
        Q, q = (U + U.T).astype(dt), rng.integers(-3, 4, 12).astype(dt)
        for f, t in ((ref.LeastSquares(A, b), LeastSquaresTwin(A, b)), (ref.Quadratic(Q, q), QuadraticTwin(Q, q))):
            g1, g2 = np.empty(12, dt), np.empty(12, dt)
            assert f.gradient(g1, x) == t.gradient(g2, x) == f(x) == t(x) and np.array_equal(g1, g2)
            assert g2.dtype == np.dtype(dt) and type(t(x)) == np.dtype(dt).type
        xr = rng.standard_normal(12).astype(dt)
        for f, t in ((ref.LeastSquares(A, b), LeastSquaresTwin(A, b)), (ref.Quadratic(Q, q), QuadraticTwin(Q, q))):
            g1, g2 = np.empty(12, dt), np.empty(12, dt)
            v1, v2 = f.gradient(g1, xr), t.gradient(g2, xr)
            eps = float(np.finfo(dt).eps)
            assert abs(float(v1) - float(v2)) <= 64 * eps * max(1.0, abs(float(v2))) and dist(g1, g2) <= 64 * eps


def test_shapes_reach_the_branches_they_are_named_for():
    R = lambda s, dt: route(s[0], s[1], dt)
    for dt in BOTH:
        assert R((1, 4), dt)["rpc"] == R((1, 4), dt)["nch"] == 1 and R((1, 4), dt)["aligned"]
        assert not R((4, 5), dt)["aligned"] and not R((33, 17), dt)["aligned"] and not R((257, 1031), dt)["aligned"]
        r = R((257, 1028), dt)
        assert r["aligned"] and not r["mfma"] and r["two_pack_threads"] >= 1 and r["one_pack_threads"] >= 1
        r = R((5000, 128), dt)
        assert r["rpc"] == 3 and 0 < r["last_rows"] < 3 and r["fold8"] >= 1 and r["fold_rest"] >= 1
        r = R((70001, 8), dt)
        assert r["row_stride_loop"] and r["aligned"] and not r["mfma"] and r["nch"] >= 2000 and r["fold8"] == 250
        assert r["rpc"] % 2 == 1 and r["rpc"] >= 3          # k_gemv_t: the two-row loop and the odd last row of a chunk
    assert not R((3, 70), F32)["aligned"] and R((3, 70), F64)["aligned"]
    # 257 packs in fp32: thread 0 alone takes the two-pack loop, the others the single-pack loop ; 514 in fp64: every thread
    # the two-pack loop, two of them the single-pack loop behind it
    r32, r64 = R((257, 1028), F32), R((257, 1028), F64)
    assert (r32["npk"], r32["two_pack_threads"], r32["one_pack_threads"]) == (257, 1, 255)
    assert (r64["npk"], r64["two_pack_threads"], r64["one_pack_threads"]) == (514, 256, 2)
    # the MFMA product (fp32, n % 64 == 0): fewer rows than one 8-row step ; several column waves ; rows per chunk = 3, every
    # chunk a ragged tail with masked rows ; rows per chunk = 9, one full 8-row step and a one-row tail
    r = R((7, 64), F32)
    assert r["mfma"] and r["rpc"] < 8
    assert R((260, 1024), F32)["mfma"] and 1024 // 64 > WAVES
    assert R((5000, 128), F32)["mfma"] and R((5000, 128), F32)["rpc"] % 4 != 0
    r = R((16400, 64), F32)
    assert r["mfma"] and r["rpc"] == 9 and r["fold_rest"] >= 1
    # the fold of the row-chunk partials: (70001, 8) has 2001 chunks, 1 + 250 * 8: the eight-at-a-time loop alone.  Its
    # remainder loop runs at (5000, 128) and (16400, 64), asserted above.
    assert R((70001, 8), F64)["fold_rest"] == 0
    # the wide case: over the persistent two-loop's threshold, aligned in fp64, more than one chunk
    r = R(WIDE, F64)
    assert WIDE[1] >= PERSIST_MIN_N and r["aligned"] and r["nch"] > 1
    # Quadratic: no transposed product ; 2052 in fp32 is 513 packs (every thread two packs, thread 0 a third)
    r = route(2052, 2052, F32, transposed=False)
    assert (r["npk"], r["two_pack_threads"], r["one_pack_threads"]) == (513, 256, 1)
    for n, dt in ((512, F64), (1024, F32)):
        r = route(n, n, dt, transposed=False)
        assert (r["npk"], r["two_pack_threads"], r["one_pack_threads"]) == (256, 0, 256)
    # every unaligned shape keeps the pairwise kinds out (n odd) or in (n even) as exact_cases lists them
    assert sum(1 for c in exact_cases() if c[3] in PAIRWISE) == sum(4 for c in exact_cases() if c[3] == "zero" and n_of(c[0], c[1]) % 2 == 0)


EXACT_HOST = [c for c in exact_cases() if c[3] in ("box", "box_vec", "xor", "vc", "cc", "eitheror")]


@pytest.mark.parametrize("case", EXACT_HOST, ids=case_id)
def test_exact_data_is_exact_in_any_summation_order(bz, ref, case):
    kind, shape, dt, D = case
    dev, orc, mu, y, x = gradient_case(bz, ref, kind, shape, dt, D, "exact")
    assert np.all(orc[0].A == np.round(orc[0].A)) if kind == "ls" else np.array_equal(orc[0].Q, orc[0].Q.T)
    g, lx, fx = assert_exact(ref, kind, dt, orc, mu, y, x)
    assert np.all(np.isfinite(g)) and np.any(g)


@pytest.mark.parametrize("case", REAL_SHAPES, ids=case_id)
def test_oracle_meets_the_forward_bound_against_its_twin(bz, ref, case):
    """the oracle's own products (BLAS, its own summation order) are sums in the type taken in some order: they must meet the
    bound the device is held to twice over"""
    kind, shape, dt = case
    dev, orc, mu, y, x = gradient_case(bz, ref, kind, shape, dt, "box", "real")
    g, lx, fx, _ = oracle_gradient(ref, orc, mu, y, x)
    gt, lt, ft, alt = oracle_gradient(ref, orc, mu, y, x, twin=True)
    bound, EL, Ef = forward_bound(kind, dt, orc, mu, y, x, gt, alt)
    ratio = float(np.max(np.abs(g.astype(F64) - gt.astype(F64)) / bound))
    print(f"{case_id(case)}: gradient error / bound {ratio:.3e}, L {abs(float(lx) - float(lt)) / EL:.3e}, f {abs(float(fx) - float(ft)) / Ef:.3e}")
    assert ratio <= 1.0 and abs(float(lx) - float(lt)) <= EL and abs(float(fx) - float(ft)) <= Ef
    assert np.all(bound > 0) and np.all(np.isfinite(bound))


@pytest.mark.parametrize("case", SPECIAL_SHAPES, ids=case_id)
def test_largest_finite_entry_overflows_no_sum(bz, ref, case):
    """x_j = the largest finite number: every sum of magnitudes of a matrix product stays finite, so the NaN / inf pattern of
    the gradient comes from element-wise operations alone and no summation order changes it.  The values: LeastSquares sums
    squares (no cancellation: the class of a sum of non-negative terms has no order) ; Quadratic sums x_i (Q x / 2 + q)_i,
    resp. the oracle's <x, Q x> and <x, q>, whose one term with i = j overflows by itself and whose other terms stay below
    the largest finite number in magnitude, summed — which is why the other entries of x are scaled by 0.02 here (at
    standard normal scale those terms sum to 14 times the largest finite number, and the class of f depends on the order:
    the device gave -inf where the oracle gave NaN).  And |q_j| <= 1 at the special positions: the oracle forms <x, Q x> / 2
    + <x, q> as ProximalOperators does, the device sum x (Q x / 2 + q); where x_j q_j overflows by itself with the sign opposite
    to x_j Q_jj x_j the former is inf - inf = NaN and the latter an infinity (measured: NEXT.md keeps it as an open difference).
    No entry of A or Q is non-finite or zero."""
    kind, shape, dt = case
    dev, orc, mu, y, x = special_case(bz, ref, kind, shape, dt)
    M = (orc[0].A if kind == "ls" else orc[0].Q).astype(LD)
    assert np.all(np.isfinite(M)) and np.all(M != 0)
    big = LD(np.finfo(dt).max)
    for j in special_positions(x.shape[0], dt):
        xs = np.abs(x.astype(LD))
        xs[j] = big
        rows = np.abs(M) @ xs + (np.abs(orc[0].b.astype(LD)) if kind == "ls" else np.abs(orc[0].q.astype(LD)))
        assert np.max(rows) < big
        if kind == "ls":
            assert np.max(rows @ np.abs(M)) < big
        else:
            others = np.arange(x.shape[0]) != j
            assert np.sum(xs[others] * rows[others]) < big and xs[j] * np.abs(M[j, j]) * big > big
            assert abs(float(orc[0].q[j])) <= 1.0


@pytest.mark.parametrize("dt", BOTH, ids=tname)
def test_quadratic_value_at_the_overflow_corner_is_nan_on_the_oracle(bz, ref, dt):
    """ProximalOperators' Quadratic returns <x, Q x> / 2 + <x, q>: with x_0 the largest finite number the first dot is an
    infinity of the sign of Q_00, the second one of the sign of q_0, opposite here, so f = inf - inf = NaN in the type;
    every other term of both dots is finite and their sums of magnitudes stay below the largest finite number.  The twin,
    whose np.longdouble does not overflow at x_0 q_0, rounds the sum once: an infinity of the sign of Q_00, which is what
    the device returns.  The gradient Q x + q is finite in every component."""
    dev, orc, mu, y, x = overflow_corner(bz, ref, dt)
    big = LD(np.finfo(dt).max)
    Q, q, ax = np.abs(orc[0].Q.astype(LD)), np.abs(orc[0].q.astype(LD)), np.abs(x.astype(LD))
    assert orc[0].Q[0, 0] != 0 and np.sign(orc[0].q[0]) == -np.sign(orc[0].Q[0, 0]) and abs(orc[0].q[0]) > 1
    rows = Q @ ax
    assert np.max(rows + q) < big and np.sum(ax[1:] * rows[1:]) < big and np.sum(ax[1:] * q[1:]) < big
    g, lx, fx, _ = oracle_gradient(ref, orc, mu, y, x)
    assert np.isnan(fx) and np.isnan(lx), (fx, lx)
    ft = oracle_gradient(ref, orc, mu, y, x, twin=True)[2]
    assert np.isinf(ft) and np.sign(ft) == np.sign(orc[0].Q[0, 0]), ft
    assert np.all(np.isfinite(oracle_gradient(ref, (orc[0], orc[1], orc[2], ref.FreeSet()), mu, y, x)[0]))


@pytest.mark.parametrize("case", RUN_CASES, ids=ids(RUN_CASES))
def test_oracle_alone_keeps_the_conditions_of_a_run_case(bz, ref, case):
    fp64 = case.dtype == np.float64
    for compact in ((False, True) if case in LBFGS_FORMS else (case.compact,)):
        p = pair_of(bz, ref, case.with_form(compact))
        bt, hv, sk = p.counts(p.compared - 1)
        print(f"{case.name} compact={compact}: compared {p.compared} of {case.states}; tight states {p.tight}; sens at the end of the range "
              f"{p.sens[p.compared - 1]:.3e}; backtracks {bt}, halvings {hv} ({p.o.start_halvings} at the start), skipped pairs {sk}")
        assert p.compared >= 10, (case.name, p.by_sens, p.compared)
        assert p.tight >= (15 if fp64 else 4), (case.name, p.tight)
        if "b" in case.claims:
            assert bt >= 2, (case.name, bt)
        if "h" in case.claims:
            assert hv - p.o.start_halvings >= 1, (case.name, hv)


def test_every_g_and_D_occurs_with_each_f_kind_in_each_type():
    for kind in ("ls", "q"):
        for dt in BOTH:
            names = [c.name.split("-") for c in TABLE if c.kind == kind and c.dtype == np.dtype(dt).type]
            assert {n[3] for n in names} == set(G_KINDS) and {n[4] for n in names} == set(D_KINDS), (kind, dt, names)
    for kind in ("ls", "q"):
        assert any("b" in c.claims and c.kind == kind for c in EVENT_CASES) and any("h" in c.claims and c.kind == kind for c in EVENT_CASES)
        assert {c.direction for c in OTHER if c.kind == kind} == {"anderson", "broyden", "lbfgs"}
        assert any(c.M == 2 for c in OTHER if c.kind == kind)


def test_wide_case_is_compared_over_all_its_states(bz, ref):
    p = pair_of(bz, ref, WIDE_CASE)
    print(f"wide: compared {p.compared} of {WIDE_CASE.states}, sens {p.sens[-1]:.3e}, counts {p.counts(p.compared - 1)}")
    assert p.compared == WIDE_CASE.states and p.sens[-1] <= 1e-11


@pytest.mark.parametrize("which", ["lasso", "qp"])
def test_solve_cases_end_first_order_and_start_above_one(bz, ref, which):
    dev, orc, n, x0 = solve_case(bz, ref, which)
    z = np.empty_like(x0)
    gz = orc[1].prox(z, x0, np.finfo(x0.dtype).eps)
    objx = float(orc[0](z)) + float(gz)
    o = ref_solve(bz, ref, which)
    print(f"{which}: f + g at the start {objx:.6g}; status {o[5]}, outer {o[2]}, inner {o[3]}")
    assert np.any(x0) and objx > 1.0 and o[5] == "first_order" and o[2] >= 2


if __name__ == "__main__":          # the probe the pinned seeds and the event cases came from
    import sys
    import bazinga_jl_amd as bz_
    which = sys.argv[1] if len(sys.argv) > 1 else "table"
    if which == "table":
        for kind in ("ls", "q"):
            for ti, dt in enumerate(BOTH):
                for c in [c for c in TABLE if c.kind == kind and c.dtype == np.dtype(dt).type]:
                    _, s_, t_, g_, D_ = c.name.split("-")
                    shape = tuple(int(v) for v in s_.split("x")) if kind == "ls" else int(s_)
                    for seed in range(40):
                        ps = [Pair(bz_, REF, DenseCase(c.name, dt, run_build(kind, shape, dt, g_, D_, seed), compact=f, kind=kind, g=g_)) for f in (False, True)]
                        if all(p.compared >= 10 and p.tight >= (15 if dt == F64 else 4) for p in ps):
                            break
                    print(repr(c.name) + ":", seed, ", #", [(p.compared, p.tight, p.counts(p.compared - 1)) for p in ps], flush=True)
    else:
        for kind, shape in (("ls", (33, 1024)), ("ls", (257, 1031)), ("q", 514), ("q", 1030)):
            for mode in ((None,) if kind == "ls" else ("convex", "nonconvex")):
                for M in (20, 2):
                    for ys, xs in ((5.0, 3.0), (20.0, 10.0), (1.0, 0.3)):
                        for seed in range(int(which)):
                            c = DenseCase("probe", F64, run_build(kind, shape, F64, "l1", "box", seed, ys=ys, xs=xs, mode=mode), M=M, kind=kind)
                            p = Pair(bz_, REF, c)
                            bt, hv, sk = p.counts(p.compared - 1)
                            if bt >= 2 or hv > p.o.start_halvings:
                                print(kind, shape, mode, "M", M, ys, xs, "seed", seed, "compared", p.compared, "tight", p.tight,
                                      "bt", bt, "hv", hv - p.o.start_halvings, "sk", sk, flush=True)
