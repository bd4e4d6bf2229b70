"""Sparse multinomial (softmax) regression on the device (BZ_F_SPARSE_MULTINOMIAL): f(X) = sum_i w_i (logsumexp_k(t_ik) - t_{i,b_i}),
T = A_f X with A_f in CSR and X n_f x K row-major.  The K-wide row kernels of bz_spmm.h (k_spmm_softmax_r over A_f, k_spmm_t_algrad /
k_spmm_t over A_f', k_spmm_fold for cut rows): creation and refusals through the raw ABI, the gradient bit for bit where the softmax
is exact, against the oracle on real data over every class width and lane map, the three- and four-launch forms, the epilogue
element by element, the iterates and whole solves.

The reference package has no such f: the oracle is the numpy class below (the formulas of include/bazinga_hip.h in the dtype of x,
its sums through ref._dot / ref._sum), driven by the unmodified ref.AugLagFun, ref.PANOCplusIteration and ref.alps, exactly as
GLMOracle is in tests/test_gpu_sparse_glm.py, whose helpers, shapes and tolerances are used here.

`python -m tests.test_gpu_sparse_multinomial` runs the oracle alone (no GPU): it checks the conditions of the exact inputs for every
case and prints the number of tight states of the oracle's own two roundings (see test_iterates_follow_the_oracle)."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_parity import LongDoubleReducer, run_traces
from tests.test_gpu_sparse import CsrOracle, csr_of, sets, structured
from tests.test_gpu_sparse_glm import what_of
from tests.test_gpu_sparse_logistic import IDS, PAIR_IDS, PAIRS, TOL, TYPED, X0, LogisticOracle, one_gradient

pytestmark = pytest.mark.gpu

POW2 = np.array([0.25, 0.5, 1.0, 2.0, 4.0])


def ref_module():
    from oracle import bazinga_ref
    return bazinga_ref


class MultinomialOracle:
    """f(X) = sum_i w^_i ((mx_i - t_{i,b_i}) + log S_i) on a dense A (m x n_f), x the flat row-major X, in the dtype of x;
    gradient A'R with R = w^ (p - onehot(b)).  mx = max_k t, e = exp(t - mx), S = sum_k e, p = e / S.  The row and column
    sums through LogisticOracle.dots (ref._dot under a reducer), S and the value through ref._sum.  w^ is one number or a
    vector, already scaled."""

    def __init__(self, A, labels, K, what=1.0):
        self.A, self.lab, self.K = np.asarray(A), np.asarray(labels).astype(np.int64), K
        self.At = np.ascontiguousarray(self.A.T)
        self.what = what

    def t_of(self, x):
        X = x.reshape(-1, self.K)
        return np.stack([LogisticOracle.dots(self.A, np.ascontiguousarray(X[:, k])) for k in range(self.K)], axis=1)

    def loss_r(self, x):
        ref = ref_module()
        dt = x.dtype.type
        t = self.t_of(x)
        rows = np.arange(t.shape[0])
        w = dt(self.what) if np.ndim(self.what) == 0 else np.asarray(self.what, x.dtype)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            mx = np.max(t, axis=1)
            e = np.exp(t - mx[:, None])
            if isinstance(ref.REDUCER, ref.LocalReducer):
                S = np.sum(e, axis=1, dtype=x.dtype)
            else:
                S = np.array([ref._sum(row) for row in e], x.dtype)
            R = e / S[:, None]
            R[rows, self.lab] -= dt(1)
            loss = w * ((mx - t[rows, self.lab]) + np.log(S))
            return loss, (w[:, None] if np.ndim(w) else w) * R

    def __call__(self, x):
        return x.dtype.type(ref_module()._sum(self.loss_r(x)[0]))

    def gradient(self, y, x):
        loss, R = self.loss_r(x)
        y[...] = np.stack([LogisticOracle.dots(self.At, np.ascontiguousarray(R[:, k])) for k in range(self.K)], axis=1).reshape(-1)
        return x.dtype.type(ref_module()._sum(loss))


def mn_of(bz, A, labels, K, weights=None, scale=1.0, seed=1):
    indptr, indices, data = csr_of(A, np.random.default_rng(seed))
    return bz.SparseMultinomial(indptr, indices, data, labels, A.shape[1], K, weights=weights, scale=scale), indptr, indices, data.shape[0]


# ---- the plan rules of the K-wide kernels, restated: segment length as tests/test_gpu_sparse.plan, lanes under KP * L <= 64
def kp_of(K):
    kp = 2
    while kp < K:
        kp *= 2
    return kp


def plan_k(indptr, nnz, K):
    S = max(512, ((nnz // (2048 * 4) // 4 + 63) // 64) * 64)
    lens = np.diff(indptr)
    segs = np.where(lens > S, -(-lens // S), 1)
    nv = int(segs.sum())
    mean = nnz / nv if nv else 0.0
    L = 1
    while kp_of(K) * L * 2 <= 64 and mean > 4.0 * L:
        L *= 2
    return L, nv, bool(np.any(lens > S))


def transpose_ptr(indices, n):
    return np.concatenate(([0], np.cumsum(np.bincount(indices, minlength=n)))).astype(np.int64)


def form(kernel, K, L, seg):
    return f"{kernel}<K={K},L={L},SEG={int(seg)}>"


# ---- 1. creation and refusals through the raw ABI
def raw_desc(bz, indptr, indices, data, lab, nf, K, slack=0, c=None, ny=None, dtype=np.float64):
    from bazinga_jl_amd.oracles import lower
    m, n = lab.shape[0], nf * K
    good = bz.SparseMultinomial(np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, dtype), np.zeros(m, dtype), nf, K)
    desc, keep = lower(good, bz.NormL1(1.0), c or bz.IdentityFunction(), bz.ZeroSet(), n, ny or n, dtype)
    arrs = (np.ascontiguousarray(indptr, np.int64), np.ascontiguousarray(indices, np.int32), np.ascontiguousarray(data, dtype),
            np.ascontiguousarray(lab, dtype))
    desc.f_sp_rowptr, desc.f_sp_col, desc.f_sp_val, desc.f_b = (a.ctypes.data for a in arrs)
    desc.f_sp_nnz = arrs[1].shape[0]
    desc.slack = slack
    return desc, (keep, arrs)


def test_creation_validates_and_refuses_what_is_not_lowered(bz, ref):
    from bazinga_jl_amd.oracles import lower
    L = bz._lib
    lib = L.load()
    ctx = bz.default_context()
    indptr, indices, data = np.array([0, 2, 3, 5]), np.array([0, 3, 1, 2, 3]), np.arange(1.0, 6.0)
    lab, nf, K = np.array([2.0, 0.0, 1.0]), 4, 3
    n = nf * K

    def create(desc, ctx=ctx):
        h = C.c_void_p()
        rc = lib.bz_problem_create(ctx._h, C.byref(desc), C.byref(h))
        msg = lib.bz_last_error().decode() if rc else ""
        if h.value:
            lib.bz_problem_destroy(h)
        return rc, bool(h.value), msg

    def refused(desc, code, *words, ctx=ctx):
        rc, made, msg = create(desc, ctx)
        assert rc == code and not made and "SparseMultinomial" in msg and all(w in msg for w in words), (rc, msg)

    mk = lambda *a, **kw: raw_desc(bz, *a, **kw)
    desc, keep = mk(indptr, indices, data, lab, nf, K)
    assert desc.f_kind == 10 and desc.f_classes == 3 and create(desc)[:2] == (0, True)
    cs = bz.SparseAffine.from_dense(np.ones((2, n)), np.zeros(2))
    desc, keep = mk(indptr, indices, data, lab, nf, K, c=cs, ny=2)
    assert desc.c_kind == L.BZ_C_SPARSE_AFFINE and create(desc)[:2] == (0, True)
    w = np.array([0.5, 0.0, 2.0])
    desc, keep = mk(indptr, indices, data, lab, nf, K)
    desc.f_w = w.ctypes.data
    assert create(desc)[:2] == (0, True)
    for good_k in (2, 64):                                                         # the ends of the range (n = nf * K)
        desc, keep = mk(indptr, indices, data, np.array([1.0, 0.0, 1.0]), nf, good_k)
        assert create(desc)[:2] == (0, True)
    # K in 2 .. 64, n % K == 0
    for bad in (0, 1, 65, -2):
        desc, keep = mk(indptr, indices, data, lab, nf, K)
        desc.f_classes = bad
        refused(desc, L.BZ_ERR_ARG, "f_classes")
    desc, keep = mk(indptr, indices, data, lab, nf, K)
    desc.f_classes = 5                                                             # 12 % 5 != 0
    refused(desc, L.BZ_ERR_ARG, "multiple")
    # the matrix checks of sp_read; the column indices lie in [0, n / K)
    for bad_ptr, row in ((np.array([0, 3, 2, 5]), "row 1"), (np.array([1, 2, 3, 5]), "row 0")):
        desc, keep = mk(bad_ptr, indices, data, lab, nf, K)
        refused(desc, L.BZ_ERR_ARG, row)
    desc, keep = mk(np.array([0, 2, 3, 4]), indices, data, lab, nf, K)             # rowptr[m] != nnz
    refused(desc, L.BZ_ERR_ARG, "nnz", "row 2")
    desc, keep = mk(indptr, np.array([0, 3, 1, 4, 3]), data, lab, nf, K)           # a column = n_f (< n), in row 2
    refused(desc, L.BZ_ERR_ARG, "column", "row 2")
    desc, keep = mk(indptr, np.array([0, 3, -1, 2, 3]), data, lab, nf, K)
    refused(desc, L.BZ_ERR_ARG, "column", "row 1")
    desc, keep = mk(indptr, indices, data, lab, nf, K)
    desc.f_rows = 0
    refused(desc, L.BZ_ERR_ARG)
    for field in ("f_b", "f_sp_rowptr", "f_sp_col", "f_sp_val"):
        desc, keep = mk(indptr, indices, data, lab, nf, K)
        setattr(desc, field, None)
        refused(desc, L.BZ_ERR_ARG)
    desc, keep = mk(indptr, indices, data, lab, nf, K)
    desc.f_sp_nnz = -1
    refused(desc, L.BZ_ERR_ARG)
    # the labels: finite, integral, in [0, K), with the row
    for bad, row in ((np.array([3.0, 0.0, 1.0]), "row 0"), (np.array([0.0, -1.0, 1.0]), "row 1"), (np.array([0.0, 1.0, 0.5]), "row 2"),
                     (np.array([0.0, np.nan, 1.0]), "row 1"), (np.array([np.inf, 0.0, 1.0]), "row 0")):
        desc, keep = mk(indptr, indices, data, bad, nf, K)
        refused(desc, L.BZ_ERR_ARG, "labels", row)
    # the scale and the weights, as the GLM kind checks them
    for bad in (0.0, -1.0, np.inf, np.nan):
        desc, keep = mk(indptr, indices, data, lab, nf, K)
        desc.f_scale = bad                                                          # (a zeroed field is an error, not a silent 1)
        refused(desc, L.BZ_ERR_ARG, "f_scale")
    for bad, row in ((np.array([1.0, -0.5, 1.0]), "row 1"), (np.array([1.0, 1.0, np.nan]), "row 2"), (np.array([np.inf, 1.0, 1.0]), "row 0")):
        desc, keep = mk(indptr, indices, data, lab, nf, K)
        desc.f_w = bad.ctypes.data
        refused(desc, L.BZ_ERR_ARG, "weights", row)
    # ... finite in the problem's type: in an fp32 problem a finite double can round to +inf
    desc, keep = mk(indptr, indices, data, lab, nf, K, dtype=np.float32)
    assert create(desc)[:2] == (0, True)
    desc.f_scale = 1e300
    refused(desc, L.BZ_ERR_ARG, "f_scale")
    w32 = np.array([1.0, 1.0, 1e30], np.float32)
    desc.f_scale, desc.f_w = 1e30, w32.ctypes.data
    refused(desc, L.BZ_ERR_ARG, "weights", "row 2")
    # the four refusals
    desc, keep = mk(indptr, indices, data, lab, nf, K, slack=1)
    refused(desc, L.BZ_ERR_UNSUPPORTED, "slack")
    desc, keep = mk(indptr, indices, data, lab, nf, K)
    A, b2 = np.ones((2, n)), np.zeros(2)
    desc.c_kind, desc.ny, desc.c_A, desc.c_b = L.BZ_C_DENSE_AFFINE, 2, A.ctypes.data, b2.ctypes.data
    refused(desc, L.BZ_ERR_UNSUPPORTED, "DenseAffine")
    ctx2 = bz.Context(device=0, rank=0, nranks=2, comm_id=None)
    desc, keep = mk(indptr, indices, data, lab, nf, K)
    refused(desc, L.BZ_ERR_UNSUPPORTED, "one rank", ctx=ctx2)
    desc, keep = mk(indptr, indices, data, lab, nf, K)
    desc.g_kind = L.BZ_G_CALLBACK
    refused(desc, L.BZ_ERR_UNSUPPORTED, "callbacks")
    # the other sparse kinds ignore f_classes
    pm = np.array([1.0, -1.0, 1.0])
    for f in (bz.SparseLeastSquares(indptr, indices, data, pm, nf), bz.SparseLogistic(indptr, indices, data, pm, nf),
              bz.SparseGLM(indptr, indices, data, pm, nf, "squared_hinge")):
        desc, keep = lower(f, bz.NormL1(1.0), bz.IdentityFunction(), bz.ZeroSet(), nf, nf, np.float64)
        desc.f_classes = 77
        assert create(desc)[:2] == (0, True)
    # the Python layer raises before any device call
    f = bz.SparseMultinomial(indptr, indices, data, lab, nf, K)
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(f, bz.NormL1(1.0), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64, slack=True)
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(f, bz.NormL1(1.0), bz.DenseAffine(A, np.zeros(2)), bz.ZeroSet(), n, 2, np.float64)


# ---- 2. the gradient bit for bit where the softmax is exact
PATTERN = np.array([1.0, -1.0, -1.0])        # the classes 0, 1, 2 of a planted row of X: the rest are zero


def exact_inputs(m, nf, p, K, ny, dtype, regime):
    """A_f of {-2, -1, 1, 2} under a density-p mask (structured; its empty row 1 gets the entry A[1, 0] = 1: an empty row ties
    all K classes, which is exact only where K is a power of two), labels uniform in [0, K), power-of-two weights, y in [-3, 3],
    mu = 1/4.  "zero": X = 0, so p = 1 / K.  "saturated": the rows of X at a few features J are +-X0 * (1, -1, -1, 0, ...), every
    other entry 0: t_i = X0 tau_i (1, -1, -1, 0, ...) with the integer tau_i = sum_J a_ij sigma_j, so that every e_k is exactly 0 or 1
    and the maximal classes of a row are one (tau > 0), two (tau < 0) or all K (tau = 0).  J holds feature 0 (A's full column) and
    up to seven more; where K is no power of two no tau may be 0, and J shrinks (8, 4, 2, 1 features, 50 draws each) until the
    draw satisfies the conditions that exact_conditions asserts."""
    rng = np.random.default_rng(m * 7 + nf + K)
    A = structured(m, nf, p, rng, True, dtype)
    if m > 2:
        A[1, 0] = 1
    lab = rng.integers(0, K, m).astype(dtype)
    w = POW2[rng.integers(0, 5, m)].astype(dtype)
    y, mu = rng.integers(-3, 4, ny).astype(dtype), np.full(ny, 0.25, dtype)
    X = np.zeros((nf, K), dtype)
    if regime == "saturated":
        pat = np.zeros(K)
        pat[:3] = PATTERN
        A64 = A.astype(np.float64)
        for size in (8, 4, 2, 1):
            for _ in range(50):
                J = np.concatenate(([0], rng.choice(np.arange(2, nf), min(size, nf - 2) - 1, replace=False))) if size > 1 else np.array([0])
                sigma = rng.choice([-1.0, 1.0], J.shape[0])
                tau = A64[:, J] @ sigma
                ok = np.any(tau > 0) and np.any(tau < 0) and (K & (K - 1) == 0 or np.all(tau != 0))
                if ok:
                    break
            if ok:
                break
        X[J] = (X0[dtype] * sigma[:, None] * pat[None, :]).astype(dtype)
    return A, lab, w, X.reshape(-1), y, mu, rng


def exact_conditions(dtype, A, X, K, regime):
    """the conditions of the saturated regime, asserted on the inputs in float64: every t_ik is a multiple of X0 (so every
    e_k = exp(t_ik - mx) is exactly 0 or 1), every row's number of maximal classes is a power of two (so p = 1 / S is exact),
    and both a unique maximum and a tie occur among the rows"""
    t = A.astype(np.float64) @ X.astype(np.float64).reshape(-1, K)
    assert np.exp(dtype(-X0[dtype])) == 0 and np.array_equal(t, X0[dtype] * np.round(t / X0[dtype]))
    nmax = (t == t.max(axis=1, keepdims=True)).sum(axis=1)
    assert np.all(nmax & (nmax - 1) == 0), np.unique(nmax)
    if regime == "saturated":
        assert np.any(nmax == 1) and np.any(nmax > 1), np.unique(nmax)
        assert set(np.unique(np.abs(X))) == {0.0, X0[dtype]}
    else:
        assert not np.any(X) and K & (K - 1) == 0
    return nmax


def assert_exact(dtype, A, X, K, r64, pen64, g_ref, g64):
    """Exactness of the gradient whatever the order of any sum: the entries of A are integers, those of X multiples of X0, the
    weights 2 * 2^j >= 1/2 and p a multiple of 1/8, so every r and every product a r is a multiple of 1/16; the sums of magnitudes
    that bound every partial sum — of a row of A_f X, and of a row of A_f' R plus the penalty part — stay below 2^24 / 160 (fp32) /
    2^53 / 160 (fp64): a tenth of the range in sixteenths.  Then the oracle in dtype has returned what its float64 run returns."""
    lim = 2.0 ** (24 if dtype == np.float32 else 53) / 160
    absA = np.abs(A.astype(np.float64))
    assert np.max(absA @ np.abs(X.astype(np.float64).reshape(-1, K))) < lim
    assert np.max(absA.T @ np.abs(r64)) + pen64 < lim
    assert np.array_equal(r64, np.round(r64 * 16) / 16)
    assert np.array_equal(g_ref.astype(np.float64), g64)


def exact_oracle(bz, ref, dtype, shape, K, D_name, regime, c_pair=None):
    """the inputs and the oracle's gradient in dtype and in float64, with the exactness conditions asserted (no GPU)"""
    m, nf, p = shape
    n = nf * K
    ny = n if c_pair is None else c_pair[0]
    A, lab, w, x, y, mu, rng = exact_inputs(m, nf, p, K, ny, dtype, regime)
    what = what_of(w, 2.0, dtype)
    nmax = exact_conditions(dtype, A, x, K, regime)
    if c_pair is None:
        cd, mk_c, Ac, bc = bz.IdentityFunction(), lambda dt: ref.IdentityFunction(), None, None
    else:
        Ac = structured(ny, n, c_pair[1], rng, True, dtype)
        bc = rng.integers(-3, 4, ny).astype(dtype)
        c_ptr, c_idx, c_val = csr_of(Ac, np.random.default_rng(3))
        cd, mk_c = bz.SparseAffine(c_ptr, c_idx, c_val, bc, n), lambda dt: CsrOracle(c_ptr, c_idx, c_val.astype(dt), bc.astype(dt), n)

    def make_al(dt):
        fo = MultinomialOracle(A.astype(dt), lab, K, np.asarray(what).astype(dt))
        al = ref.AugLagFun(fo, mk_c(dt), sets(bz, ref, D_name, dt)[1], mu.astype(dt), y.astype(dt), x.astype(dt))
        g = np.empty(n, dt)
        return al, al.gradient(g, x.astype(dt)), g, fo
    al, lx, g_ref, fo = make_al(dtype)
    al64, _, g64, fo64 = make_al(np.float64)
    pen = np.abs(al64.yupd) if Ac is None else np.abs(Ac.astype(np.float64)).T @ np.abs(al64.yupd)
    if Ac is not None:
        assert 8 * np.max(np.abs(Ac.astype(np.float64)) @ np.abs(x.astype(np.float64)) + np.abs(bc)) < 2.0 ** (24 if dtype == np.float32 else 53) / 10
    # R and the gradient in exact arithmetic (float64 holds them: the bounds below): p = [t_k = mx] / (the number of maximal
    # classes) — the float64 oracle itself is not exact on the fp32 inputs, where exp(-128) is tiny and not zero in float64
    t64 = A.astype(np.float64) @ x.astype(np.float64).reshape(-1, K)
    r64 = (t64 == t64.max(axis=1, keepdims=True)) / nmax[:, None].astype(np.float64)
    r64[np.arange(A.shape[0]), lab.astype(np.int64)] -= 1.0
    r64 *= (np.asarray(what, np.float64) * np.ones(A.shape[0]))[:, None]
    jtv = al64.yupd if Ac is None else Ac.astype(np.float64).T @ al64.yupd
    g64 = (A.astype(np.float64).T @ r64).reshape(-1) + jtv
    assert_exact(dtype, A, x, K, r64, np.max(pen), g_ref, g64)
    return (A, lab, w, x, y, mu, cd, n, ny), (g_ref, float(lx), float(al.fx)), nmax


def exact_run(bz, ref, dtype, shape, K, D_name, regime, c_pair=None):
    (A, lab, w, x, y, mu, cd, n, ny), (g_ref, lx, fx), _ = exact_oracle(bz, ref, dtype, shape, K, D_name, regime, c_pair)
    f, indptr, indices, nnz = mn_of(bz, A, lab, K, w, 2.0)
    (g_dev, vals), pr = one_gradient(bz, (f, bz.NormL1(1.0), cd, sets(bz, ref, D_name, dtype)[0]), n, ny, dtype, mu, y, x)
    assert g_dev.dtype == dtype and np.array_equal(g_dev, g_ref)
    # (the values: their sums are carried in double on the device and in dtype by the oracle)
    assert abs(vals[0] - lx) <= TOL[dtype] * max(1.0, abs(lx)) and abs(vals[1] - fx) <= TOL[dtype] * max(1.0, abs(fx))
    return g_dev, vals, pr, plan_k(indptr, nnz, K), plan_k(transpose_ptr(indices, A.shape[1]), nnz, K)


EXACT = [("zero", K) for K in (2, 4, 8)] + [("saturated", K) for K in (3, 5, 8)]


@pytest.mark.parametrize("regime,K", EXACT)
@pytest.mark.parametrize("case", TYPED, ids=IDS)
def test_exact_gradient_bit_for_bit(bz, ref, case, regime, K):
    """Integer A in {+-1, +-2}, power-of-two weights and scale 2, mu = 1/4, integer y, D = box; X = 0 (p = 1 / K exactly, K a power
    of two) or saturated (every e_k exactly 0 or 1 and a power-of-two number of maximal classes in every row, asserted on the
    inputs): every product and every sum is exact, so no summation order can change a bit of the gradient, which equals the
    oracle's BIT FOR BIT.  Two row launches, no element-wise kernel."""
    dtype, shape = case
    _, _, pr, (La, _, seg_a), (Lt, _, seg_t) = exact_run(bz, ref, dtype, shape, K, "box", regime)
    assert pr["gemv"]["form"] == form("k_spmm_t_algrad", K, Lt, seg_t), pr["gemv"]["form"]
    assert pr["gemv"]["launches"] == 2 and pr["al_gradient"]["launches"] == 0
    assert pr["misc"]["launches"] == int(seg_a) + int(seg_t)                  # a fold launch per cut matrix


# ---- 3. general gradients on real random data
def special_shapes():
    """(name, A) where the lane map can go wrong"""
    rng = np.random.default_rng(77)
    out = []
    A = structured(41, 37, 0.1, rng, False, np.float64)           # an empty row (1), an empty column (1), a full row and column
    A[2, :] = 0
    A[2, 5] = 1.5                                                  # a row with one entry
    out.append(("41x37", A))
    A = structured(257, 131, 0.3, rng, False, np.float64)         # rows of about 40 entries: longer than 4 L at every L the
    out.append(("257x131", A))                                     # class width leaves; m, n_f no multiples of the rows per workgroup
    out.append(("23x1", rng.standard_normal((23, 1))))             # n_f = 1
    A = structured(600, 19, 0.2, rng, False, np.float64)
    A[:, 3] = 1.0                                                  # a column of ones (an intercept): a row of 600 in A_f', cut
    out.append(("600x19-ones", A))
    A = rng.standard_normal((3, 1200)) * (rng.random((3, 1200)) < 0.9)      # rows of about 1080 entries: A_f cut
    out.append(("3x1200", A))
    return out


SPECIAL = special_shapes()


def real_inputs(A, K, ny, dtype, seed=5):
    rng = np.random.default_rng(seed + A.shape[0] + K)
    m, nf = A.shape
    return (rng.integers(0, K, m).astype(dtype), rng.standard_normal(nf * K).astype(dtype), rng.standard_normal(ny).astype(dtype),
            (10.0 ** rng.uniform(-2, 0, ny)).astype(dtype), rng)


def csr_with_duplicate(A, rng):
    """csr_of, with the first entry of row 0 stored twice (a column index twice in a row: the entry contributes twice)"""
    indptr, indices, data = csr_of(A, rng)
    indices, data = np.insert(indices, 0, indices[0]), np.insert(data, 0, data[0])
    indptr = indptr.copy()
    indptr[1:] += 1
    A2 = A.copy()
    A2[0, indices[0]] *= 2
    return indptr, indices, data, A2


@pytest.mark.parametrize("D", ["zero", "box"])
@pytest.mark.parametrize("K", [2, 3, 5, 8, 33, 64])
@pytest.mark.parametrize("name,A", SPECIAL, ids=[s[0] for s in SPECIAL])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_general_gradient_against_the_oracle_and_between_the_forms(bz, ref, dtype, name, A, K, D, monkeypatch):
    """random real data against the numpy oracle: 1e-12 / 2e-5 of the gradient's largest entry, of max(1, |value|) for the two
    values (the rule and the numbers of tests/test_gpu_sparse_logistic.py).  K = 2, 8, 64 have KP = K (64: a whole wave per
    row), 3 and 5 idle class lanes, 33 a half-idle wave.  The shapes: a row with one entry, an empty row and an empty column, a
    column index twice in a row, rows longer than 4 L entries, m and n_f no multiples of the rows per workgroup, n_f = 1, m = 600
    with a column of ones (A_f' cut), 3 x 1200 at density 0.9 (A_f cut).  And the gradient under BZ_SPLS_FUSED=0 equals the
    default's BIT FOR BIT (the same row sums, the same element operations), with the launch counts (2, 0) and (2, 1)."""
    m, nf = A.shape
    n = nf * K
    indptr, indices, data, A2 = csr_with_duplicate(A.astype(dtype), np.random.default_rng(2))
    lab, x, y, mu, rng = real_inputs(A, K, n, dtype)
    w = rng.uniform(0.5, 1.5, m).astype(dtype)
    Dd, Dr = sets(bz, ref, D, dtype)
    out = {}
    for kind in ("fused", "three"):
        monkeypatch.setenv("BZ_SPLS_FUSED", "0" if kind == "three" else "1")
        f = bz.SparseMultinomial(indptr, indices, data, lab, nf, K, weights=w, scale=1.0 / m)
        out[kind], pr = one_gradient(bz, (f, bz.NormL1(1.0), bz.IdentityFunction(), Dd), n, n, dtype, mu, y, x)
        assert (pr["gemv"]["launches"], pr["al_gradient"]["launches"]) == ((2, 0) if kind == "fused" else (2, 1))
        La, _, seg_a = plan_k(indptr, data.shape[0], K)
        Lt, _, seg_t = plan_k(transpose_ptr(indices, nf), data.shape[0], K)
        assert pr["gemv"]["form"] == form("k_spmm_t_algrad" if kind == "fused" else "k_spmm_t", K, Lt, seg_t), pr["gemv"]["form"]
        assert pr["misc"]["launches"] == int(seg_a) + int(seg_t)
        if name == "600x19-ones":
            assert seg_t and not seg_a
        if name == "3x1200":
            assert seg_a and not seg_t
    al = ref.AugLagFun(MultinomialOracle(A2, lab, K, what_of(w, 1.0 / m, dtype)), ref.IdentityFunction(), Dr, mu.copy(), y.copy(), x)
    g_ref = np.empty(n, dtype)
    lx = float(al.gradient(g_ref, x))
    fx, tol, scale = float(al.fx), TOL[dtype], np.max(np.abs(g_ref))
    (g_dev, vals), (g3, vals3) = out["fused"], out["three"]
    print(f"max|g - g_ref| / max|g_ref| = {np.max(np.abs(g_dev.astype(np.float64) - g_ref)) / scale:.3e}, "
          f"value {abs(vals[0] - lx) / max(1.0, abs(lx)):.3e}, f {abs(vals[1] - fx) / max(1.0, abs(fx)):.3e}, "
          f"forms equal {np.array_equal(g_dev, g3)}")
    assert np.max(np.abs(g_dev.astype(np.float64) - g_ref)) <= tol * scale
    assert abs(vals[0] - lx) <= tol * max(1.0, abs(lx))
    assert abs(vals[1] - fx) <= tol * max(1.0, abs(fx))
    assert np.array_equal(g_dev, g3)
    assert abs(vals3[0] - lx) <= tol * max(1.0, abs(lx)) and vals[1] == vals3[1]


@pytest.mark.parametrize("case", [c for c in TYPED if c[1] in ((257, 1031, 0.06), (1031, 257, 0.02), (41, 121, 0.25), (303, 67, 0.3))], ids=IDS)
def test_general_gradient_on_the_logistic_shapes(bz, ref, case):
    """real data on four of the TYPED shapes (more lane counts on both matrices), K = 5, D = box, no weights"""
    dtype, (m, nf, p) = case
    K = 5
    n = nf * K
    A = structured(m, nf, p, np.random.default_rng(m * 11 + nf), False, dtype)
    lab, x, y, mu, rng = real_inputs(A, K, n, dtype)
    f = mn_of(bz, A, lab, K, seed=2)[0]
    Dd, Dr = sets(bz, ref, "box", dtype)
    (g_dev, vals), pr = one_gradient(bz, (f, bz.NormL1(1.0), bz.IdentityFunction(), Dd), n, n, dtype, mu, y, x)
    al = ref.AugLagFun(MultinomialOracle(A, lab, K), ref.IdentityFunction(), Dr, mu.copy(), y.copy(), x)
    g_ref = np.empty(n, dtype)
    lx = float(al.gradient(g_ref, x))
    assert np.max(np.abs(g_dev.astype(np.float64) - g_ref)) <= TOL[dtype] * np.max(np.abs(g_ref))
    assert abs(vals[0] - lx) <= TOL[dtype] * max(1.0, abs(lx)) and abs(vals[1] - float(al.fx)) <= TOL[dtype] * max(1.0, abs(float(al.fx)))


# ---- 4. pairwise D
def test_pairwise_D_takes_the_three_launch_form(bz, ref):
    """XOR pairs, c = Identity, n even: the projection of an element needs its partner, so the gradient is k_spmm_softmax_r, the
    plain product k_spmm_t and k_algrad_elem whatever BZ_SPLS_FUSED says; within the tolerance of the general test"""
    m, nf, K = 41, 24, 5
    n = nf * K
    A = structured(m, nf, 0.2, np.random.default_rng(4), False, np.float64)
    lab, x, y, mu, _ = real_inputs(A, K, n, np.float64)
    f = mn_of(bz, A, lab, K)[0]
    (g_dev, vals), pr = one_gradient(bz, (f, bz.Zero(), bz.IdentityFunction(), bz.XorPairs()), n, n, np.float64, mu, y, x)
    assert pr["gemv"]["launches"] == 2 and pr["gemv"]["form"].startswith("k_spmm_t<K=5,L=") and pr["al_gradient"]["launches"] == 1
    al = ref.AugLagFun(MultinomialOracle(A, lab, K), ref.IdentityFunction(), ref.PairwiseSet("xor"), mu.copy(), y.copy(), x)
    g_ref = np.empty(n)
    lx = float(al.gradient(g_ref, x))
    assert np.max(np.abs(g_dev - g_ref)) <= 1e-12 * np.max(np.abs(g_ref)) and abs(vals[0] - lx) <= 1e-12 * max(1.0, abs(lx))


# ---- 5. beside a sparse c
@pytest.mark.parametrize("regime,K", [("zero", 4), ("saturated", 3), ("saturated", 8)])
@pytest.mark.parametrize("case", [(t, c) for t in (np.float64, np.float32) for c in PAIRS], ids=PAIR_IDS)
def test_exact_gradient_beside_a_sparse_c(bz, ref, case, regime, K):
    """the four-launch form beside c(x) = A_c x - b_c in CSR with another row count: bit for bit the oracle's on the exact data"""
    dtype, (shape, c_pair) = case
    _, _, pr, _, _ = exact_run(bz, ref, dtype, shape, K, "box", regime, c_pair)
    assert pr["gemv"]["launches"] == 4 and pr["al_gradient"]["launches"] == 0
    assert pr["gemv"]["form"].startswith("k_spmv_t_finish<L="), pr["gemv"]["form"]


@pytest.mark.parametrize("case", [(t, c) for t in (np.float64, np.float32) for c in PAIRS], ids=PAIR_IDS)
def test_general_gradient_beside_a_sparse_c(bz, ref, case):
    dtype, ((m, nf, p), (ny, pc)) = case
    K = 5
    n = nf * K
    rng = np.random.default_rng(m + ny)
    A = structured(m, nf, p, rng, False, dtype)
    Ac = structured(ny, n, pc, rng, False, dtype)
    bc = rng.standard_normal(ny).astype(dtype)
    lab, x, y, mu, _ = real_inputs(A, K, ny, dtype)
    c_ptr, c_idx, c_val = csr_of(Ac, np.random.default_rng(3))
    f = mn_of(bz, A, lab, K)[0]
    Dd, Dr = sets(bz, ref, "box", dtype)
    (g_dev, vals), pr = one_gradient(bz, (f, bz.NormL1(1.0), bz.SparseAffine(c_ptr, c_idx, c_val, bc, n), Dd), n, ny, dtype, mu, y, x)
    assert pr["gemv"]["launches"] == 4 and pr["al_gradient"]["launches"] == 0
    al = ref.AugLagFun(MultinomialOracle(A, lab, K), CsrOracle(c_ptr, c_idx, c_val, bc, n), Dr, mu.copy(), y.copy(), x)
    g_ref = np.empty(n, dtype)
    lx = float(al.gradient(g_ref, x))
    assert np.max(np.abs(g_dev.astype(np.float64) - g_ref)) <= TOL[dtype] * np.max(np.abs(g_ref))
    assert abs(vals[0] - lx) <= TOL[dtype] * max(1.0, abs(lx)) and abs(vals[1] - float(al.fx)) <= TOL[dtype] * max(1.0, abs(float(al.fx)))


# ---- 6. the epilogue element by element
def epilogue_t(m, K, dtype):
    """T (m x K): row i of the identity-pattern A_f touches feature i alone, so with A_f = I and X = T, t_ik = X[i, k]"""
    rng = np.random.default_rng(31 + K)
    T = rng.uniform(-30.0, 30.0, (m, K))
    T[::5] *= 0.01                                                  # near-uniform rows
    T[1::7] *= 20.0                                                 # rows far apart: p underflows in the losing classes
    return T.astype(dtype)


@pytest.mark.parametrize("wmode", ["none", "uniform", "vector"])
@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_epilogue_element_by_element(bz, ref, dtype, K, wmode):
    """A_f = I (m = n_f = 300), X = T: t_ik = T[i, k].  mu = 1, y = 0, D = free: the penalty part of the gradient is zero and
    grad[i, k] = 1 * r_ik, so R is read off the gradient.  Per element |r_dev - r_ref| <= 16 eps w^_i: p = e / S carries the
    roundings of t - mx (none: same operation), exp (about an ulp on each side), the K-term sum (K - 1 roundings in another
    order) and the quotient, all relative to p <= 1, and p - [k = b] one more: a few ulps of w^, not of r, which cancels at the
    label.  No weights, the uniform 0.25, a vector with zeros in it and the scale 1/3.  The losses of six rows one by one,
    through one-hot weight vectors, within 8 eps max(1, |loss|)."""
    m = 300
    T = epilogue_t(m, K, dtype)
    rng = np.random.default_rng(3)
    lab = rng.integers(0, K, m).astype(dtype)
    weights, scale = {"none": (None, 1.0), "uniform": (None, 0.25),
                      "vector": (np.resize(np.array([1.0, 0.0, 0.3, 2.5, 0.0], dtype), m), 1.0 / 3.0)}[wmode]
    n = m * K
    x, y, mu = T.reshape(-1), np.zeros(n, dtype), np.ones(n, dtype)
    rest = (bz.Zero(), bz.IdentityFunction(), bz.FreeSet())
    ident = (np.arange(m + 1), np.arange(m), np.ones(m, dtype))
    f = bz.SparseMultinomial(*ident, lab, m, K, weights=weights, scale=scale)
    (g_dev, vals), pr = one_gradient(bz, (f, *rest), n, n, dtype, mu, y, x)
    what = what_of(weights, scale, dtype)
    fo = MultinomialOracle(np.eye(m, dtype=dtype), lab, K, what)
    loss_ref, R_ref = fo.loss_r(x)
    eps = float(np.finfo(dtype).eps)
    wcol = (np.asarray(what, np.float64) * np.ones(m))[:, None]
    err = np.abs(g_dev.reshape(m, K).astype(np.float64) - R_ref.astype(np.float64))
    print(f"max |r_dev - r_ref| / (eps w) = {np.max(err[wcol[:, 0] > 0] / (eps * wcol[wcol[:, 0] > 0])):.2f}")
    assert g_dev.dtype == dtype and np.all(err <= 16 * eps * wcol)
    fx = float(ref._sum(loss_ref))
    assert abs(vals[1] - fx) <= TOL[dtype] * max(1.0, abs(fx)) and vals[0] == vals[1]
    for i in (0, 1, 5, 8, 150, 299):
        onehot = np.zeros(m, dtype)
        onehot[i] = 2.0
        fi = bz.SparseMultinomial(*ident, lab, m, K, weights=onehot, scale=0.5)
        (_, vi), _ = one_gradient(bz, (fi, *rest), n, n, dtype, mu, y, x)
        li = float(MultinomialOracle(np.eye(m, dtype=dtype), lab, K, dtype(1)).loss_r(x)[0][i])
        assert abs(vi[1] - li) <= 8 * eps * max(1.0, abs(li)), (i, vi[1], li)


@pytest.mark.parametrize("K", [3, 8])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_epilogue_edge_values(bz, ref, dtype, K):
    """A_f = I, X = T.  A NaN in one class of one row reaches that row's K entries of R and the value, and no other row (also
    where the NaN sits in the class the ordered max drops, and in an idle-lane neighbour's place, class K - 1); t = +inf gives
    NaN (inf - inf); very negative t in all but one class gives p exactly one-hot: r = w (onehot - [k = b]) bit for bit; an empty
    row gives the loss w log K, and t = 0 gives p = 1 / K."""
    m = 8
    n = m * K
    rest = (bz.Zero(), bz.IdentityFunction(), bz.FreeSet())
    y, mu = np.zeros(n, dtype), np.ones(n, dtype)
    lab = (np.arange(m) % K).astype(dtype)
    big = dtype(-1e4)

    def run(T, ptr=None):
        f = bz.SparseMultinomial(np.arange(m + 1) if ptr is None else ptr, np.arange(m if ptr is None else ptr[-1]),
                                 np.ones(m if ptr is None else ptr[-1], dtype), lab, m, K, scale=0.5)
        (g, vals), _ = one_gradient(bz, (f, *rest), n, n, dtype, mu, y, T.reshape(-1).astype(dtype))
        return g.reshape(m, K), vals
    base = np.random.default_rng(9).uniform(-3, 3, (m, K))
    for row, cls in ((2, 0), (3, K - 1), (5, 1)):
        T = base.copy()
        T[row, cls] = np.nan
        R, vals = run(T)
        assert np.all(np.isnan(R[row])) and np.isnan(vals[1]) and np.isnan(vals[0])
        assert np.all(np.isfinite(np.delete(R, row, axis=0)))
    T = base.copy()
    T[4, 1] = np.inf
    R, vals = run(T)
    assert np.all(np.isnan(R[4])) and np.isnan(vals[1]) and np.all(np.isfinite(np.delete(R, 4, axis=0)))
    T = np.full((m, K), big)
    win = (np.arange(m) * 3 + 1) % K
    T[np.arange(m), win] = 0.0
    R, vals = run(T)
    onehot = lambda c: (np.arange(K)[None, :] == c[:, None]).astype(dtype)
    assert np.array_equal(R, dtype(0.5) * (onehot(win) - onehot(lab.astype(np.int64))))
    assert vals[1] == float(np.sum(np.where(win == lab, 0.0, 0.5 * 1e4)))
    # rows 6 and 7 empty (t = 0 whatever X holds): their loss is w log K; columns 6 and 7 are empty too: a zero gradient there
    ptr = np.concatenate((np.arange(7), [6, 6]))
    R, vals = run(base, ptr)
    eps = float(np.finfo(dtype).eps)
    fo = MultinomialOracle(np.diag(np.r_[np.ones(6), 0.0, 0.0]).astype(dtype), lab, K, dtype(0.5))
    loss_ref = fo.loss_r(base.reshape(-1).astype(dtype))[0].astype(np.float64)
    assert np.all(np.abs(loss_ref[6:] - 0.5 * np.log(K)) <= 4 * eps) and not np.any(R[6:])
    assert abs(vals[1] - float(np.sum(loss_ref))) <= 8 * eps * float(np.sum(loss_ref))
    # ... and p = 1 / K at t = 0, read off the gradient with X = 0
    R, vals = run(np.zeros((m, K)))
    want = 0.5 * (1.0 / K - onehot(lab.astype(np.int64)).astype(np.float64))
    assert np.max(np.abs(R.astype(np.float64) - want)) <= 2 * eps
    assert abs(vals[1] - m * 0.5 * np.log(K)) <= 8 * eps * m * 0.5 * np.log(K)


# ---- 7. the empty matrix
@pytest.mark.parametrize("K", [3, 4])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_empty_matrix(bz, ref, dtype, K):
    """nnz = 0 is accepted: every t is 0, f = sum_i w^_i log K and the gradient is the penalty part alone, bit for bit on
    integer data"""
    m, nf = 23, 37
    n = nf * K
    rng = np.random.default_rng(8)
    lab = rng.integers(0, K, m).astype(dtype)
    w = POW2[rng.integers(0, 5, m)].astype(dtype)
    x, y = (rng.integers(-3, 4, k).astype(dtype) for k in (n, n))
    mu = np.full(n, 0.25, dtype)
    f = bz.SparseMultinomial(np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, dtype), lab, nf, K, weights=w, scale=0.5)
    Dd, Dr = sets(bz, ref, "box", dtype)
    (g_dev, vals), _ = one_gradient(bz, (f, bz.NormL1(1.0), bz.IdentityFunction(), Dd), n, n, dtype, mu, y, x)
    fo = MultinomialOracle(np.zeros((m, nf), dtype), lab, K, what_of(w, 0.5, dtype))
    al = ref.AugLagFun(fo, ref.IdentityFunction(), Dr, mu.copy(), y.copy(), x)
    g_ref = np.empty(n, dtype)
    lx = float(al.gradient(g_ref, x))
    assert np.array_equal(g_dev, g_ref) and np.array_equal(g_dev, al.yupd)
    want = float(np.sum(0.5 * w.astype(np.float64))) * np.log(K)
    assert abs(vals[1] - want) <= TOL[dtype] * want
    assert abs(vals[0] - lx) <= TOL[dtype] * max(1.0, abs(lx))


# ---- 8. launches and identical runs
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_launches_of_two_gradients_and_identical_runs(bz, ref, dtype):
    """two gradients: four row launches with c = Identity, eight beside a sparse c, none from k_algrad_elem; the same bits on
    both runs; the bytes of the model: the matrix once per pass and the K-wide vectors"""
    m, nf, K = 257, 100, 5
    n = nf * K
    A = structured(m, nf, 0.05, np.random.default_rng(6), False, dtype)
    lab, x, y, mu, rng = real_inputs(A, K, n, dtype)
    w = rng.uniform(0.5, 1.5, m).astype(dtype)
    f, indptr, indices, nnz = mn_of(bz, A, lab, K, w, 1.0 / m)
    runs, pr = one_gradient(bz, (f, bz.NormL1(1.0), bz.IdentityFunction(), bz.ZeroSet()), n, n, dtype, mu, y, x, times=2)
    assert pr["gemv"]["launches"] == 4 and pr["al_gradient"]["launches"] == 0 and pr["misc"]["launches"] == 0
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    sz = np.dtype(dtype).itemsize
    La, nva, _ = plan_k(indptr, nnz, K)
    Lt, nvt, _ = plan_k(transpose_ptr(indices, nf), nnz, K)
    # per pass: the entries and the row pointers once, the gathered K-wide vector once; A_f: labels, weights and R (m K); A_f':
    # x, mu, mu y and the gradient (n each)
    model = 2 * nnz * (sz + 4) + (nva + 1) * 8 + (nvt + 1) * 8 + (n + m * K) * sz + (2 * m + m * K) * sz + 4 * n * sz
    assert pr["gemv"]["bytes"] == 2 * model, (pr["gemv"], model)
    ny = 41
    Ac = structured(ny, n, 0.1, rng, False, dtype)
    c_ptr, c_idx, c_val = csr_of(Ac, np.random.default_rng(3))
    dev = (f, bz.NormL1(1.0), bz.SparseAffine(c_ptr, c_idx, c_val, rng.standard_normal(ny).astype(dtype), n), sets(bz, ref, "box", dtype)[0])
    runs, pr = one_gradient(bz, dev, n, ny, dtype, mu[:ny], y[:ny], x, times=2)
    assert pr["gemv"]["launches"] == 8 and pr["al_gradient"]["launches"] == 0
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


# ---- 9. the iterates
def mn_problem(bz, ref, shape, dtype, weighted=False, beside_c=False, lam=0.5, hi=0.5):
    """sparse_multinomial(m, n_f, K): NormL1(lam), c = Identity, D = box(-5, hi), plain or with the weights 0.5 + u11 and the
    scale 1 / m; or beside the constraints of budget_bands(n, 10) with g = IndBox(0, 1).
    hi = 0.5: PANOCplus estimates its first step size from grad L(x0 + 1) - grad L(x0), and adding one number to the K classes
    of every feature leaves the softmax — f and grad f — unchanged; with x0 = 0 and a box that holds both 0 and 1 the penalty
    is flat there too, the estimate is 0 and gamma = alpha / 0 on the device and in the reference alike.  With the upper bound
    0.5 the probe point leaves the box and the estimate is the penalty's; the step-size halvings then do the rest."""
    m, nf, K = shape
    n = nf * K
    d = bz.synth.sparse_multinomial(m, nf, K, 5, dtype)
    w = (0.5 + bz.synth.uniform(11, m)).astype(dtype) if weighted else None
    scale = 1.0 / m if weighted else 1.0
    f = bz.SparseMultinomial(d["indptr"], d["indices"], d["data"], d["labels"], nf, K, weights=w, scale=scale)
    fo = MultinomialOracle(f.toarray(), d["labels"], K, what_of(w, scale, dtype))
    if not beside_c:
        dev = (f, bz.NormL1(lam), bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(-5.0, hi)))
        orc = (fo, ref.NormL1(lam), ref.IdentityFunction(), ref.ClosedSet(ref.IndBox(dtype(-5), dtype(hi))))
        return n, n, dev, orc
    bb = bz.synth.budget_bands(n, 10, dtype)
    csr = (bb["indptr"], bb["indices"], bb["data"], bb["b"], n)
    dev = (f, bz.IndBox(0.0, 1.0), bz.SparseAffine(*csr), bz.ClosedSet(bz.IndBox(bb["lo"], bb["hi"])))
    orc = (fo, ref.IndBox(dtype(0), dtype(1)), CsrOracle(*csr), ref.ClosedSet(ref.IndBox(bb["lo"], bb["hi"])))
    return n, 11, dev, orc


# (shape, dtype, weighted, beside a sparse c) -> the tight states asked of the device (see the docstring below)
STATES = [((256, 16, 4), np.float64, False, False, 28), ((256, 12, 3), np.float64, False, False, 28),
          ((256, 16, 4), np.float32, False, False, 7), ((256, 12, 3), np.float32, False, False, 3),
          ((256, 16, 4), np.float64, True, False, 28), ((256, 12, 3), np.float64, False, True, 28)]
STATE_IDS = [f"{s[0][0]}x{s[0][1]}x{s[0][2]}-{'f64' if s[1] is np.float64 else 'f32'}{'-weighted' if s[2] else ''}{'-sparse_c' if s[3] else ''}"
             for s in STATES]
BASE = {np.float64: 1e-9, np.float32: 5e-5}


def oracle_tight_states(bz, ref, shape, dtype, weighted, beside_c, iters=30):
    """the oracle alone: the states among `iters` at which its own two roundings (plain and extended-precision sums) are
    within base / 100 of each other — where the rule max(base, 100 sens) asks the device for `base`"""
    n, ny, dev, orc = mn_problem(bz, ref, shape, dtype, weighted, beside_c, lam=0.5 / 256 if weighted else 0.5)
    mu, y = np.full(ny, 0.1, dtype), (0.1 * np.random.default_rng(2).standard_normal(ny)).astype(dtype)
    x0 = np.zeros(n, dtype)
    eps = float(np.finfo(dtype).eps)
    its, sts = [], []
    for red in (None, LongDoubleReducer()):
        ref.set_reducer(red)
        al = ref.AugLagFun(orc[0], orc[2], orc[3], mu.copy(), y.copy(), x0)
        it = ref.PANOCplusIteration(al, ref.NonsmoothCostFun(orc[1]), x0, minimum_gamma=eps)
        its.append(it)
        sts.append(it.init())
    ref.set_reducer(None)
    env, tight = 0.0, 0
    err = lambda a, b: float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64))) / max(1.0, float(np.max(np.abs(b)))))
    for k in range(iters):
        env = max(env, err(sts[1].x, sts[0].x), err(sts[1].z, sts[0].z))
        assert np.isfinite(env) and np.isfinite(float(sts[0].gamma)) and np.all(np.isfinite(sts[0].x))
        tight += 100 * env <= BASE[dtype]
        if k + 1 < iters:
            sts[0] = its[0].step(sts[0])
            ref.set_reducer(LongDoubleReducer())
            sts[1] = its[1].step(sts[1])
            ref.set_reducer(None)
    return tight


@pytest.mark.parametrize("shape,dtype,weighted,beside_c,tight", STATES, ids=STATE_IDS)
def test_iterates_follow_the_oracle(bz, ref, shape, dtype, weighted, beside_c, tight):
    """30 states: x and z inside max(base, 100 * sens) — base 1e-9 / 5e-5, sens the oracle's own extended-precision
    envelope — and gamma equal to 1e-12 / 1e-5 relative: the rule and the numbers of tests/test_gpu_sparse_logistic.py.
    The number of states at which the device is asked for `base` itself: the oracle's own two roundings, run alone on a CPU
    (`python -m tests.test_gpu_sparse_multinomial`), stay within base / 100 of each other on 30 of 30 states in the four fp64
    cases, on 9 of 30 for (256, 16, 4) in fp32 and on 5 of 30 for (256, 12, 3) in fp32; asked for: 28, 7 and 3, a margin of two
    states under each count."""
    n, ny, dev, orc = mn_problem(bz, ref, shape, dtype, weighted, beside_c, lam=0.5 / 256 if weighted else 0.5)
    mu, y = np.full(ny, 0.1, dtype), (0.1 * np.random.default_rng(2).standard_normal(ny)).astype(dtype)
    x0 = np.zeros(n, dtype)
    eps = float(np.finfo(dtype).eps)
    prob, st, rows = run_traces(bz, ref, dev, orc, n, mu, y, x0, 30, minimum_gamma=eps, dtype=dtype, ny=ny)
    pr = prob.profile2()
    stats = prob.panoc_stats()
    prob.close()
    base = BASE[dtype]
    for k, ex, ez, g_d, g_r, sn_d, sn_r, fused, sens in rows:
        print(f"k={k} ex={ex:.3e} ez={ez:.3e} gamma {g_d:.9g} / {g_r:.9g} sens={sens:.3e}")
    print(f"gamma halvings {int(stats.n_gamma_halvings)}, tau backtracks {int(stats.n_backtracks)} in 30 states")
    for k, ex, ez, g_d, g_r, sn_d, sn_r, fused, sens in rows:
        assert np.isfinite(g_r) and abs(g_d - g_r) <= (1e-12 if dtype == np.float64 else 1e-5) * g_r, k
        assert ex <= max(base, 100 * sens) and ez <= max(base, 100 * sens), (k, ex, ez, sens)
    assert sum(1 for r in rows if r[1] <= base and r[2] <= base) >= tight
    assert pr["gemv"]["form"].startswith("k_spmm_" if not beside_c else "k_spmv_t_finish"), pr["gemv"]["form"]
    assert pr["k_fused_iterates"]["launches"] == 0 and pr["k_fused_sep"]["launches"] == 0


# ---- 10. whole solves
@pytest.mark.parametrize("vector", [False, True], ids=["lambda", "lambda_vec"])
def test_whole_solves(bz, ref, vector):
    """bz.alps, resident and through the host outer loop, against ref.alps on sparse_multinomial(256, 16, 4) with
    g = NormL1(0.5), and with a vector lambda whose first feature's K coefficients (the intercept's row of X) are unpenalised:
    status and outer count equal, x within 1e-4 (the bound of the GLM whole-solve test).  set_g_lambda followed by a solve equals
    the solve of a fresh problem bit for bit.
    D = box(-5, 5), which holds x0 = 0 and the step-size probe x0 + 1: the estimate would be 0 (mn_problem's docstring), so the
    subsolver is given its first step size, gamma = 0.1 with adaptive = True (the reference's own keywords), on both sides."""
    shape = (256, 16, 4)
    K = shape[2]
    n, ny, dev, orc = mn_problem(bz, ref, shape, np.float64, hi=5.0)
    lam = 0.5
    if vector:
        lam = np.full(n, 0.5)
        lam[:K] = 0.0
        dev = (dev[0], bz.NormL1(lam)) + dev[2:]
        orc = (orc[0], ref.NormL1(lam)) + orc[2:]
    sub = lambda **kw: bz.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, gamma=0.1, adaptive=True, **kw)
    subr = lambda **kw: ref.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, gamma=0.1, adaptive=True, **kw)
    o = ref.alps(*orc, np.zeros(n), np.zeros(ny), subsolver=subr, subsolver_maxit=100000)
    assert o[5] == "first_order"
    for resident in (True, False):
        a = bz.alps(*dev, np.zeros(n), np.zeros(ny), subsolver=sub, subsolver_maxit=100000, resident=resident)
        print(f"vector={vector} resident={resident}: status {a[5]} outer {a[2]}/{o[2]} inner {a[3]}/{o[3]} "
              f"max|x - x_ref| {np.max(np.abs(a[0] - o[0])):.3e}")
        assert a[5] == o[5] and a[2] == o[2]
        assert np.max(np.abs(a[0] - o[0])) <= 1e-4
    # lambda set on a live problem: a solve at another lambda first, then the setter, then the solve
    other = 0.3 if not vector else 0.6 * lam + 0.1
    live = bz.Problem(dev[0], bz.NormL1(other), *dev[2:], n, ny, np.float64)
    first = bz.alps(dev[0], bz.NormL1(other), *dev[2:], np.zeros(n), np.zeros(ny), subsolver=sub, subsolver_maxit=100000, problem=live)
    live.set_g_lambda(lam)
    again = bz.alps(*dev, np.zeros(n), np.zeros(ny), subsolver=sub, subsolver_maxit=100000, problem=live)
    live.close()
    fresh = bz.alps(*dev, np.zeros(n), np.zeros(ny), subsolver=sub, subsolver_maxit=100000, resident=True)
    assert np.array_equal(again[0], fresh[0]) and np.array_equal(again[1], fresh[1]) and again[2:4] == fresh[2:4]
    assert not np.array_equal(first[0], fresh[0])


if __name__ == "__main__":
    # the oracle alone, no GPU: the conditions of the exact inputs, and the tight states of the oracle's own two roundings
    import bazinga_jl_amd as bz_
    ref_ = ref_module()
    for regime, K in EXACT:
        for dtype, shape in TYPED:
            _, _, nmax = exact_oracle(bz_, ref_, dtype, shape, K, "box", regime)
            print(f"{regime} K={K} {IDS((dtype, shape))}: maximal classes per row {dict(zip(*np.unique(nmax, return_counts=True)))}")
    for (shape, c_pair) in PAIRS:
        for dtype in (np.float64, np.float32):
            for regime, K in (("zero", 4), ("saturated", 3), ("saturated", 8)):
                exact_oracle(bz_, ref_, dtype, shape, K, "box", regime, c_pair)
    print("exact inputs: all conditions hold")
    for sid, (shape, dtype, weighted, beside_c, tight) in zip(STATE_IDS, STATES):
        print(f"{sid}: {oracle_tight_states(bz_, ref_, shape, dtype, weighted, beside_c)} of 30 states tight in the oracle; {tight} asked")
