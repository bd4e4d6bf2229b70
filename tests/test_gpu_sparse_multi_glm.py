"""The sparse multi-response GLM f on the device (BZ_F_SPARSE_MULTI_GLM): f(X) = sum_i w_i sum_k l(B_ik, t_ik), T = A_f X with A_f in
CSR, X n_f x K and B m x K row-major.  The K-wide row kernels of bz_spmm.h with K independent row losses as the epilogue
(k_spmm_glm_r<LOSS> over A_f, k_spmm_t_algrad / k_spmm_t over A_f', k_spmm_fold for cut rows): creation and refusals through the raw
ABI, the gradient bit for bit on exact data and against K scalar SparseGLM problems, against the oracle on real data over every
width and lane map, the isolation of a row's K responses, the epilogue element by element, the iterates and whole solves.

The reference package has no such f: the oracle is the numpy class below (GLMOracle's formulas on the K columns of T, its sums
through ref._dot / ref._sum), driven by the unmodified ref.AugLagFun, ref.PANOCplusIteration and ref.alps.  The helpers, shapes,
rules and numbers are those of tests/test_gpu_sparse_multinomial.py and tests/test_gpu_sparse_glm.py, imported from there.

`python -m tests.test_gpu_sparse_multi_glm` runs the oracle alone (no GPU): the conditions of the exact inputs for every case, the
tight states of the oracle's own two roundings (see test_iterates_follow_the_oracle) and the whole solves' lambdas."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_parity import LongDoubleReducer, _err, run_traces
from tests.test_gpu_sparse import CsrOracle, csr_of, sets, structured
from tests.test_gpu_sparse_glm import DELTA, LOSSES, POW2, GLMOracle, what_of
from tests.test_gpu_sparse_logistic import IDS, PAIR_IDS, PAIRS, TOL, TYPED, X0, LogisticOracle, one_gradient
from tests.test_gpu_sparse_multinomial import BASE, SPECIAL, csr_with_duplicate, form, plan_k, transpose_ptr

pytestmark = pytest.mark.gpu

F64_F32 = pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])


def ref_module():
    from oracle import bazinga_ref
    return bazinga_ref


class MultiGLMOracle:
    """f(X) = sum_i w^_i sum_k l(B_ik, t_ik) on a dense A (m x n_f), x the flat row-major X, in the dtype of x; gradient A'R with
    R = w^ l'.  l and l' are GLMOracle.terms on T (m x K); the row and column sums through LogisticOracle.dots (ref._dot under
    a reducer) and the value through ref._sum (least squares: halved once).  w^ is one number or a vector with one entry per
    ROW, already scaled."""

    def __init__(self, A, B, loss, delta=None, what=1.0):
        self.A, self.B = np.asarray(A), np.asarray(B)
        self.K = self.B.shape[1]
        self.At = np.ascontiguousarray(self.A.T)
        self.loss, self.delta, self.what = loss, delta, what

    def t_of(self, x):
        X = x.reshape(-1, self.K)
        return np.stack([LogisticOracle.dots(self.A, np.ascontiguousarray(X[:, k])) for k in range(self.K)], axis=1)

    def loss_r(self, x):
        dt = x.dtype.type
        l, dl = GLMOracle.terms(self, self.B.astype(x.dtype, copy=False), self.t_of(x))
        w = dt(self.what) if np.ndim(self.what) == 0 else np.asarray(self.what, x.dtype)[:, None]
        with np.errstate(over="ignore", invalid="ignore"):
            return w * l, w * dl

    def value(self, terms, dt):
        fx = dt(ref_module()._sum(np.ascontiguousarray(terms).reshape(-1)))
        return dt(0.5) * fx if self.loss == "least_squares" else fx

    def __call__(self, x):
        return self.value(self.loss_r(x)[0], x.dtype.type)

    def gradient(self, y, x):
        terms, R = self.loss_r(x)
        y[...] = np.stack([LogisticOracle.dots(self.At, np.ascontiguousarray(R[:, k])) for k in range(self.K)], axis=1).reshape(-1)
        return self.value(terms, x.dtype.type)


def B_of(loss, rng, m, K, dtype, real=False):
    """labels +-1, counts 0 .. 3, and for the two regression losses integers of [-3, 3] (real: standard normal numbers)"""
    if loss in ("logistic", "squared_hinge"):
        return np.where(rng.random((m, K)) < 0.5, -1.0, 1.0).astype(dtype)
    if loss == "poisson":
        return rng.integers(0, 4, (m, K)).astype(dtype)
    return (rng.standard_normal((m, K)) if real else rng.integers(-3, 4, (m, K))).astype(dtype)


def delta_of(loss):
    return DELTA if loss == "huber" else None


def mg_of(bz, A, B, loss, weights=None, scale=1.0, seed=1):
    indptr, indices, data = csr_of(A, np.random.default_rng(seed))
    f = bz.SparseMultiGLM(indptr, indices, data, B, A.shape[1], loss, delta=delta_of(loss), weights=weights, scale=scale)
    return f, indptr, indices, data.shape[0]


# ---- 1. creation and refusals through the raw ABI
def raw_desc(bz, indptr, indices, data, B, nf, loss="huber", delta=1.0, slack=0, c=None, ny=None, dtype=np.float64):
    from bazinga_jl_amd.oracles import lower
    m, K = B.shape
    n = nf * K
    good = bz.SparseMultiGLM(np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, dtype), B.astype(dtype), nf, loss, delta=delta)
    desc, keep = lower(good, bz.NormL1(1.0), c or bz.IdentityFunction(), bz.ZeroSet(), n, ny or n, dtype)
    arrs = (np.ascontiguousarray(indptr, np.int64), np.ascontiguousarray(indices, np.int32), np.ascontiguousarray(data, dtype))
    desc.f_sp_rowptr, desc.f_sp_col, desc.f_sp_val = (a.ctypes.data for a in arrs)
    desc.f_sp_nnz = arrs[1].shape[0]
    desc.slack = slack
    return desc, (keep, arrs)


def test_creation_validates_and_refuses_what_is_not_lowered(bz, ref):
    from bazinga_jl_amd.oracles import lower
    L = bz._lib
    lib = L.load()
    ctx = bz.default_context()
    indptr, indices, data = np.array([0, 2, 3, 5]), np.array([0, 3, 1, 2, 3]), np.arange(1.0, 6.0)
    B, nf = np.array([[1.0, -1.0, 1.0], [-1.0, -1.0, 1.0], [1.0, 1.0, -1.0]]), 4
    K = B.shape[1]
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
        assert rc == code and not made and "SparseMultiGLM" in msg and all(w in msg for w in words), (rc, msg)

    mk = lambda *a, **kw: raw_desc(bz, indptr, indices, data, B, nf, *a, **kw)
    for loss in LOSSES:
        desc, keep = raw_desc(bz, indptr, indices, data, np.abs(B) if loss == "poisson" else B, nf, loss, 1.0 if loss == "huber" else None)
        assert desc.f_kind == L.BZ_F_SPARSE_MULTI_GLM == 11 and desc.f_classes == 3 and create(desc)[:2] == (0, True)
    cs = bz.SparseAffine.from_dense(np.ones((2, n)), np.zeros(2))
    desc, keep = mk(c=cs, ny=2)
    assert desc.c_kind == L.BZ_C_SPARSE_AFFINE and create(desc)[:2] == (0, True)
    w = np.array([0.5, 0.0, 2.0])
    desc, keep = mk()
    desc.f_w = w.ctypes.data
    assert create(desc)[:2] == (0, True)
    for good_k in (2, 64):                                                         # the ends of the range (n = nf * K)
        desc, keep = raw_desc(bz, indptr, indices, data, np.ones((3, good_k)), nf)
        assert create(desc)[:2] == (0, True)
    # K in 2 .. 64 (K = 1 is kind 9), n % K == 0
    for bad in (0, 1, 65):
        desc, keep = mk()
        desc.f_classes = bad
        refused(desc, L.BZ_ERR_ARG, "f_classes")
    desc, keep = mk()
    desc.f_classes = 5                                                             # 12 % 5 != 0
    refused(desc, L.BZ_ERR_ARG, "multiple")
    # the matrix checks of sp_read; the column indices lie in [0, n / K)
    desc, keep = raw_desc(bz, np.array([0, 3, 2, 5]), indices, data, B, nf)
    refused(desc, L.BZ_ERR_ARG, "row 1")
    desc, keep = raw_desc(bz, indptr, np.array([0, 3, 1, 4, 3]), data, B, nf)      # a column = n_f (< n), in row 2
    refused(desc, L.BZ_ERR_ARG, "column", "row 2")
    desc, keep = mk()
    desc.f_rows = 0
    refused(desc, L.BZ_ERR_ARG)
    desc, keep = mk()
    desc.f_b = None
    refused(desc, L.BZ_ERR_ARG)
    # the loss, delta, the scale, the weights: kind 9's checks
    for bad in (-1, 5):
        desc, keep = mk()
        desc.f_loss = bad
        refused(desc, L.BZ_ERR_ARG, "f_loss")
    for bad in (0.0, -1.0, np.inf, np.nan):
        desc, keep = mk()
        desc.f_loss_delta = bad                                                     # (Huber with delta = 0)
        refused(desc, L.BZ_ERR_ARG, "delta")
        desc, keep = mk()
        desc.f_scale = bad                                                          # (a zeroed field is an error, not a silent 1)
        refused(desc, L.BZ_ERR_ARG, "f_scale")
    desc, keep = mk("squared_hinge", None)                                          # delta is Huber's alone
    desc.f_loss_delta = np.nan
    assert create(desc)[:2] == (0, True)
    for bad, row in ((np.array([1.0, -0.5, 1.0]), "row 1"), (np.array([1.0, 1.0, np.nan]), "row 2"), (np.array([np.inf, 1.0, 1.0]), "row 0")):
        desc, keep = mk()
        desc.f_w = bad.ctypes.data
        refused(desc, L.BZ_ERR_ARG, "weights", row)
    # ... finite in the problem's type: in an fp32 problem a finite double can round to +inf
    desc, keep = mk(dtype=np.float32)
    assert create(desc)[:2] == (0, True)
    desc.f_scale = 1e300
    refused(desc, L.BZ_ERR_ARG, "f_scale")
    desc.f_scale, desc.f_loss_delta = 1.0, 1e300
    refused(desc, L.BZ_ERR_ARG, "delta")
    w32 = np.array([1.0, 1.0, 1e30], np.float32)
    desc.f_scale, desc.f_loss_delta, desc.f_w = 1e30, 1.0, w32.ctypes.data
    refused(desc, L.BZ_ERR_ARG, "weights", "row 2")
    # the four refusals
    desc, keep = mk(slack=1)
    refused(desc, L.BZ_ERR_UNSUPPORTED, "slack")
    desc, keep = mk()
    A, b2 = np.ones((2, n)), np.zeros(2)
    desc.c_kind, desc.ny, desc.c_A, desc.c_b = L.BZ_C_DENSE_AFFINE, 2, A.ctypes.data, b2.ctypes.data
    refused(desc, L.BZ_ERR_UNSUPPORTED, "DenseAffine")
    ctx2 = bz.Context(device=0, rank=0, nranks=2, comm_id=None)
    desc, keep = mk()
    refused(desc, L.BZ_ERR_UNSUPPORTED, "one rank", ctx=ctx2)
    desc, keep = mk()
    desc.g_kind = L.BZ_G_CALLBACK
    refused(desc, L.BZ_ERR_UNSUPPORTED, "callbacks")
    # f_classes set beside kind 9 changes nothing there: K is not read, whatever it holds (77 and 5 are no K of this kind, and
    # 4 % 5 != 0)
    fg = bz.SparseGLM(indptr, indices, data, B[:, 0], nf, "squared_hinge")
    for classes in (3, 5, 77, -1):
        desc, keep = lower(fg, bz.NormL1(1.0), bz.IdentityFunction(), bz.ZeroSet(), nf, nf, np.float64)
        desc.f_classes = classes
        assert desc.f_kind == 9 and create(desc)[:2] == (0, True)
    # the Python layer raises before any device call
    f = bz.SparseMultiGLM(indptr, indices, data, B, nf, "squared_hinge")
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(f, bz.NormL1(1.0), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64, slack=True)
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(f, bz.NormL1(1.0), bz.DenseAffine(A, np.zeros(2)), bz.ZeroSet(), n, 2, np.float64)


# ---- 2. the gradient bit for bit with the oracle on exact data
ZERO_LOSSES = LOSSES                                              # X = 0: every loss is exact (logistic: e = 1, l' = -b / 2 ; Poisson: l' = 1 - b)
INT_LOSSES = ("least_squares", "huber", "squared_hinge")         # integer X: no transcendental


def exact_inputs(m, nf, p, K, ny, dtype, loss, regime):
    """A_f of {-2, -1, 1, 2} under a density-p mask (structured), B integer (labels +-1, counts 0 .. 3, else [-3, 3]),
    power-of-two weights, y in [-3, 3], mu = 1/4, and X = 0 ("zero") or, "int", entries of {-1, 1} in the K responses of up to
    four features, every other entry 0 (so |t_ik| <= 8): for Huber (delta = 2) and the hinge the first of 200 draws at which
    both branches of the loss's compare occur among the m K entries (asserted)."""
    rng = np.random.default_rng(m * 7 + nf + K)
    A = structured(m, nf, p, rng, True, dtype)
    B = B_of(loss, rng, m, K, dtype)
    w = POW2[rng.integers(0, 5, m)].astype(dtype)
    y, mu = rng.integers(-3, 4, ny).astype(dtype), np.full(ny, 0.25, dtype)
    X = np.zeros((nf, K), dtype)
    if regime == "int":
        assert loss in INT_LOSSES
        for _ in range(200):
            X = np.zeros((nf, K), dtype)
            J = rng.choice(nf, min(nf, 4), replace=False)
            X[J] = rng.choice([-1.0, 1.0], (J.shape[0], K))
            t = A.astype(np.float64) @ X.astype(np.float64)
            side = np.abs(t - B) <= DELTA if loss == "huber" else (1.0 - B * t) <= 0
            if loss == "least_squares" or (side.any() and not side.all()):
                break
        assert loss == "least_squares" or (side.any() and not side.all()), "no X with both branches"
    return A, B, w, X.reshape(-1), y, mu, rng


def assert_exact(dtype, A, X, B, K, r64, pen64, g_ref, g64):
    """Exactness of the gradient whatever the order of any sum, asserted on the inputs in float64: the entries of A and X are
    integers, B is integer, the weights 2 * 2^j >= 1/2 and l' an integer or a multiple of 1/2 (the logistic loss at X = 0), so
    every r and every product a r is a multiple of 1/16 (asserted for R); the sums of magnitudes that bound every partial sum —
    of a row of A_f X with B, and of a row of A_f' R plus the penalty part — stay below 2^24 / 160 (fp32) / 2^53 / 160 (fp64): a
    tenth of the range in sixteenths.  Then the oracle in dtype has returned what its float64 run returns."""
    lim = 2.0 ** (24 if dtype == np.float32 else 53) / 160
    absA = np.abs(A.astype(np.float64))
    assert np.max(absA @ np.abs(X.astype(np.float64).reshape(-1, K)) + np.abs(B)) < lim
    assert np.max(absA.T @ np.abs(r64)) + pen64 < lim
    assert np.array_equal(r64, np.round(r64 * 16) / 16)
    assert np.array_equal(g_ref.astype(np.float64), g64)


def exact_oracle(bz, ref, dtype, shape, K, loss, regime, c_pair=None):
    """the inputs and the oracle's gradient in dtype, with the exactness conditions asserted against its float64 run (no GPU)"""
    m, nf, p = shape
    n = nf * K
    ny = n if c_pair is None else c_pair[0]
    A, B, w, x, y, mu, rng = exact_inputs(m, nf, p, K, ny, dtype, loss, regime)
    what = what_of(w, 2.0, dtype)
    if c_pair is None:
        cd, mk_c, Ac, bc = bz.IdentityFunction(), lambda dt: ref.IdentityFunction(), None, None
    else:
        Ac = structured(ny, n, c_pair[1], rng, True, dtype)
        bc = rng.integers(-3, 4, ny).astype(dtype)
        c_ptr, c_idx, c_val = csr_of(Ac, np.random.default_rng(3))
        cd, mk_c = bz.SparseAffine(c_ptr, c_idx, c_val, bc, n), lambda dt: CsrOracle(c_ptr, c_idx, c_val.astype(dt), bc.astype(dt), n)

    def make_al(dt):
        fo = MultiGLMOracle(A.astype(dt), B.astype(dt), loss, delta_of(loss), np.asarray(what).astype(dt))
        al = ref.AugLagFun(fo, mk_c(dt), sets(bz, ref, "box", dt)[1], mu.astype(dt), y.astype(dt), x.astype(dt))
        g = np.empty(n, dt)
        return al, al.gradient(g, x.astype(dt)), g, fo
    al, lx, g_ref, fo = make_al(dtype)
    al64, _, g64, fo64 = make_al(np.float64)
    pen = np.abs(al64.yupd) if Ac is None else np.abs(Ac.astype(np.float64)).T @ np.abs(al64.yupd)
    if Ac is not None:
        assert 8 * np.max(np.abs(Ac.astype(np.float64)) @ np.abs(x.astype(np.float64)) + np.abs(bc)) < 2.0 ** (24 if dtype == np.float32 else 53) / 10
    assert_exact(dtype, A, x, B, K, fo64.loss_r(x.astype(np.float64))[1], np.max(pen), g_ref, g64)
    return (A, B, w, x, y, mu, cd, n, ny), (g_ref, float(lx), float(al.fx))


def exact_run(bz, ref, dtype, shape, K, loss, regime, c_pair=None):
    (A, B, w, x, y, mu, cd, n, ny), (g_ref, lx, fx) = exact_oracle(bz, ref, dtype, shape, K, loss, regime, c_pair)
    f, indptr, indices, nnz = mg_of(bz, A, B, loss, w, 2.0)
    (g_dev, vals), pr = one_gradient(bz, (f, bz.NormL1(1.0), cd, sets(bz, ref, "box", dtype)[0]), n, ny, dtype, mu, y, x)
    assert g_dev.dtype == dtype and np.array_equal(g_dev, g_ref), (loss, regime)
    # (the values: their sums are carried in double on the device and in dtype by the oracle)
    assert abs(vals[0] - lx) <= TOL[dtype] * max(1.0, abs(lx)) and abs(vals[1] - fx) <= TOL[dtype] * max(1.0, abs(fx)), (loss, regime)
    return pr, plan_k(indptr, nnz, K), plan_k(transpose_ptr(indices, A.shape[1]), nnz, K)


EXACT = [("zero", loss) for loss in ZERO_LOSSES] + [("int", loss) for loss in INT_LOSSES]


@pytest.mark.parametrize("K", [2, 3, 5, 8])
@pytest.mark.parametrize("case", TYPED, ids=IDS)
def test_exact_gradient_bit_for_bit(bz, ref, case, K):
    """Integer A in {+-1, +-2}, integer B, power-of-two weights and scale 2, mu = 1/4, integer y, D = box; X = 0 for all five
    losses (the logistic loss has e = 1 and l' = -b / 2, Poisson l' = 1 - b) and integer X with |t| <= 8 for least squares, Huber
    (delta = 2) and the squared hinge: every product and every sum is exact (asserted on the inputs), so no summation order can
    change a bit of the gradient, which equals the oracle's BIT FOR BIT.  Two row launches, no element-wise kernel."""
    dtype, shape = case
    for regime, loss in EXACT:
        pr, (La, _, seg_a), (Lt, _, seg_t) = exact_run(bz, ref, dtype, shape, K, loss, regime)
        assert pr["gemv"]["form"] == form("k_spmm_t_algrad", K, Lt, seg_t), pr["gemv"]["form"]
        assert pr["gemv"]["launches"] == 2 and pr["al_gradient"]["launches"] == 0
        assert pr["misc"]["launches"] == int(seg_a) + int(seg_t)                  # a fold launch per cut matrix


@pytest.mark.parametrize("K", [2, 3, 5, 8])
@pytest.mark.parametrize("case", [(t, c) for t in (np.float64, np.float32) for c in PAIRS], ids=PAIR_IDS)
def test_exact_gradient_beside_a_sparse_c(bz, ref, case, K):
    """the four-launch form beside c(x) = A_c x - b_c in CSR with another row count: bit for bit the oracle's on the exact data"""
    dtype, (shape, c_pair) = case
    for regime, loss in EXACT:
        pr, _, _ = exact_run(bz, ref, dtype, shape, K, loss, regime, c_pair)
        assert pr["gemv"]["launches"] == 4 and pr["al_gradient"]["launches"] == 0
        assert pr["gemv"]["form"].startswith("k_spmv_t_finish<L="), pr["gemv"]["form"]


# ---- 3. bit for bit with K scalar problems
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("K", [3, 8])
@F64_F32
def test_the_gradient_is_that_of_K_scalar_problems_bit_for_bit(bz, ref, dtype, K, loss, monkeypatch):
    """BZ_SPMV_L=1 on both sides and an uncut matrix: with one lane per row and response the K-wide kernels and the scalar
    kernels add the same products in the same order, in the pass over A_f and in the pass over A_f', and the epilogues are one
    body.  So for every k, column k of the K-wide AL gradient equals, by array_equal, the AL gradient of
    SparseGLM(A, B[:, k], loss, weights, scale) at x = X[:, k] with the mu and y of the elements j K + k.  Real random data,
    non-uniform mu and y, D = box, a weight per row.  A wrong index into B, a weight indexed by (i, k) and swapped lane indices
    all break it.  Neither matrix is cut: no fold launch, SEG=0 in A_f''s form (the profile's last row launch) and in the plan of
    both."""
    monkeypatch.setenv("BZ_SPMV_L", "1")
    m, nf = 257, 131
    n = nf * K
    rng = np.random.default_rng(17 + K)
    A = structured(m, nf, 0.3, rng, False, dtype)
    B = B_of(loss, rng, m, K, dtype, real=True)
    w = rng.uniform(0.5, 1.5, m).astype(dtype)
    X = (0.5 * rng.standard_normal((nf, K))).astype(dtype)
    y, mu = rng.standard_normal(n).astype(dtype), (10.0 ** rng.uniform(-2, 0, n)).astype(dtype)
    indptr, indices, data = csr_of(A, np.random.default_rng(2))
    Dd = sets(bz, ref, "box", dtype)[0]
    f = bz.SparseMultiGLM(indptr, indices, data, B, nf, loss, delta=delta_of(loss), weights=w, scale=1.0 / m)
    (g_dev, vals), pr = one_gradient(bz, (f, bz.NormL1(1.0), bz.IdentityFunction(), Dd), n, n, dtype, mu, y, X.reshape(-1))
    assert pr["gemv"]["form"] == form("k_spmm_t_algrad", K, 1, False), pr["gemv"]["form"]
    assert pr["gemv"]["launches"] == 2 and pr["misc"]["launches"] == 0
    assert not plan_k(indptr, data.shape[0], K)[2] and not plan_k(transpose_ptr(indices, nf), data.shape[0], K)[2]
    G = g_dev.reshape(nf, K)
    fsum = 0.0
    for k in range(K):
        fk = bz.SparseGLM(indptr, indices, data, np.ascontiguousarray(B[:, k]), nf, loss, delta=delta_of(loss), weights=w, scale=1.0 / m)
        sel = np.arange(nf) * K + k
        (gk, vk), prk = one_gradient(bz, (fk, bz.NormL1(1.0), bz.IdentityFunction(), Dd), nf, nf, dtype, mu[sel], y[sel], np.ascontiguousarray(X[:, k]))
        assert prk["gemv"]["form"] == "k_spmv_ls_t_algrad<L=1,SEG=0>" and prk["misc"]["launches"] == 0, prk["gemv"]["form"]
        assert np.array_equal(G[:, k], gk), (k, int(np.count_nonzero(G[:, k] != gk)))
        fsum += vk[1]
    assert abs(vals[1] - fsum) <= TOL[dtype] * max(1.0, abs(fsum))


# ---- 4. general gradients on real random data
def real_inputs(A, K, loss, dtype, seed=5):
    """B by the loss, X, y, mu in [0.01, 1] and a weight per row.  The Poisson loss: X is scaled by the largest row norm of A, so
    that every t_ik has a standard deviation of one at the most and exp(t) stays far from fp32's range."""
    rng = np.random.default_rng(seed + A.shape[0] + K)
    m, nf = A.shape
    n = nf * K
    B = B_of(loss, rng, m, K, dtype, real=True)
    x = rng.standard_normal(n)
    if loss == "poisson":
        x /= max(1.0, float(np.max(np.linalg.norm(A.astype(np.float64), axis=1))))
    return (B, x.astype(dtype), rng.standard_normal(n).astype(dtype), (10.0 ** rng.uniform(-2, 0, n)).astype(dtype),
            rng.uniform(0.5, 1.5, m).astype(dtype))


GENERAL = [("least_squares", K) for K in (2, 3, 5, 8, 33, 64)] + [(loss, K) for loss in LOSSES[1:] for K in (3, 8)]


@pytest.mark.parametrize("D", ["zero", "box"])
@pytest.mark.parametrize("loss,K", GENERAL)
@pytest.mark.parametrize("name,A", SPECIAL, ids=[s[0] for s in SPECIAL])
@F64_F32
def test_general_gradient_against_the_oracle_and_between_the_forms(bz, ref, dtype, name, A, loss, K, D, monkeypatch):
    """random real data against the numpy oracle: 1e-12 / 2e-5 of the gradient's largest entry, of max(1, |value|) for the two
    values (the project's rule and numbers).  Least squares at K = 2, 8, 64 (KP = K; 64: a whole wave per row), 3 and 5 (idle
    response lanes) and 33 (a half-idle wave); all five losses at K = 3 and 8.  The multinomial test's shapes: a row with one
    entry, an empty row and an empty column, a column index twice in a row, rows longer than 4 L entries, m and n_f no multiples
    of the rows per workgroup, n_f = 1, m = 600 with a column of ones (A_f' cut), 3 x 1200 at density 0.9 (A_f cut: the fold runs
    the loss arm).  Weights with the scale 1 / m.  And the gradient under BZ_SPLS_FUSED=0 equals the default's BIT FOR BIT, with
    the launch counts (2, 0) and (2, 1)."""
    m, nf = A.shape
    n = nf * K
    indptr, indices, data, A2 = csr_with_duplicate(A.astype(dtype), np.random.default_rng(2))
    B, x, y, mu, w = real_inputs(A2, K, loss, dtype)
    Dd, Dr = sets(bz, ref, D, dtype)
    out = {}
    for kind in ("fused", "three"):
        monkeypatch.setenv("BZ_SPLS_FUSED", "0" if kind == "three" else "1")
        f = bz.SparseMultiGLM(indptr, indices, data, B, nf, loss, delta=delta_of(loss), weights=w, scale=1.0 / m)
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
    al = ref.AugLagFun(MultiGLMOracle(A2, B, loss, delta_of(loss), what_of(w, 1.0 / m, dtype)), ref.IdentityFunction(), Dr, mu.copy(), y.copy(), x)
    g_ref = np.empty(n, dtype)
    lx = float(al.gradient(g_ref, x))
    fx, tol, scale = float(al.fx), TOL[dtype], np.max(np.abs(g_ref))
    (g_dev, vals), (g3, vals3) = out["fused"], out["three"]
    print(f"max|g - g_ref| / max|g_ref| = {np.max(np.abs(g_dev.astype(np.float64) - g_ref)) / scale:.3e}, "
          f"value {abs(vals[0] - lx) / max(1.0, abs(lx)):.3e}, f {abs(vals[1] - fx) / max(1.0, abs(fx)):.3e}, "
          f"forms equal {np.array_equal(g_dev, g3)}")
    assert np.isfinite(lx) and np.isfinite(fx)
    assert np.max(np.abs(g_dev.astype(np.float64) - g_ref)) <= tol * scale
    assert abs(vals[0] - lx) <= tol * max(1.0, abs(lx))
    assert abs(vals[1] - fx) <= tol * max(1.0, abs(fx))
    assert np.array_equal(g_dev, g3)
    assert abs(vals3[0] - lx) <= tol * max(1.0, abs(lx)) and vals[1] == vals3[1]


# ---- 5. the K responses of a row are isolated
def special_value(loss, b, t, w, dtype):
    """r = w l'(b, t) at t = NaN, +inf or -inf by the header's rules"""
    if t != t:
        return np.nan
    if loss == "huber":
        return w * (DELTA if t > 0 else -DELTA)                     # v = +-inf: l' = +-delta
    if loss == "logistic":
        return w * (-b * 0.0) if b * t > 0 else w * -b              # u = +inf: sigma(-u) = 0 ; u = -inf: l' = -b
    return np.inf if t > 0 else w * (0.0 - b)                       # Poisson: e = +inf ; e = 0: l' = -b


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "+inf", "-inf"])
@pytest.mark.parametrize("loss", ["huber", "logistic", "poisson"])
@pytest.mark.parametrize("K", [3, 8])
@F64_F32
def test_a_special_value_stays_in_its_own_response(bz, ref, dtype, K, loss, bad):
    """A_f = [I | top I] with top the type's largest number (m = 8 rows, 16 features), X = [T; Z], mu = 1, y = 0, D = free,
    g = Zero: t = T + top Z, and the first m rows of the gradient ARE R (feature i occurs in row i alone, with the entry 1, and
    the penalty part is zero at a finite x).  Z = 0 gives t = T; one entry Z[i, k] = 2, -2 or NaN makes t_ik +inf, -inf or NaN
    while every x stays finite or sits in a feature whose gradient is not read.  Against the run with Z = 0 only that (i, k)
    entry of R changes and every other entry — the row's other K - 1 included — keeps its bits; the entry itself follows the
    header's rule for the loss.  At three places: the first response, an inner one and the last (K - 1, whose sum an idle
    lane holds again at K = 3).  The softmax couples a row's lanes; this kind must not."""
    m = 8
    n = 2 * m * K
    rng = np.random.default_rng(9 + K)
    B = B_of(loss, rng, m, K, dtype)
    T = rng.uniform(-2.0, 2.0, (m, K)).astype(dtype)
    top = np.finfo(dtype).max
    wide = (2 * np.arange(m + 1), np.stack([np.arange(m), m + np.arange(m)], axis=1).reshape(-1), np.resize(np.array([1.0, top], dtype), 2 * m))
    f = bz.SparseMultiGLM(*wide, B, 2 * m, loss, delta=delta_of(loss), scale=0.5)
    rest = (bz.Zero(), bz.IdentityFunction(), bz.FreeSet())
    y, mu = np.zeros(n, dtype), np.ones(n, dtype)
    X = np.concatenate((T, np.zeros((m, K), dtype)))
    (g0, v0), _ = one_gradient(bz, (f, *rest), n, n, dtype, mu, y, X.reshape(-1))
    R0 = g0.reshape(2 * m, K)[:m]
    assert np.all(np.isfinite(R0)) and np.isfinite(v0[1])
    for i, k in ((2, 0), (5, 1), (3, K - 1)):
        X1 = X.copy()
        X1[m + i, k] = bad if bad != bad else np.sign(bad) * 2.0            # (top * 2 overflows to +-inf in the row sum)
        (g1, v1), _ = one_gradient(bz, (f, *rest), n, n, dtype, mu, y, X1.reshape(-1))
        R1 = g1.reshape(2 * m, K)[:m]
        others = np.ones((m, K), bool)
        others[i, k] = False
        assert np.array_equal(R1[others], R0[others]), (i, k, np.argwhere(R1 != R0))
        want = special_value(loss, float(B[i, k]), float(bad), 0.5, dtype)
        # (by value: the gradient is r + 0, the penalty part's zero, which turns r = -0 into +0)
        assert (np.isnan(R1[i, k]) and np.isnan(v1[1])) if want != want else R1[i, k] == want, (i, k, R1[i, k], want)


# ---- 6. the epilogue element by element
def epilogue_t(m, K, loss, dtype, exact):
    """T (m x K) for A_f = I.  Real: uniform in [-30, 30] (Poisson: [-8, 8]), every fifth row near zero and — but for Poisson —
    every seventh twenty times as far out.  Exact (the two losses with an exponential): multiples of X0, where exp(-X0) is
    exactly 0 in the type — the logistic loss at u in {0, +-X0, +-2 X0} has e in {0, 1}, Poisson at t in {0, -X0, -2 X0} too."""
    rng = np.random.default_rng(31 + K)
    if exact:
        return (X0[dtype] * rng.integers(-2, 1 if loss == "poisson" else 3, (m, K))).astype(dtype)
    T = rng.uniform(-30.0, 30.0, (m, K))
    T[::5] *= 0.01
    if loss == "poisson":
        T *= 8.0 / 30.0
    else:
        T[1::7] *= 20.0
    return T.astype(dtype)


@pytest.mark.parametrize("wmode", ["none", "uniform", "vector"])
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("K", [3, 8])
@F64_F32
def test_epilogue_element_by_element(bz, ref, dtype, K, loss, wmode):
    """A_f = I (m = n_f = 300), X = T: t_ik = T[i, k].  mu = 1, y = 0, D = free, g = Zero: the penalty part of the gradient is
    zero and grad[i, k] = 1 * r_ik, so R is read off the gradient and held to w^ * l' of bz.SparseGLM.loss_and_derivative in the
    dtype by array_equal, for every loss; no weights, the uniform 0.25, a vector (one per row) with zeros in it and the scale
    1/3.  The value within the tolerance of the general test.

    Least squares, Huber and the squared hinge have no transcendental: array_equal on real random T.  The logistic and Poisson
    losses go through exp, and the device's exp and numpy's are two implementations whose last bits differ: on real random T,
    run on the MI355X, 35 to 104 of 900 / 2400 entries of R differed from numpy's in fp64 for the logistic loss (1.5 eps at the
    most) and 22 to 112 for Poisson (82 eps of r at the most, r = e - b cancelling), in fp32 89 to 647 (1.6 eps and 366 eps) —
    while the same kernels equal the scalar kind's bit for bit on such data
    (test_the_gradient_is_that_of_K_scalar_problems_bit_for_bit).  So for these two losses array_equal is asserted where the
    exponential is exact in any implementation — u (logistic) and t (Poisson) multiples of X0 with exp(-X0) = 0 in the type, 0
    among them, so that every select of the arm, both signs of b and every weight are still decided element by element — and
    the real random T is held to a bound per element.  Poisson, where r = e - b cancels: the project's rule for this loss
    (tests/test_gpu_sparse_glm.py), 1e-12 / 2e-5 of w^ max(1, e, |b|).  Logistic, r = -b w^ s with s = e / (1 + e) or 1 / (1 + e)
    and e = exp(-|u|): 8 eps of |r| — two exponentials within an ulp of the true value are 2 eps apart, and 1 + e, the quotient
    and the product with w^ round once each on either side, 5 eps in all — plus w^ times the smallest normal number, for the e
    that are subnormal (fp32 beyond |u| = 87), where an ulp is no relative bound."""
    m = 300
    rng = np.random.default_rng(3)
    B = B_of(loss, rng, m, K, dtype, real=True)
    weights, scale = {"none": (None, 1.0), "uniform": (None, 0.25),
                      "vector": (np.resize(np.array([1.0, 0.0, 0.3, 2.5, 0.0], dtype), m), 1.0 / 3.0)}[wmode]
    n = m * K
    y, mu = np.zeros(n, dtype), np.ones(n, dtype)
    ident = (np.arange(m + 1), np.arange(m), np.ones(m, dtype))
    f = bz.SparseMultiGLM(*ident, B, m, loss, delta=delta_of(loss), weights=weights, scale=scale)
    what = what_of(weights, scale, dtype)
    wcol = what if np.ndim(what) == 0 else what[:, None]
    eps = float(np.finfo(dtype).eps)
    transcendental = loss in ("logistic", "poisson")
    for exact in ((True, False) if transcendental else (True,)):
        T = epilogue_t(m, K, loss, dtype, exact and transcendental)
        (g_dev, vals), pr = one_gradient(bz, (f, bz.Zero(), bz.IdentityFunction(), bz.FreeSet()), n, n, dtype, mu, y, T.reshape(-1))
        l, dl = bz.SparseGLM.loss_and_derivative(loss, delta_of(loss), B, T)
        R_ref, terms = wcol * dl, wcol * l
        assert R_ref.dtype == dtype and g_dev.dtype == dtype and np.all(np.isfinite(R_ref)) and np.all(np.isfinite(terms))
        R_dev = g_dev.reshape(m, K)
        differ = np.argwhere(R_dev != R_ref)
        err = np.abs(R_dev.astype(np.float64) - R_ref.astype(np.float64))
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = err / np.abs(R_ref.astype(np.float64))
        print(f"{'exact' if exact else 'real'} T: {differ.shape[0]} of {m * K} entries of R differ" +
              (f": first at {tuple(differ[0])}, t = {T[tuple(differ[0])]!r}, {R_dev[tuple(differ[0])]!r} / {R_ref[tuple(differ[0])]!r}, "
               f"largest relative difference {np.nanmax(rel) / eps:.2f} eps" if differ.shape[0] else ""))
        fx = float(ref._sum(np.ascontiguousarray(terms).reshape(-1))) * (0.5 if loss == "least_squares" else 1.0)
        print(f"value {vals[1]!r} / {fx!r}")
        if exact:
            if transcendental:                                      # (every branch of the arm is taken, and e is 0 or 1)
                u = (B * T if loss == "logistic" else T).astype(np.float64)
                assert np.exp(dtype(-X0[dtype])) == 0 and (u == 0).any() and (u < 0).any() and (loss == "poisson" or (u > 0).any())
            assert np.array_equal(R_dev, R_ref)
        else:
            w64 = np.abs(np.asarray(wcol, np.float64))
            if loss == "logistic":
                assert np.all(err <= 8 * eps * np.abs(R_ref.astype(np.float64)) + w64 * float(np.finfo(dtype).tiny))
            else:
                with np.errstate(over="ignore"):
                    size = np.maximum(np.exp(T.astype(np.float64)), np.maximum(1.0, B.astype(np.float64)))
                assert np.all(err <= TOL[dtype] * w64 * size)
        assert abs(vals[1] - fx) <= TOL[dtype] * max(1.0, abs(fx)) and vals[0] == vals[1]


# ---- 7. the empty matrix, and identical runs
@pytest.mark.parametrize("loss", LOSSES)
@F64_F32
def test_empty_matrix(bz, ref, dtype, loss):
    """nnz = 0 is accepted: every t is 0, f = sum_i w^_i sum_k l(B_ik, 0) and the gradient is the penalty part alone, bit for bit
    on integer data"""
    m, nf, K = 23, 37, 3
    n = nf * K
    rng = np.random.default_rng(8)
    B = B_of(loss, rng, m, K, dtype)
    w = POW2[rng.integers(0, 5, m)].astype(dtype)
    x, y = (rng.integers(-3, 4, k).astype(dtype) for k in (n, n))
    mu = np.full(n, 0.25, dtype)
    f = bz.SparseMultiGLM(np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, dtype), B, nf, loss, delta=delta_of(loss), weights=w, scale=0.5)
    Dd, Dr = sets(bz, ref, "box", dtype)
    (g_dev, vals), _ = one_gradient(bz, (f, bz.NormL1(1.0), bz.IdentityFunction(), Dd), n, n, dtype, mu, y, x)
    fo = MultiGLMOracle(np.zeros((m, nf), dtype), B, loss, delta_of(loss), what_of(w, 0.5, dtype))
    al = ref.AugLagFun(fo, ref.IdentityFunction(), Dr, mu.copy(), y.copy(), x)
    g_ref = np.empty(n, dtype)
    lx, fx = float(al.gradient(g_ref, x)), float(al.fx)
    assert np.array_equal(g_dev, g_ref) and np.array_equal(g_dev, al.yupd)
    assert abs(vals[1] - fx) <= TOL[dtype] * max(1.0, abs(fx)) and abs(vals[0] - lx) <= TOL[dtype] * max(1.0, abs(lx))


@F64_F32
def test_launches_of_two_gradients_and_identical_runs(bz, ref, dtype):
    """two gradients: four row launches with c = Identity, eight beside a sparse c, none from k_algrad_elem; the same bits on
    both runs; the bytes of the model: the matrix once per pass, K values of B and of R per row of A_f and one weight"""
    m, nf, K = 257, 100, 5
    n = nf * K
    A = structured(m, nf, 0.05, np.random.default_rng(6), False, dtype)
    B, x, y, mu, w = real_inputs(A, K, "logistic", dtype)
    f, indptr, indices, nnz = mg_of(bz, A, B, "logistic", w, 1.0 / m)
    runs, pr = one_gradient(bz, (f, bz.NormL1(1.0), bz.IdentityFunction(), bz.ZeroSet()), n, n, dtype, mu, y, x, times=2)
    assert pr["gemv"]["launches"] == 4 and pr["al_gradient"]["launches"] == 0 and pr["misc"]["launches"] == 0
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    sz = np.dtype(dtype).itemsize
    La, nva, _ = plan_k(indptr, nnz, K)
    Lt, nvt, _ = plan_k(transpose_ptr(indices, nf), nnz, K)
    # per pass: the entries and the row pointers once, the gathered K-wide vector once; A_f: B and R (m K each) and the weights
    # (m); A_f': x, mu, mu y and the gradient (n each)
    model = 2 * nnz * (sz + 4) + (nva + 1) * 8 + (nvt + 1) * 8 + (n + m * K) * sz + (m + 2 * m * K) * sz + 4 * n * sz
    assert pr["gemv"]["bytes"] == 2 * model, (pr["gemv"], model)
    ny = 41
    rng = np.random.default_rng(12)
    Ac = structured(ny, n, 0.1, rng, False, dtype)
    c_ptr, c_idx, c_val = csr_of(Ac, np.random.default_rng(3))
    dev = (f, bz.NormL1(1.0), bz.SparseAffine(c_ptr, c_idx, c_val, rng.standard_normal(ny).astype(dtype), n), sets(bz, ref, "box", dtype)[0])
    runs, pr = one_gradient(bz, dev, n, ny, dtype, mu[:ny], y[:ny], x, times=2)
    assert pr["gemv"]["launches"] == 8 and pr["al_gradient"]["launches"] == 0
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


# ---- 8. the iterates
def mg_problem(bz, ref, shape, loss, dtype, weighted=False, beside_c=False, lam=0.5, g=None):
    """sparse_multiresponse(m, n_f, K, 5, dtype, loss): NormL1(lam) (or g = (device g, oracle g)), c = Identity, D = box(-5, 5),
    plain or with the weights 0.5 + u11 and the scale 1 / m; or beside the constraints of budget_bands(n, 10) with
    g = IndBox(0, 1)"""
    m, nf, K = shape
    n = nf * K
    d = bz.synth.sparse_multiresponse(m, nf, K, 5, dtype, loss)
    w = (0.5 + bz.synth.uniform(11, m)).astype(dtype) if weighted else None
    scale = 1.0 / m if weighted else 1.0
    f = bz.SparseMultiGLM(d["indptr"], d["indices"], d["data"], d["B"], nf, loss, delta=d["delta"], weights=w, scale=scale)
    fo = MultiGLMOracle(f.toarray(), d["B"], loss, d["delta"], what_of(w, scale, dtype))
    if not beside_c:
        gd, go = g or (bz.NormL1(lam), ref.NormL1(lam))
        dev = (f, gd, bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(-5.0, 5.0)))
        orc = (fo, go, ref.IdentityFunction(), ref.ClosedSet(ref.IndBox(dtype(-5), dtype(5))))
        return n, n, dev, orc
    bb = bz.synth.budget_bands(n, 10, dtype)
    csr = (bb["indptr"], bb["indices"], bb["data"], bb["b"], n)
    dev = (f, bz.IndBox(0.0, 1.0), bz.SparseAffine(*csr), bz.ClosedSet(bz.IndBox(bb["lo"], bb["hi"])))
    orc = (fo, ref.IndBox(dtype(0), dtype(1)), CsrOracle(*csr), ref.ClosedSet(ref.IndBox(bb["lo"], bb["hi"])))
    return n, 11, dev, orc


# (shape, loss, dtype, weighted, beside a sparse c) -> the tight states asked of the device (see the docstring below)
STATES = [((256, 16, 4), "least_squares", np.float64, False, False, 28), ((256, 12, 3), "least_squares", np.float64, False, False, 28),
          ((256, 16, 4), "least_squares", np.float32, False, False, 28), ((256, 12, 3), "least_squares", np.float32, False, False, 28),
          ((256, 16, 4), "logistic", np.float64, False, False, 28), ((256, 12, 3), "logistic", np.float64, True, False, 19),
          ((256, 12, 3), "least_squares", np.float64, False, True, 28)]
STATE_IDS = [f"{s[0][0]}x{s[0][1]}x{s[0][2]}-{s[1]}-{'f64' if s[2] is np.float64 else 'f32'}{'-weighted' if s[3] else ''}{'-sparse_c' if s[4] else ''}"
             for s in STATES]


def state_problem(bz, ref, shape, loss, dtype, weighted, beside_c):
    return mg_problem(bz, ref, shape, loss, dtype, weighted, beside_c, lam=0.5 / 256 if weighted else 0.5)


def tight_states(bz, ref, shape, loss, dtype, weighted, beside_c, iters=30):
    """the oracle alone: the states among `iters` at which its own two roundings (plain and extended-precision sums) are within
    base / 100 of each other — where the rule max(base, 100 sens) asks the device for `base`.  (The loop of
    tests.test_gpu_sparse_multinomial.oracle_tight_states, which builds the softmax's problem itself, on this kind's problem.)"""
    n, ny, dev, orc = state_problem(bz, ref, shape, loss, dtype, weighted, beside_c)
    mu, y = np.full(ny, 0.1, dtype), (0.1 * np.random.default_rng(2).standard_normal(ny)).astype(dtype)
    x0 = np.zeros(n, dtype)
    eps = float(np.finfo(dtype).eps)
    its, sts = [], []
    for red in (None, LongDoubleReducer()):
        ref.set_reducer(red)
        al = ref.AugLagFun(orc[0], orc[2], orc[3], mu.copy(), y.copy(), x0)
        its.append(ref.PANOCplusIteration(al, ref.NonsmoothCostFun(orc[1]), x0, minimum_gamma=eps))
        sts.append(its[-1].init())
    ref.set_reducer(None)
    env, tight = 0.0, 0
    for k in range(iters):
        env = max(env, _err(sts[1].x, sts[0].x), _err(sts[1].z, sts[0].z))
        assert np.isfinite(env) and np.isfinite(float(sts[0].gamma))
        tight += 100 * env <= BASE[dtype]
        if k + 1 < iters:
            sts[0] = its[0].step(sts[0])
            ref.set_reducer(LongDoubleReducer())
            sts[1] = its[1].step(sts[1])
            ref.set_reducer(None)
    return tight


@pytest.mark.parametrize("shape,loss,dtype,weighted,beside_c,tight", STATES, ids=STATE_IDS)
def test_iterates_follow_the_oracle(bz, ref, shape, loss, dtype, weighted, beside_c, tight):
    """30 states: x and z inside max(base, 100 * sens) — base 1e-9 / 5e-5, sens the oracle's own extended-precision
    envelope — and gamma equal to 1e-12 / 1e-5 relative: run_traces' rule and the numbers of
    tests/test_gpu_sparse_multinomial.py.  The number of states at which the device is asked for `base` itself: the oracle's own
    two roundings, run alone on a CPU (`python -m tests.test_gpu_sparse_multi_glm`), stay within base / 100 of each other on
    30 of 30 states in the four least-squares cases in fp64 and fp32, beside the sparse c and for the plain logistic case, and on
    21 of 30 for the weighted logistic case (scale 1 / m with lambda / m); asked for: 28 and 19, two states under each count.
    No fp32 case's oracle runs part from each other by more than the bound: the data draw is the generator's default in every
    case."""
    n, ny, dev, orc = state_problem(bz, ref, shape, loss, dtype, weighted, beside_c)
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


# ---- 9. whole solves
# (name, shape, loss, lambda): lambda chosen on the CPU oracle so that ref.alps ends first_order (`python -m
# tests.test_gpu_sparse_multi_glm` prints the status, the counts and the zero rows at each).  The planted X* has one active
# feature of 16; at these lambdas the oracle ends first_order after 6 outer iterations in every case, with 9 of the 16 rows of X
# all zero at 0.02 under NormL1 (17 inner iterations), 5 of 16 at 0.02 under NormL21 (16), and 3 of 16 at 1.0 for the logistic
# loss (280).  (From 0.05 on both least-squares problems keep the planted row alone; at 0.01 the group penalty zeroes no row.)
SOLVES = [("lasso", (256, 16, 4), "least_squares", 0.02), ("multitask", (256, 16, 4), "least_squares", 0.02),
          ("multilabel", (256, 16, 4), "logistic", 1.0)]


def solve_problem(bz, ref, name, shape, loss, lam):
    K = shape[2]
    g = (bz.NormL21(lam, K), bz.NormL21(lam, K)) if name == "multitask" else None      # (no reference class: the numpy prox is the oracle's)
    return mg_problem(bz, ref, shape, loss, np.float64, lam=lam, g=g)


@pytest.mark.parametrize("name,shape,loss,lam", SOLVES, ids=[s[0] for s in SOLVES])
def test_whole_solves(bz, ref, name, shape, loss, lam):
    """bz.alps, resident and through the host outer loop, against ref.alps on sparse_multiresponse(256, 16, 4), D = box(-5, 5):
    (a) least squares with NormL1 and (c) multi-label logistic with NormL1, (b) the multi-task Lasso, least squares with
    NormL21(lambda, group=K) against the numpy group prox — at least one feature's whole row of X is zero and at least one is
    not, on both sides.  The subsolver is the DEFAULT PANOCplus with no gamma: every loss here sees the step-size probe x0 + 1
    (the softmax kind cannot run this).  Status and outer count equal, x within 1e-4 (the bound of the GLM and multinomial
    whole-solve tests).  set_g_lambda on a live problem followed by a solve equals a fresh problem's solve bit for bit."""
    n, ny, dev, orc = solve_problem(bz, ref, name, shape, loss, lam)
    K = shape[2]
    sub = lambda **kw: bz.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
    subr = lambda **kw: ref.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
    o = ref.alps(*orc, np.zeros(n), np.zeros(ny), subsolver=subr, subsolver_maxit=100000)
    assert o[5] == "first_order"
    for resident in (True, False):
        a = bz.alps(*dev, np.zeros(n), np.zeros(ny), subsolver=sub, subsolver_maxit=100000, resident=resident)
        print(f"{name} resident={resident}: status {a[5]} outer {a[2]}/{o[2]} inner {a[3]}/{o[3]} "
              f"max|x - x_ref| {np.max(np.abs(a[0] - o[0])):.3e}")
        assert a[5] == o[5] and a[2] == o[2]
        assert np.max(np.abs(a[0] - o[0])) <= 1e-4
        if name == "multitask":
            for X in (a[0].reshape(-1, K), o[0].reshape(-1, K)):
                zero = np.all(X == 0, axis=1)
                assert zero.any() and not zero.all(), zero
            assert np.array_equal(np.all(a[0].reshape(-1, K) == 0, axis=1), np.all(o[0].reshape(-1, K) == 0, axis=1))
    # lambda set on a live problem: a solve at another lambda first, then the setter, then the solve
    mk_g = (lambda v: bz.NormL21(v, K)) if name == "multitask" else bz.NormL1
    other = 0.6 * lam
    live = bz.Problem(dev[0], mk_g(other), *dev[2:], n, ny, np.float64)
    first = bz.alps(dev[0], mk_g(other), *dev[2:], np.zeros(n), np.zeros(ny), subsolver=sub, subsolver_maxit=100000, problem=live)
    live.set_g_lambda(lam)
    again = bz.alps(*dev, np.zeros(n), np.zeros(ny), subsolver=sub, subsolver_maxit=100000, problem=live)
    live.close()
    fresh = bz.alps(*dev, np.zeros(n), np.zeros(ny), subsolver=sub, subsolver_maxit=100000, resident=True)
    assert np.array_equal(again[0], fresh[0]) and np.array_equal(again[1], fresh[1]) and again[2:4] == fresh[2:4]
    assert not np.array_equal(first[0], fresh[0])


if __name__ == "__main__":
    # the oracle alone, no GPU: the conditions of the exact inputs, the tight states of the oracle's own two roundings, and the
    # whole solves of the oracle at their lambdas
    import bazinga_jl_amd as bz_
    ref_ = ref_module()
    for K in (2, 3, 5, 8):
        for regime, loss in EXACT:
            for dtype, shape in TYPED:
                exact_oracle(bz_, ref_, dtype, shape, K, loss, regime)
            for (shape, c_pair) in PAIRS:
                for dtype in (np.float64, np.float32):
                    exact_oracle(bz_, ref_, dtype, shape, K, loss, regime, c_pair)
    print("exact inputs: all conditions hold")
    for sid, (shape, loss, dtype, weighted, beside_c, tight) in zip(STATE_IDS, STATES):
        print(f"{sid}: {tight_states(bz_, ref_, shape, loss, dtype, weighted, beside_c)} of 30 states tight in the oracle; {tight} asked")
    for name, shape, loss, lam in SOLVES:
        n, ny, dev, orc = solve_problem(bz_, ref_, name, shape, loss, lam)
        subr = lambda **kw: ref_.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
        o = ref_.alps(*orc, np.zeros(n), np.zeros(ny), subsolver=subr, subsolver_maxit=100000)
        zero = np.all(o[0].reshape(-1, shape[2]) == 0, axis=1)
        print(f"{name} lambda = {lam}: {o[5]}, outer {o[2]}, inner {o[3]}, {int(zero.sum())} of {zero.shape[0]} rows of X all zero")
