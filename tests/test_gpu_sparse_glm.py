"""f(x) = sum_i w_i l(b_i, a_i'x) with a sparse A in CSR on the device (BZ_F_SPARSE_GLM): the row kernel over A_f with one epilogue
per loss (k_spmv_glm_r<loss>: r_i = w_i l'(b_i, a_i'x) and the rows' weighted losses), then the kernels over A_f' that the sparse
least squares f has.  The plain least-squares and logistic losses against kinds 7 and 8 bit for bit; Huber, squared hinge and
Poisson exactly on integer data, element by element on a diagonal matrix, over 30 iterates and in whole solves against the oracle.

The reference package has no such losses: the oracle for f is the numpy class below (the formulas of include/bazinga_hip.h in the
problem's dtype, its sums through ref._sum / ref._dot), driven by the unmodified ref.AugLagFun, ref.PANOCplusIteration and
ref.alps, as LogisticOracle is in tests/test_gpu_sparse_logistic.py, whose shapes, helpers and tolerances are used here."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_parity import run_traces
from tests.test_gpu_sparse import CsrOracle, csr_of, plan, sets, structured, transpose_ptr
from tests.test_gpu_sparse_logistic import IDS, PAIR_IDS, PAIRS, TOL, TYPED, LogisticOracle, one_gradient, real_inputs
from tests.test_sparse_least_squares_host import CUT32

pytestmark = pytest.mark.gpu

LOSSES = ("least_squares", "logistic", "huber", "squared_hinge", "poisson")
NEW = ("huber", "squared_hinge", "poisson")


class GLMOracle:
    """f(x) = sum_i w^_i l(b_i, t_i), t = A x on a dense A, in the dtype of x; gradient A'r with r = w^ l'.  w^ is one number
    or a vector, already scaled.  The row and column sums through LogisticOracle.dots (ref._dot under a reducer) and the
    value through ref._sum."""

    def __init__(self, A, b, loss, delta=None, what=1.0):
        self.A, self.b = np.asarray(A), np.asarray(b)
        self.At = np.ascontiguousarray(self.A.T)
        self.loss, self.delta, self.what = loss, delta, what

    def terms(self, b, t):
        """l(b, t) and l'(b, t) (least_squares: v^2, halved on the sum)"""
        dt = t.dtype.type
        with np.errstate(over="ignore", invalid="ignore"):
            if self.loss == "least_squares":
                v = t - b
                return v * v, v
            if self.loss == "logistic":
                u = b * t
                e = np.exp(-np.abs(u))
                s = np.where(u >= 0, e / (dt(1) + e), dt(1) / (dt(1) + e))
                return np.where(u < 0, -u, dt(0)) + np.log1p(e), -b * s
            if self.loss == "huber":
                v, d = t - b, dt(self.delta)
                a = np.where(v < 0, -v, v)
                inside = a <= d
                return (np.where(inside, dt(0.5) * v * v, d * (a - dt(0.5) * d)),
                        np.where(inside, v, np.where(v > 0, d, np.where(v < 0, -d, v))))
            if self.loss == "squared_hinge":
                h = dt(1) - b * t
                off = h <= 0
                return np.where(off, dt(0), dt(0.5) * h * h), np.where(off, dt(0), -b * h)
            e = np.exp(t)
            bt = np.where(b == 0, dt(0), b * t)
            return np.where(e < np.inf, e - bt, e), e - b

    def loss_r(self, x):
        dt = x.dtype.type
        l, dl = self.terms(self.b.astype(x.dtype, copy=False), LogisticOracle.dots(self.A, x))
        w = dt(self.what) if np.ndim(self.what) == 0 else np.asarray(self.what, x.dtype)
        with np.errstate(over="ignore", invalid="ignore"):
            return w * l, w * dl

    def value(self, terms, dt):
        from oracle import bazinga_ref as ref
        fx = dt(ref._sum(terms))
        return dt(0.5) * fx if self.loss == "least_squares" else fx

    def __call__(self, x):
        return self.value(self.loss_r(x)[0], x.dtype.type)

    def gradient(self, y, x):
        terms, r = self.loss_r(x)
        y[...] = LogisticOracle.dots(self.At, r)
        return self.value(terms, x.dtype.type)


def what_of(weights, scale, dtype):
    """w^ = T(scale * w), the product in float64 rounded once; one number without a weight vector"""
    return dtype(scale) if weights is None else (scale * np.asarray(weights, np.float64)).astype(dtype)


def b_of(loss, rng, m, dtype):
    if loss in ("logistic", "squared_hinge"):
        return np.where(rng.random(m) < 0.5, -1.0, 1.0).astype(dtype)
    if loss == "poisson":
        return rng.integers(0, 4, m).astype(dtype)
    return rng.integers(-3, 4, m).astype(dtype)


def glm_of(bz, A, b, loss, delta=None, weights=None, scale=1.0, seed=1):
    indptr, indices, data = csr_of(A, np.random.default_rng(seed))
    return bz.SparseGLM(indptr, indices, data, b, A.shape[1], loss, delta=delta, weights=weights, scale=scale), indptr, indices, data.shape[0]


# ---- 1. creation and refusals through the raw ABI
def raw_desc(bz, indptr, indices, data, b, n, loss="huber", delta=1.0, slack=0, c=None, ny=None):
    from bazinga_jl_amd.oracles import lower
    m = b.shape[0]
    good = bz.SparseGLM(np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), b, n, loss, delta=delta)
    desc, keep = lower(good, bz.NormL1(1.0), c or bz.IdentityFunction(), bz.ZeroSet(), n, ny or n, np.float64)
    arrs = (np.ascontiguousarray(indptr, np.int64), np.ascontiguousarray(indices, np.int32), np.ascontiguousarray(data, np.float64))
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
    b, n = np.array([1.0, -1.0, 1.0]), 4

    def create(desc, ctx=ctx):
        h = C.c_void_p()
        rc = lib.bz_problem_create(ctx._h, C.byref(desc), C.byref(h))
        msg = lib.bz_last_error().decode() if rc else ""
        if h.value:
            lib.bz_problem_destroy(h)
        return rc, bool(h.value), msg

    def refused(desc, code, *words, ctx=ctx):
        rc, made, msg = create(desc, ctx)
        assert rc == code and not made and "SparseGLM" in msg and all(w in msg for w in words), (rc, msg)

    for loss in LOSSES:
        desc, keep = raw_desc(bz, indptr, indices, data, np.abs(b) if loss == "poisson" else b, n, loss, 1.0 if loss == "huber" else None)
        assert desc.f_kind == 9 and create(desc)[:2] == (0, True)
    cs = bz.SparseAffine.from_dense(np.array([[1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 2.0]]), np.zeros(2))
    desc, keep = raw_desc(bz, indptr, indices, data, b, n, c=cs, ny=2)
    assert desc.c_kind == L.BZ_C_SPARSE_AFFINE and create(desc)[:2] == (0, True)
    w = np.array([0.5, 0.0, 2.0])
    desc, keep = raw_desc(bz, indptr, indices, data, b, n)
    desc.f_w = w.ctypes.data
    assert create(desc)[:2] == (0, True)
    # the matrix checks of kind 7
    for bad_ptr, row in ((np.array([0, 3, 2, 5]), "row 1"), (np.array([1, 2, 3, 5]), "row 0")):
        desc, keep = raw_desc(bz, bad_ptr, indices, data, b, n)
        refused(desc, L.BZ_ERR_ARG, row)
    desc, keep = raw_desc(bz, np.array([0, 2, 3, 4]), indices, data, b, n)               # rowptr[m] != nnz
    refused(desc, L.BZ_ERR_ARG, "nnz", "row 2")
    desc, keep = raw_desc(bz, indptr, np.array([0, 3, 1, 4, 3]), data, b, n)             # a column = n, in row 2
    refused(desc, L.BZ_ERR_ARG, "row 2")
    desc, keep = raw_desc(bz, indptr, indices, data, b, n)
    desc.f_rows = 0
    refused(desc, L.BZ_ERR_ARG)
    desc, keep = raw_desc(bz, indptr, indices, data, b, n)
    desc.f_b = None
    refused(desc, L.BZ_ERR_ARG)
    # the loss, delta, the scale, the weights
    for bad in (-1, 5, 77):
        desc, keep = raw_desc(bz, indptr, indices, data, b, n)
        desc.f_loss = bad
        refused(desc, L.BZ_ERR_ARG, "f_loss")
    for bad in (0.0, -1.0, np.inf, np.nan):
        desc, keep = raw_desc(bz, indptr, indices, data, b, n)
        desc.f_loss_delta = bad
        refused(desc, L.BZ_ERR_ARG, "delta")
        desc, keep = raw_desc(bz, indptr, indices, data, b, n)
        desc.f_scale = bad                                                              # (a zeroed field is an error, not a silent 1)
        refused(desc, L.BZ_ERR_ARG, "f_scale")
    desc, keep = raw_desc(bz, indptr, indices, data, b, n, "squared_hinge", None)        # delta is Huber's alone
    desc.f_loss_delta = np.nan
    assert create(desc)[:2] == (0, True)
    for bad, row in ((np.array([1.0, -0.5, 1.0]), "row 1"), (np.array([1.0, 1.0, np.nan]), "row 2"), (np.array([np.inf, 1.0, 1.0]), "row 0")):
        desc, keep = raw_desc(bz, indptr, indices, data, b, n)
        desc.f_w = bad.ctypes.data
        refused(desc, L.BZ_ERR_ARG, "weights", row)
    # the numbers the kernel multiplies by are the rounded ones: in an fp32 problem a finite double can round to +inf
    f32 = bz.SparseGLM(indptr, indices, data.astype(np.float32), b.astype(np.float32), n, "huber", delta=1.0, weights=np.ones(3, np.float32))
    desc, keep32 = lower(f32, bz.NormL1(1.0), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float32)
    assert create(desc)[:2] == (0, True)
    desc.f_scale = 1e300
    refused(desc, L.BZ_ERR_ARG, "f_scale")
    desc.f_scale, desc.f_loss_delta = 1.0, 1e300
    refused(desc, L.BZ_ERR_ARG, "delta")
    w32 = np.array([1.0, 1.0, 1e30], np.float32)
    desc.f_scale, desc.f_loss_delta, desc.f_w = 1e30, 1.0, w32.ctypes.data
    refused(desc, L.BZ_ERR_ARG, "weights", "row 2")
    # the four refusals
    desc, keep = raw_desc(bz, indptr, indices, data, b, n, slack=1)
    refused(desc, L.BZ_ERR_UNSUPPORTED, "slack")
    desc, keep = raw_desc(bz, indptr, indices, data, b, n)
    A, b2 = np.ones((2, n)), np.zeros(2)
    desc.c_kind, desc.ny, desc.c_A, desc.c_b = L.BZ_C_DENSE_AFFINE, 2, A.ctypes.data, b2.ctypes.data
    refused(desc, L.BZ_ERR_UNSUPPORTED, "DenseAffine")
    ctx2 = bz.Context(device=0, rank=0, nranks=2, comm_id=None)
    desc, keep = raw_desc(bz, indptr, indices, data, b, n)
    refused(desc, L.BZ_ERR_UNSUPPORTED, "one rank", ctx=ctx2)
    desc, keep = raw_desc(bz, indptr, indices, data, b, n)
    desc.g_kind = L.BZ_G_CALLBACK
    refused(desc, L.BZ_ERR_UNSUPPORTED, "callbacks")
    # kinds 7 and 8 ignore the new fields
    junk = np.array([np.nan])
    for f in (bz.SparseLeastSquares(indptr, indices, data, b, n), bz.SparseLogistic(indptr, indices, data, b, n)):
        desc, keep = lower(f, bz.NormL1(1.0), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64)
        desc.f_loss, desc.f_loss_delta, desc.f_w, desc.f_scale = 77, np.nan, junk.ctypes.data, -1.0
        assert desc.f_kind in (7, 8) and create(desc)[:2] == (0, True)
    # the Python layer raises before any device call
    f = bz.SparseGLM(indptr, indices, data, b, n, "squared_hinge")
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(f, bz.NormL1(1.0), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64, slack=True)
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(f, bz.NormL1(1.0), bz.DenseAffine(A, np.zeros(2)), bz.ZeroSet(), n, 2, np.float64)


# ---- 2. the least-squares and logistic losses: the bits of kinds 7 and 8
def old_and_new(bz, loss, A, b, seed=2):
    """kind 7 / 8 and the three spellings of the same f as a SparseGLM: no weights, a weight vector of ones, scale = 1 given"""
    indptr, indices, data = csr_of(A, np.random.default_rng(seed))
    n, m = A.shape[1], A.shape[0]
    old = (bz.SparseLeastSquares if loss == "least_squares" else bz.SparseLogistic)(indptr, indices, data, b, n)
    new = [bz.SparseGLM(indptr, indices, data, b, n, loss), bz.SparseGLM(indptr, indices, data, b, n, loss, weights=np.ones(m, A.dtype)),
           bz.SparseGLM(indptr, indices, data, b, n, loss, scale=1.0)]
    return old, new


SAME = [TYPED[4], TYPED[9], TYPED[len(TYPED) - 9], (np.float32, CUT32[0])]


@pytest.mark.parametrize("loss", ["least_squares", "logistic"])
@pytest.mark.parametrize("case", SAME, ids=IDS)
def test_plain_losses_give_the_bits_of_kinds_7_and_8(bz, ref, case, loss):
    """one AL gradient and both values: array_equal / == against the existing kind, for the GLM without weights (which runs the
    existing kernel) and with a weight vector of ones (which runs k_spmv_glm_r: a multiplication by 1 is exact)"""
    dtype, (m, n, p) = case
    A, _, x, y, mu, rng = real_inputs(m, n, p, n, dtype)
    b = b_of(loss, rng, m, dtype) if loss == "logistic" else rng.standard_normal(m).astype(dtype)
    old, new = old_and_new(bz, loss, A, b)
    rest = (bz.NormL1(1.0), bz.IdentityFunction(), sets(bz, ref, "box", dtype)[0])
    (g0, v0), pr0 = one_gradient(bz, (old, *rest), n, n, dtype, mu, y, x)
    for f in new:
        (g1, v1), pr1 = one_gradient(bz, (f, *rest), n, n, dtype, mu, y, x)
        assert np.array_equal(g0, g1) and v0 == v1
        assert pr1["gemv"]["launches"] == 2 and pr1["gemv"]["bytes"] == pr0["gemv"]["bytes"] + (m * np.dtype(dtype).itemsize if f.weights is not None else 0)


@pytest.mark.parametrize("loss", ["least_squares", "logistic"])
def test_plain_losses_give_the_iterates_of_kinds_7_and_8(bz, ref, loss):
    """30 PANOC states on sparse_logistic(256, 64, 5) (least squares: with sparse_lasso's b): x, z and the scalars equal"""
    m, n = 256, 64
    d = bz.synth.sparse_logistic(m, n, 5)
    b = d["labels"] if loss == "logistic" else bz.synth.sparse_lasso(m, n, 5)["b"]
    args = (d["indptr"], d["indices"], d["data"], b, n)
    old = (bz.SparseLeastSquares if loss == "least_squares" else bz.SparseLogistic)(*args)
    fs = [old, bz.SparseGLM(*args, loss), bz.SparseGLM(*args, loss, weights=np.ones(m)), bz.SparseGLM(*args, loss, scale=1.0)]
    mu, y = np.full(n, 0.1), 0.1 * np.random.default_rng(2).standard_normal(n)
    opts = bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=float(np.finfo(np.float64).eps)).c_opts()
    probs = [bz.Problem(f, bz.NormL1(0.5), bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(-5.0, 5.0)), n, n, np.float64) for f in fs]
    for p in probs:
        p.set_multipliers(mu, y)
        p.panoc_begin(opts, np.zeros(n))
    for k in range(30):
        x0, z0, s0 = probs[0].panoc_vector("x"), probs[0].panoc_vector("z"), probs[0].panoc_scalars()
        for p in probs[1:]:
            s1 = p.panoc_scalars()
            assert np.array_equal(x0, p.panoc_vector("x")) and np.array_equal(z0, p.panoc_vector("z")), k
            assert all(s0[key] == s1[key] or (s0[key] != s0[key] and s1[key] != s1[key]) for key in s0), (k, s0, s1)
        for p in probs:
            p.panoc_step()
    for p in probs:
        p.close()


# ---- 3. the exact gradient on integer data
DELTA = 2.0
POW2 = np.array([0.25, 0.5, 1.0, 2.0, 4.0])


def branches(loss, b, t):
    """which side of the loss's compare every row takes"""
    return np.abs(t - b) <= DELTA if loss == "huber" else (1.0 - b * t) <= 0


def integer_inputs(m, n, p, ny, dtype, loss, regime):
    """A_f of {-2, -1, 1, 2} under a density-p mask (structured), b integer (labels +-1, counts 0 .. 3), power-of-two weights, y
    in [-3, 3], mu = 1/4, and x = 0 ("zero") or, "far", integers of [-4, 4] at eight places: the first draw at which both
    branches of the loss's compare occur among the rows (asserted)"""
    rng = np.random.default_rng(m * 7 + n)
    A = structured(m, n, p, rng, True, dtype)
    b = b_of(loss, rng, m, dtype)
    w = POW2[rng.integers(0, 5, m)].astype(dtype)
    y, mu = rng.integers(-3, 4, ny).astype(dtype), np.full(ny, 0.25, dtype)
    x = np.zeros(n, dtype)
    if regime == "far":
        assert loss != "poisson"
        for _ in range(200):
            x = np.zeros(n, dtype)
            x[rng.choice(n, min(n, 8), replace=False)] = rng.integers(1, 5, min(n, 8)) * rng.choice([-1, 1], min(n, 8))
            side = branches(loss, b.astype(np.float64), A.astype(np.float64) @ x.astype(np.float64))
            if side.any() and not side.all():
                break
        assert side.any() and not side.all(), "no x with both branches"
    return A, b, w, x, y, mu, rng


def assert_exact(dtype, A, x, b, r64, pen64, g_ref, g64):
    """Exactness of the gradient whatever the order of any sum: every input is an integer or a power of two >= 1/4, so every
    product is a multiple of 1/8; the sums of magnitudes that bound every partial sum — of a row of A_f x with b, and of a row
    of A_f' r plus the penalty part — stay below 2^24 / 80 (fp32) / 2^53 / 80 (fp64): a tenth of the range in eighths.  Then
    the oracle in dtype has returned what its float64 run returns."""
    lim = 2.0 ** (24 if dtype == np.float32 else 53) / 80
    absA = np.abs(A.astype(np.float64))
    assert np.max(absA @ np.abs(x.astype(np.float64)) + np.abs(b)) < lim
    assert np.max(absA.T @ np.abs(r64) + pen64) < lim
    assert np.array_equal(g_ref.astype(np.float64), g64)


def exact_run(bz, ref, dtype, shape, loss, D_name, regime, c_pair=None, with_w=True):
    m, n, p = shape
    ny = n if c_pair is None else c_pair[0]
    A, b, w, x, y, mu, rng = integer_inputs(m, n, p, ny, dtype, loss, regime)
    delta = DELTA if loss == "huber" else None
    f, indptr, indices, nnz = glm_of(bz, A, b, loss, delta, w if with_w else None, 2.0)
    what = what_of(w if with_w else None, 2.0, dtype)
    if c_pair is None:
        cd, mk_c = bz.IdentityFunction(), lambda dt: ref.IdentityFunction()
        Ac = None
    else:
        Ac = structured(ny, n, c_pair[1], rng, True, dtype)
        bc = rng.integers(-3, 4, ny).astype(dtype)
        c_ptr, c_idx, c_val = csr_of(Ac, np.random.default_rng(3))
        cd, mk_c = bz.SparseAffine(c_ptr, c_idx, c_val, bc, n), lambda dt: CsrOracle(c_ptr, c_idx, c_val.astype(dt), bc.astype(dt), n)
    (g_dev, vals), pr = one_gradient(bz, (f, bz.NormL1(1.0), cd, sets(bz, ref, D_name, dtype)[0]), n, ny, dtype, mu, y, x)

    def make_al(dt):
        fo = GLMOracle(A.astype(dt), b.astype(dt), loss, delta, np.asarray(what).astype(dt))
        al = ref.AugLagFun(fo, mk_c(dt), sets(bz, ref, D_name, dt)[1], mu.astype(dt), y.astype(dt), x.astype(dt))
        g = np.empty(n, dt)
        return al, al.gradient(g, x.astype(dt)), g, fo
    al, lx, g_ref, fo = make_al(dtype)
    al64, _, g64, fo64 = make_al(np.float64)
    pen = np.abs(al64.yupd) if Ac is None else np.abs(Ac.astype(np.float64)).T @ np.abs(al64.yupd)
    if Ac is not None:
        assert 8 * np.max(np.abs(Ac.astype(np.float64)) @ np.abs(x.astype(np.float64)) + np.abs(bc)) < 2.0 ** (24 if dtype == np.float32 else 53) / 10
    assert_exact(dtype, A, x, b, fo64.loss_r(x.astype(np.float64))[1], np.max(pen), g_ref, g64)
    assert g_dev.dtype == dtype and np.array_equal(g_dev, g_ref)
    # (the values: their sums are carried in double on the device and in dtype by the oracle)
    lx, fx = float(lx), float(al.fx)
    assert abs(vals[0] - lx) <= TOL[dtype] * max(1.0, abs(lx)) and abs(vals[1] - fx) <= TOL[dtype] * max(1.0, abs(fx))
    return g_dev, vals, pr, plan(indptr, nnz), plan(transpose_ptr(indices, n), nnz)


EXACT = [(loss, regime) for loss in NEW for regime in ("zero", "far") if (loss, regime) != ("poisson", "far")]


@pytest.mark.parametrize("loss,regime", EXACT)
@pytest.mark.parametrize("case", TYPED, ids=IDS)
def test_exact_gradient_bit_for_bit(bz, ref, case, loss, regime):
    """Integer A, x, b and delta, power-of-two weights and scale 2, mu = 1/4, integer y, D = box: every product and every sum is
    exact, so no summation order can change a bit of the gradient, which equals the oracle's BIT FOR BIT.  Huber and the hinge at
    x = 0 and at an x where both of their branches occur; Poisson at x = 0, where e = exp(0) = 1 exactly.  Two row launches, no
    element-wise kernel."""
    dtype, shape = case
    _, _, pr, (La, _, seg_a), (Lt, _, seg_t) = exact_run(bz, ref, dtype, shape, loss, "box", regime)
    assert pr["gemv"]["form"] == f"k_spmv_ls_t_algrad<L={Lt},SEG={int(seg_t)}>", pr["gemv"]["form"]
    assert pr["gemv"]["launches"] == 2 and pr["al_gradient"]["launches"] == 0
    assert pr["misc"]["launches"] == int(seg_a) + int(seg_t)                  # a fold launch per cut matrix


@pytest.mark.parametrize("D", ["zero", "free"])
@pytest.mark.parametrize("case", TYPED, ids=IDS)
def test_exact_gradient_of_the_huber_loss_under_the_other_sets(bz, ref, case, D):
    dtype, shape = case
    exact_run(bz, ref, dtype, shape, "huber", D, "far")


@pytest.mark.parametrize("loss", NEW)
@pytest.mark.parametrize("case", [(np.float64, (257, 1031, 0.9)), (np.float64, (1031, 257, 0.9)), (np.float32, (41, 121, 0.25))], ids=IDS)
def test_exact_gradient_in_the_three_launch_form(bz, ref, case, loss, monkeypatch):
    """BZ_SPLS_FUSED=0 on the exact data: the plain product over A_f' and k_algrad_elem in its mode 1, against the same oracle
    and against the default form with array_equal"""
    dtype, shape = case
    regime = "zero" if loss == "poisson" else "far"
    g2, vals2, _, _, _ = exact_run(bz, ref, dtype, shape, loss, "box", regime)
    monkeypatch.setenv("BZ_SPLS_FUSED", "0")
    g3, vals3, pr, _, (Lt, _, seg_t) = exact_run(bz, ref, dtype, shape, loss, "box", regime)
    assert pr["gemv"]["form"] == f"k_spmv_ls_t<L={Lt},SEG={int(seg_t)}>", pr["gemv"]["form"]
    assert pr["gemv"]["launches"] == 2 and pr["al_gradient"]["launches"] == 1
    assert np.array_equal(g2, g3) and vals2[1] == vals3[1]


@pytest.mark.parametrize("loss", NEW)
@pytest.mark.parametrize("case", [(t, c) for t in (np.float64, np.float32) for c in PAIRS], ids=PAIR_IDS)
def test_exact_gradient_beside_a_sparse_c(bz, ref, case, loss):
    """the four-launch form beside c(x) = A_c x - b_c in CSR with another row count: bit for bit the oracle's"""
    dtype, (shape, c_pair) = case
    _, _, pr, _, _ = exact_run(bz, ref, dtype, shape, loss, "box", "zero" if loss == "poisson" else "far", c_pair)
    assert pr["gemv"]["launches"] == 4 and pr["al_gradient"]["launches"] == 0
    assert pr["gemv"]["form"].startswith("k_spmv_t_finish<L="), pr["gemv"]["form"]


# ---- 4. the epilogue element by element
def diagonal_inputs(loss, dtype, wmode):
    n = 1024
    big = 1e300 if dtype == np.float64 else 1e30
    special = [700.0, -700.0, 1e3, -1e3, big, -big, np.nan, np.nan, float(np.finfo(dtype).tiny)]
    t = np.concatenate((np.linspace(-90.0, 90.0, 1000), special, np.resize([1.0, -1.0], n - 1000 - len(special)))).astype(dtype)
    b = {"huber": np.resize(np.array([0.5, -1.0, 3.0], dtype), n), "squared_hinge": np.resize(np.array([1.0, 1.0, -1.0], dtype), n),
         "poisson": np.resize(np.array([0.0, 1.0, 3.0], dtype), n)}[loss]
    weights, scale = {"none": (None, 1.0), "uniform": (None, 0.25), "vector": (np.resize(np.array([1.0, 0.0, 0.3, 2.5, 0.0], dtype), n), 1.0 / 3.0)}[wmode]
    return n, t, b, weights, scale


@pytest.mark.parametrize("wmode", ["none", "uniform", "vector"])
@pytest.mark.parametrize("loss", NEW)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_epilogue_element_by_element(bz, ref, dtype, loss, wmode):
    """A_f diagonal, n = 1024, x = ones: row i has t_i = its entry.  t: 1000 points of linspace(-90, 90), +-700, +-1e3, +-1e30 /
    +-1e300, two NaN, the smallest normal number (and +-1 up to n); no weights, the uniform 0.25, a vector with zeros in it and the
    scale 1/3.  mu = 1, y = 0, D = free: the penalty part of the gradient is zero and grad_i = t_i r_i, one product in the type.
    Huber (delta = 1.5) and the squared hinge have no transcendental: the gradient equals t * r of the numpy oracle in the dtype
    BIT FOR BIT.  Poisson: r = e - b cancels, so r_i = grad_i / t_i is held to 1e-12 / 2e-5 of max(e, b) per element.  NaN and the
    infinities of the gradient in the oracle's places, and in both values; the values of the finite rows alone within the
    tolerance."""
    n, t, b, weights, scale = diagonal_inputs(loss, dtype, wmode)
    delta = 1.5 if loss == "huber" else None
    x, y, mu = np.ones(n, dtype), np.zeros(n, dtype), np.ones(n, dtype)
    rest = (bz.Zero(), bz.IdentityFunction(), bz.FreeSet())
    f = bz.SparseGLM(np.arange(n + 1), np.arange(n), t, b, n, loss, delta=delta, weights=weights, scale=scale)
    (g_dev, vals), pr = one_gradient(bz, (f, *rest), n, n, dtype, mu, y, x)
    fo = GLMOracle(np.diag(t), b, loss, delta, what_of(weights, scale, dtype))
    terms_ref, r_ref = fo.loss_r(x)
    with np.errstate(over="ignore", invalid="ignore"):
        g_ref = t * r_ref
    assert g_dev.dtype == dtype
    assert np.array_equal(np.isnan(g_dev), np.isnan(g_ref)) and np.count_nonzero(np.isnan(g_ref)) >= 2
    assert np.array_equal(np.isinf(g_dev), np.isinf(g_ref)) and np.array_equal(np.sign(g_dev[np.isinf(g_ref)]), np.sign(g_ref[np.isinf(g_ref)]))
    assert np.isnan(vals[0]) and np.isnan(vals[1])                           # the NaN rows reach the value too
    ok = np.isfinite(g_ref)
    if loss == "poisson":
        with np.errstate(invalid="ignore", over="ignore"):
            r_dev = g_dev / t
            scale_el = np.maximum(np.exp(t.astype(np.float64)), b.astype(np.float64)) * np.abs(np.asarray(fo.what, np.float64))
        err = np.abs(r_dev[ok].astype(np.float64) - r_ref[ok].astype(np.float64))
        bound = TOL[dtype] * scale_el[ok]
        worst = int(np.argmax(err - bound))
        print(f"worst element: t = {t[ok][worst]!r}, r_dev = {r_dev[ok][worst]!r}, r_ref = {r_ref[ok][worst]!r}, "
              f"max err / max(e, b) = {np.max(err[bound > 0] / scale_el[ok][bound > 0]):.3e}")
        assert np.all(err <= bound)
    else:
        differ = np.flatnonzero(ok & (g_dev != g_ref))
        print(f"{differ.shape[0]} elements differ" + (f": first t = {t[differ[0]]!r}, {g_dev[differ[0]]!r} / {g_ref[differ[0]]!r}" if differ.shape[0] else ""))
        assert np.array_equal(g_dev[ok], g_ref[ok])
    # the values on the rows whose loss is finite: the other entries of the diagonal set to zero (t = 0)
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(terms_ref) & np.isfinite(t) & (np.abs(t) < (64 if loss == "poisson" else 1e3))      # (their fp32 sum stays finite)
    t2 = np.where(fin, t, dtype(0))
    f2 = bz.SparseGLM(np.arange(n + 1), np.arange(n), t2, b, n, loss, delta=delta, weights=weights, scale=scale)
    (_, vals2), _ = one_gradient(bz, (f2, *rest), n, n, dtype, mu, y, x)
    fx = float(GLMOracle(np.diag(t2), b, loss, delta, fo.what)(x))
    print(f"value {vals2[1]!r} / {fx!r}")
    assert np.isfinite(fx) and abs(vals2[1] - fx) <= TOL[dtype] * max(1.0, abs(fx)) and vals2[0] == vals2[1]


def test_epilogue_edge_values(bz, ref):
    """through a diagonal A_f whose entries are +-DBL_MAX with x = 2 (the row sum overflows to +-inf): Huber at v = +-inf gives
    +inf and +-delta ; the hinge at u = +inf gives 0 and 0, at u = -inf +inf and -b inf ; Poisson at t = -inf gives 0 with b = 0
    and +inf with b > 0, at t = +inf +inf and +inf.  And fp32 Poisson at t = 100, where exp overflows: +inf, not NaN."""
    dtype = np.float64
    n = 4
    top = float(np.finfo(dtype).max)
    x, y, mu = np.full(n, 2.0), np.zeros(n), np.ones(n)
    rest = (bz.Zero(), bz.IdentityFunction(), bz.FreeSet())
    ptr, idx = np.array([0, 1, 2, 2, 2]), np.array([0, 1])

    def run(loss, data, b, delta=None, dt=np.float64, xs=2.0):
        f = bz.SparseGLM(ptr, idx, np.array(data, dt), np.array(b, dt), n, loss, delta=delta)
        return one_gradient(bz, (f, *rest), n, n, dt, mu.astype(dt), y.astype(dt), np.full(n, xs, dt))[0]
    # Huber, delta = 3: rows 0 / 1 at v = +inf / -inf: r = +-3, grad = a r = +-top * +-3 = +inf in both; the value +inf
    g, vals = run("huber", [top, -top], [1.0, 1.0, 0.0, 0.0], 3.0)
    assert vals[1] == np.inf and g[0] == np.inf and g[1] == np.inf and not np.any(g[2:])
    # the hinge: u = +inf in rows 0 and 1 (b = 1, t = +inf ; b = -1, t = -inf): 0 and 0 ; rows 2 and 3 are empty: h = 1, loss 1/2
    g, vals = run("squared_hinge", [top, -top], [1.0, -1.0, 1.0, -1.0])
    assert vals[1] == 1.0 and not np.any(g)
    # u = -inf in rows 0 and 1: loss +inf, r = -b inf, grad = a r = +inf
    g, vals = run("squared_hinge", [-top, top], [1.0, -1.0, 1.0, -1.0])
    assert vals[1] == np.inf and g[0] == np.inf and g[1] == np.inf and not np.any(g[2:])
    # Poisson at t = -inf: b = 0 gives loss 0 and r = 0 ; the empty rows give e = 1 ; b = 2 gives +inf
    g, vals = run("poisson", [-top, 0.0], [0.0, 0.0, 0.0, 0.0])
    assert vals[1] == 3.0 and g[0] == 0.0                                    # (grad_0 = -top * 0)
    g, vals = run("poisson", [-top, 0.0], [2.0, 0.0, 0.0, 0.0])
    assert vals[1] == np.inf and g[0] == np.inf                              # (r_0 = 0 - 2, grad_0 = -top * -2)
    g, vals = run("poisson", [top, 0.0], [2.0, 0.0, 0.0, 0.0])
    assert vals[1] == np.inf and g[0] == np.inf
    # fp32, t = 100: exp overflows; the loss is +inf (never inf - inf) and r = +inf
    g, vals = run("poisson", [100.0, 0.0], [3.0, 0.0, 0.0, 0.0], dt=np.float32, xs=1.0)
    assert vals[1] == np.inf and vals[0] == np.inf and g[0] == np.inf and not np.isnan(g).any()
    # Huber at v = +-delta exactly is inside, the hinge at u = 1 is off
    g, vals = run("huber", [1.0, -2.0], [-1.0, -1.0, 0.0, 0.0], 3.0)         # t = 2, -4 ; v = 3, -3
    assert np.array_equal(g[:2], [3.0, 6.0]) and vals[1] == 9.0
    g, vals = run("squared_hinge", [0.5, -0.5], [1.0, -1.0, 1.0, 1.0])       # u = 1 in rows 0 and 1
    assert not np.any(g) and vals[1] == 1.0


# ---- 5. the empty matrix
@pytest.mark.parametrize("loss", NEW)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_empty_matrix(bz, ref, dtype, loss):
    """nnz = 0 is accepted: every t is 0, f = sum_i w^_i l(b_i, 0) and the gradient is the penalty part alone, bit for bit on
    integer data"""
    m, n = 23, 37
    rng = np.random.default_rng(8)
    b = b_of(loss, rng, m, dtype)
    w = POW2[rng.integers(0, 5, m)].astype(dtype)
    x, y = (rng.integers(-3, 4, k).astype(dtype) for k in (n, n))
    mu = np.full(n, 0.25, dtype)
    delta = DELTA if loss == "huber" else None
    f = bz.SparseGLM(np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, dtype), b, n, loss, delta=delta, weights=w, scale=0.5)
    Dd, Dr = sets(bz, ref, "box", dtype)
    (g_dev, vals), _ = one_gradient(bz, (f, bz.NormL1(1.0), bz.IdentityFunction(), Dd), n, n, dtype, mu, y, x)
    fo = GLMOracle(np.zeros((m, n), dtype), b, loss, delta, what_of(w, 0.5, dtype))
    al = ref.AugLagFun(fo, ref.IdentityFunction(), Dr, mu.copy(), y.copy(), x)
    g_ref = np.empty(n, dtype)
    lx = float(al.gradient(g_ref, x))
    at0 = {"huber": np.where(np.abs(b) <= DELTA, 0.5 * b * b, DELTA * (np.abs(b) - 0.5 * DELTA)), "squared_hinge": np.full(m, 0.5),
           "poisson": np.ones(m)}[loss]
    assert np.array_equal(g_dev, g_ref) and np.array_equal(g_dev, al.yupd)
    assert vals[1] == float(np.dot(0.5 * w.astype(np.float64), at0))          # (multiples of 1/16: exact)
    assert abs(vals[0] - lx) <= TOL[dtype] * max(1.0, abs(lx))


# ---- 6. launches and bytes
@pytest.mark.parametrize("vector", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_launches_of_two_gradients_and_identical_runs(bz, ref, dtype, vector):
    """two gradients: four row launches with c = Identity, eight beside a sparse c, none from k_algrad_elem; the same bits on
    both runs; the bytes of the logistic kind's model plus, per pass over A_f, m elements when the weights are a vector"""
    m, n = 257, 500
    A, _, x, y, mu, rng = real_inputs(m, n, 0.03, n, dtype)
    b = rng.standard_normal(m).astype(dtype)
    w = rng.uniform(0.5, 1.5, m).astype(dtype) if vector else None
    f, indptr, indices, nnz = glm_of(bz, A, b, "huber", 1.0, w, 1.0 / m)
    runs, pr = one_gradient(bz, (f, bz.NormL1(1.0), bz.IdentityFunction(), bz.ZeroSet()), n, n, dtype, mu, y, x, times=2)
    assert pr["gemv"]["launches"] == 4 and pr["al_gradient"]["launches"] == 0 and pr["misc"]["launches"] == 0
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    sz = np.dtype(dtype).itemsize
    La, nva, _ = plan(indptr, nnz)
    Lt, nvt, _ = plan(transpose_ptr(indices, n), nnz)
    model = 2 * nnz * (sz + 4) + (nva + 1) * 8 + (nvt + 1) * 8 + (n + m) * sz + 2 * m * sz + 4 * n * sz + (m * sz if vector else 0)
    assert pr["gemv"]["bytes"] == 2 * model, (pr["gemv"], model)
    # beside a sparse c
    ny = 41
    Ac = structured(ny, n, 0.1, rng, False, dtype)
    c_ptr, c_idx, c_val = csr_of(Ac, np.random.default_rng(3))
    dev = (f, bz.NormL1(1.0), bz.SparseAffine(c_ptr, c_idx, c_val, rng.standard_normal(ny).astype(dtype), n), sets(bz, ref, "box", dtype)[0])
    runs, pr = one_gradient(bz, dev, n, ny, dtype, mu[:ny], y[:ny], x, times=2)
    assert pr["gemv"]["launches"] == 8 and pr["al_gradient"]["launches"] == 0
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


# ---- 7. the iterates, 8. whole solves
def glm_problem(bz, ref, loss, dtype, weighted=False, beside_c=False, lam=0.5):
    """sparse_glm(256, 64, 5, loss): NormL1(lam), c = Identity, D = box(-5, 5), plain or with the weights 0.5 + u11 and the
    scale 1 / m ; or beside the constraints of budget_bands(64, 10) with g = IndBox(0, 1)"""
    m, n = 256, 64
    d = bz.synth.sparse_glm(m, n, 5, loss, dtype)
    w = (0.5 + bz.synth.uniform(11, m)).astype(dtype) if weighted else None
    scale = 1.0 / m if weighted else 1.0
    f = bz.SparseGLM(d["indptr"], d["indices"], d["data"], d["b"], n, loss, delta=d["delta"], weights=w, scale=scale)
    fo = GLMOracle(f.toarray(), d["b"], loss, d["delta"], what_of(w, scale, dtype))
    if not beside_c:
        dev = (f, bz.NormL1(lam), bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(-5.0, 5.0)))
        orc = (fo, ref.NormL1(lam), ref.IdentityFunction(), ref.ClosedSet(ref.IndBox(dtype(-5), dtype(5))))
        return n, n, dev, orc
    bb = bz.synth.budget_bands(n, 10, dtype)
    csr = (bb["indptr"], bb["indices"], bb["data"], bb["b"], n)
    dev = (f, bz.IndBox(0.0, 1.0), bz.SparseAffine(*csr), bz.ClosedSet(bz.IndBox(bb["lo"], bb["hi"])))
    orc = (fo, ref.IndBox(dtype(0), dtype(1)), CsrOracle(*csr), ref.ClosedSet(ref.IndBox(bb["lo"], bb["hi"])))
    return n, 11, dev, orc


STATES = [("huber", np.float64, False, False), ("squared_hinge", np.float64, False, False), ("poisson", np.float64, False, False),
          ("poisson", np.float32, True, False), ("huber", np.float64, False, True)]


@pytest.mark.parametrize("loss,dtype,weighted,beside_c", STATES,
                         ids=lambda v: v if isinstance(v, str) else ("f64" if v is np.float64 else "f32" if v is np.float32 else str(int(v))))
def test_iterates_follow_the_oracle(bz, ref, loss, dtype, weighted, beside_c):
    """30 states: x and z inside max(base, 100 * sens) — base 1e-9 / 5e-5, sens the oracle's own extended-precision
    envelope — and gamma equal to 1e-12 / 1e-5 relative: the rule and the numbers of tests/test_gpu_sparse_logistic.py.
    The gamma halvings and tau backtracks that occurred are printed."""
    n, ny, dev, orc = glm_problem(bz, ref, loss, dtype, weighted, beside_c, lam=0.5 / 256 if weighted else 0.5)
    mu, y = np.full(ny, 0.1, dtype), (0.1 * np.random.default_rng(2).standard_normal(ny)).astype(dtype)
    x0 = np.zeros(n, dtype)
    eps = float(np.finfo(dtype).eps)
    prob, st, rows = run_traces(bz, ref, dev, orc, n, mu, y, x0, 30, minimum_gamma=eps, dtype=dtype, ny=ny)
    pr = prob.profile2()
    stats = prob.panoc_stats()
    prob.close()
    base = 1e-9 if dtype == np.float64 else 5e-5
    for k, ex, ez, g_d, g_r, sn_d, sn_r, fused, sens in rows:
        print(f"k={k} ex={ex:.3e} ez={ez:.3e} gamma {g_d:.9g} / {g_r:.9g} sens={sens:.3e}")
    halv, bt = int(stats.n_gamma_halvings), int(stats.n_backtracks)
    print(f"{loss}: gamma halvings {halv}, tau backtracks {bt} in 30 states" + (": NONE occurred" if not halv and not bt else ""))
    for k, ex, ez, g_d, g_r, sn_d, sn_r, fused, sens in rows:
        assert abs(g_d - g_r) <= (1e-12 if dtype == np.float64 else 1e-5) * g_r, k
        assert ex <= max(base, 100 * sens) and ez <= max(base, 100 * sens), (k, ex, ez, sens)
    assert pr["gemv"]["form"].startswith("k_spmv_"), pr["gemv"]["form"]
    assert pr["k_fused_iterates"]["launches"] == 0 and pr["k_fused_sep"]["launches"] == 0


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("loss", NEW)
def test_whole_solves(bz, ref, loss, weighted):
    """bz.alps, resident and through the host outer loop, against ref.alps on sparse_glm(256, 64, 5), plain and with weights and
    the scale 1 / m: first_order on both sides, objective within 1e-4 relative, x within 1e-4 (the bounds of
    tests/test_gpu_sparse_logistic.py).  Iteration counts are printed.
    The scaled problems have lambda and tol_dual scaled by 1 / m too, on both sides: the dual residual of the scaled objective
    is 1 / m of the unscaled one's, so at the default 1e-6 the solution is not determined to the bound — the oracle alone, started
    1e-9 away from x0 = 0, ends 6.6e-4 away on the Poisson problem (107 against 113 inner iterations); with tol_dual / m the same
    two runs end 1.5e-12 apart."""
    lam = 0.5 / 256 if weighted else 0.5
    tols = {"tol_dual": 1e-6 / 256} if weighted else {}
    n, ny, dev, orc = glm_problem(bz, ref, loss, np.float64, weighted, lam=lam)
    fo = orc[0]
    obj = lambda x: float(fo(x) + lam * np.sum(np.abs(x)))
    sub = lambda **kw: bz.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
    subr = lambda **kw: ref.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
    o = ref.alps(*orc, np.zeros(n), np.zeros(ny), subsolver=subr, subsolver_maxit=100000, **tols)
    assert o[5] == "first_order"
    for resident in (True, False):
        a = bz.alps(*dev, np.zeros(n), np.zeros(ny), subsolver=sub, subsolver_maxit=100000, resident=resident, **tols)
        print(f"{loss} weighted={weighted} resident={resident}: status {a[5]} outer {a[2]}/{o[2]} inner {a[3]}/{o[3]} "
              f"obj {obj(a[0]):.9g}/{obj(o[0]):.9g} max|x - x_ref| {np.max(np.abs(a[0] - o[0])):.3e}")
        assert a[5] == "first_order"
        assert abs(obj(a[0]) - obj(o[0])) <= 1e-4 * abs(obj(o[0]))
        assert np.max(np.abs(a[0] - o[0])) <= 1e-4
