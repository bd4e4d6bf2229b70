"""f(x) = sum_i log(1 + exp(-b_i a_i'x)) with a sparse A in CSR on the device (BZ_F_SPARSE_LOGISTIC): the row kernel over A_f with
the logistic epilogue (k_spmv_logit_r: r_i = -b_i sigma(-b_i a_i'x) and the rows' losses), then the kernels over A_f' that the
sparse least squares f has (k_spmv_ls_t_algrad: the whole AL gradient of c = Identity in two launches; k_spmv_ls_t, the plain
product for the three-launch form and beside a sparse c), the epilogue element by element, the iterates and whole solves against
the oracle, creation-time validation.

The reference package has no logistic loss: the oracle for f is the numpy class below (the formula of include/bazinga_hip.h in
the problem's dtype, its sums through ref._sum / ref._dot), driven by the unmodified ref.AugLagFun, ref.PANOCplusIteration and
ref.alps; c is ref.IdentityFunction or the CSR duck-type of tests/test_gpu_sparse.py."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_parity import run_traces
from tests.test_gpu_sparse import CASES32, CASES64, CsrOracle, csr_of, plan, sets, structured, transpose_ptr
from tests.test_sparse_least_squares_host import CUT32

pytestmark = pytest.mark.gpu

IDS = lambda c: f"{'f64' if c[0] == np.float64 else 'f32'}-{c[1][0]}x{c[1][1]}-{c[1][2]}"
TYPED = [(np.float64, c) for c in CASES64] + [(np.float32, c) for c in CASES32]
# a sparse c beside the sparse f: the shapes of tests/test_gpu_sparse_least_squares.py
PAIRS = [((41, 121, 0.1), (30, 0.2)), ((257, 1031, 0.03), (41, 0.1))]
PAIR_IDS = lambda c: f"{'f64' if c[0] == np.float64 else 'f32'}-{c[1][0][0]}x{c[1][0][1]}+{c[1][1][0]}"
TOL = {np.float64: 1e-12, np.float32: 2e-5}
# exp(-X0) is exactly 0 in the type: a row sum of X0 * (an integer) gives exp(-|u|) in {0, 1}
X0 = {np.float64: 1024.0, np.float32: 128.0}


def ref_module():
    from oracle import bazinga_ref
    return bazinga_ref


class LogisticOracle:
    """f(x) = sum_i softplus(-u_i), u = b * (A x) on a dense A, in the dtype of x; gradient A'r with r = -b sigma(-u).  The
    row and column sums through ref._dot and the value through ref._sum, so that a reducer set on the oracle carries them
    (under the default reducer, whose dot is numpy's, the rows' dots are one matrix product)."""

    def __init__(self, A, b):
        self.A, self.b = np.asarray(A), np.asarray(b)
        self.At = np.ascontiguousarray(self.A.T)

    @staticmethod
    def dots(M, v):
        ref = ref_module()
        if isinstance(ref.REDUCER, ref.LocalReducer):
            return M @ v
        return np.array([ref._dot(row, v) for row in M], v.dtype)

    def loss_r(self, x):
        dt = x.dtype.type
        t = self.dots(self.A, x)
        u = self.b * t
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp(-np.abs(u))
            loss = np.where(u < 0, -u, dt(0)) + np.log1p(e)
            s = np.where(u >= 0, e / (dt(1) + e), dt(1) / (dt(1) + e))
        return loss, -self.b * s

    def __call__(self, x):
        return x.dtype.type(ref_module()._sum(self.loss_r(x)[0]))

    def gradient(self, y, x):
        ref = ref_module()
        loss, r = self.loss_r(x)
        y[...] = self.dots(self.At, r)
        return x.dtype.type(ref._sum(loss))


def labels_of(rng, m, dtype):
    return np.where(rng.random(m) < 0.5, -1.0, 1.0).astype(dtype)


def sparse_logit(bz, A, b, seed=1):
    indptr, indices, data = csr_of(A, np.random.default_rng(seed))
    return bz.SparseLogistic(indptr, indices, data, b, A.shape[1]), indptr, indices, data.shape[0]


def one_gradient(bz, dev, n, ny, dtype, mu, y, x, times=1):
    prob = bz.Problem(*dev, n, ny, dtype)
    prob.set_multipliers(mu, y)
    prob.profile_reset()
    prob.profile_enable(True)
    runs = [prob.eval_al_gradient(x) for _ in range(times)]
    pr = prob.profile2()
    prob.close()
    return runs[0] if times == 1 else runs, pr


# ---- 1. creation and refusals through the raw ABI
def raw_desc(bz, indptr, indices, data, b, n, slack=0, c=None, ny=None):
    from bazinga_jl_amd.oracles import lower
    m = b.shape[0]
    good = bz.SparseLogistic(np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), b, n)
    desc, keep = lower(good, bz.NormL1(1.0), c or bz.IdentityFunction(), bz.ZeroSet(), n, ny or n, np.float64)
    arrs = (np.ascontiguousarray(indptr, np.int64), np.ascontiguousarray(indices, np.int32), np.ascontiguousarray(data, np.float64))
    desc.f_sp_rowptr, desc.f_sp_col, desc.f_sp_val = (a.ctypes.data for a in arrs)
    desc.f_sp_nnz = arrs[1].shape[0]
    desc.slack = slack
    return desc, (keep, arrs)


def test_creation_validates_the_matrix_and_refuses_what_is_not_lowered(bz, ref):
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

    desc, keep = raw_desc(bz, indptr, indices, data, b, n)
    assert desc.f_kind == 8 and create(desc)[:2] == (0, True)
    cs = bz.SparseAffine.from_dense(np.array([[1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 2.0]]), np.zeros(2))
    desc, keep = raw_desc(bz, indptr, indices, data, b, n, c=cs, ny=2)
    assert desc.c_kind == L.BZ_C_SPARSE_AFFINE and create(desc)[:2] == (0, True)
    for bad_ptr, row in ((np.array([0, 3, 2, 5]), "row 1"), (np.array([1, 2, 3, 5]), "row 0")):
        desc, keep = raw_desc(bz, bad_ptr, indices, data, b, n)
        rc, made, msg = create(desc)
        assert rc == L.BZ_ERR_ARG and not made and row in msg and "SparseLogistic" in msg, msg
    desc, keep = raw_desc(bz, np.array([0, 2, 3, 4]), indices, data, b, n)               # rowptr[m] != nnz
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_ARG and not made and "nnz" in msg and "row 2" in msg and "SparseLogistic" in msg, msg
    desc, keep = raw_desc(bz, indptr, np.array([0, 3, 1, 4, 3]), data, b, n)             # a column = n, in row 2
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_ARG and not made and "row 2" in msg and "SparseLogistic" in msg, msg
    desc, keep = raw_desc(bz, indptr, indices, data, b, n)
    desc.f_rows = 0
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_ARG and not made and "SparseLogistic" in msg, msg
    desc, keep = raw_desc(bz, indptr, indices, data, b, n)
    desc.f_b = None
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_ARG and not made and "SparseLogistic" in msg, msg
    # the four refusals
    desc, keep = raw_desc(bz, indptr, indices, data, b, n, slack=1)
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_UNSUPPORTED and not made and "slack" in msg and "SparseLogistic" in msg, msg
    desc, keep = raw_desc(bz, indptr, indices, data, b, n)
    A, b2 = np.ones((2, n)), np.zeros(2)
    desc.c_kind, desc.ny, desc.c_A, desc.c_b = L.BZ_C_DENSE_AFFINE, 2, A.ctypes.data, b2.ctypes.data
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_UNSUPPORTED and not made and "DenseAffine" in msg and "SparseLogistic" in msg, msg
    ctx2 = bz.Context(device=0, rank=0, nranks=2, comm_id=None)
    desc, keep = raw_desc(bz, indptr, indices, data, b, n)
    rc, made, msg = create(desc, ctx2)
    assert rc == L.BZ_ERR_UNSUPPORTED and not made and "one rank" in msg and "SparseLogistic" in msg, msg
    desc, keep = raw_desc(bz, indptr, indices, data, b, n)
    desc.g_kind = L.BZ_G_CALLBACK
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_UNSUPPORTED and not made and "callbacks" in msg and "SparseLogistic" in msg, msg
    # the Python layer raises before any device call
    f = bz.SparseLogistic(indptr, indices, data, b, n)
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(f, bz.NormL1(1.0), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64, slack=True)
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(f, bz.NormL1(1.0), bz.DenseAffine(A, np.zeros(2)), bz.ZeroSet(), n, 2, np.float64)


# ---- 2. the gradient bit for bit where the transcendental functions are exact
def integer_inputs(m, n, p, ny, dtype, regime):
    """A_f of {-2, -1, 1, 2} under a density-p mask (structured), labels +-1, y in [-3, 3], mu = 1/4, and x = 0 ("zero") or
    X0 times integers of [-4, 4] ("far"): every u is 0, or at least X0 in size"""
    rng = np.random.default_rng(m * 7 + n)
    A = structured(m, n, p, rng, True, dtype)
    b = labels_of(rng, m, dtype)
    x = (X0[dtype] * rng.integers(-4, 5, n)).astype(dtype)
    if regime == "zero":
        x = np.zeros(n, dtype)
    return A, b, x, rng.integers(-3, 4, ny).astype(dtype), np.full(ny, 0.25, dtype), rng


def assert_exact_in(dtype, A, b, x, y, make_al, g_ref, Ac=None, bc=None):
    """Exactness of the gradient, whatever the order of any sum, asserted on the oracle's float64 recomputation
    (make_al(np.float64)): every u is 0 or at least X0 in size (so exp(-|u|) is 0 or 1 and sigma in {0, 1/2, 1} in both types);
    the sums of magnitudes that bound every partial sum — of a row of A_f x, of a row of A_f' r in halves plus the penalty part
    of the gradient (beside a sparse c: of a row of A_c x - b_c in quarters and of A_c' yhat) — stay below a tenth of 2^24
    (fp32) / 2^53 (fp64).  Then the oracle in dtype has returned the exact gradient A_f' r + (the penalty part), r in {0, -+1/2, -+1}."""
    lim = 2.0 ** (24 if dtype == np.float32 else 53) / 10
    x64, absA = x.astype(np.float64), np.abs(A.astype(np.float64))
    al64, lx64, g64 = make_al(np.float64)
    u = b.astype(np.float64) * (A.astype(np.float64) @ x64)
    assert np.all((u == 0) | (np.abs(u) >= X0[dtype]))
    assert np.exp(dtype(-X0[dtype])) == 0
    r = -b.astype(np.float64) * np.where(u == 0, 0.5, np.where(u > 0, 0.0, 1.0))
    yhat = al64.yupd
    assert np.max(absA @ np.abs(x64)) < lim
    pen_part = np.max(np.abs(yhat))
    if Ac is not None:
        absC = np.abs(Ac.astype(np.float64))
        assert 4 * np.max(absC @ np.abs(x64) + np.abs(bc)) < lim
        pen_part = np.max(absC.T @ np.abs(yhat))
    assert 2 * (np.max(absA.T @ np.abs(r)) + pen_part) < lim
    # (the closed form, not g64: with the fp32 X0 the float64 oracle still sees exp(-128) = 2.6e-56)
    exact = A.astype(np.float64).T @ r + (yhat if Ac is None else Ac.astype(np.float64).T @ yhat)
    assert np.array_equal(g_ref.astype(np.float64), exact)


def exact_identity(bz, ref, dtype, case, D_name, regime):
    m, n, p = case
    A, b, x, y, mu, _ = integer_inputs(m, n, p, n, dtype, regime)
    f, indptr, indices, nnz = sparse_logit(bz, A, b)
    (g_dev, vals), pr = one_gradient(bz, (f, bz.NormL1(1.0), bz.IdentityFunction(), sets(bz, ref, D_name, dtype)[0]), n, n, dtype, mu, y, x)

    def make_al(dt):
        al = ref.AugLagFun(LogisticOracle(A.astype(dt), b.astype(dt)), ref.IdentityFunction(), sets(bz, ref, D_name, dt)[1],
                           mu.astype(dt), y.astype(dt), x.astype(dt))
        g = np.empty(n, dt)
        return al, al.gradient(g, x.astype(dt)), g
    al, lx, g_ref = make_al(dtype)
    assert_exact_in(dtype, A, b, x, y, make_al, g_ref)
    assert g_dev.dtype == dtype and np.array_equal(g_dev, g_ref)
    # (the value: log1p(1) need not agree in its last bit between two libraries)
    lx, fx = float(lx), float(al.fx)
    assert abs(vals[0] - lx) <= TOL[dtype] * max(1.0, abs(lx)) and abs(vals[1] - fx) <= TOL[dtype] * max(1.0, abs(fx))
    return pr, plan(indptr, nnz), plan(transpose_ptr(indices, n), nnz)


@pytest.mark.parametrize("regime", ["zero", "far"])
@pytest.mark.parametrize("D", ["zero", "free", "box"])
@pytest.mark.parametrize("case", TYPED, ids=IDS)
def test_exact_gradient_bit_for_bit(bz, ref, case, D, regime):
    """Integer A, labels +-1, mu = 1/4, integer y, and x = 0 (every u = 0: r = -b/2) or x = X0 * integers (every u is 0 or
    beyond where exp(-|u|) is 0: sigma in {0, 1/2, 1}): every product and every sum is exact, so no summation order can change
    a bit of the gradient, which equals the oracle's BIT FOR BIT.  Two row launches, no element-wise kernel."""
    dtype, shape = case
    pr, (La, _, seg_a), (Lt, _, seg_t) = exact_identity(bz, ref, dtype, shape, D, regime)
    assert pr["gemv"]["form"] == f"k_spmv_ls_t_algrad<L={Lt},SEG={int(seg_t)}>", pr["gemv"]["form"]
    assert pr["gemv"]["launches"] == 2 and pr["al_gradient"]["launches"] == 0
    assert pr["misc"]["launches"] == int(seg_a) + int(seg_t)                  # a fold launch per cut matrix


@pytest.mark.parametrize("case", [(np.float64, (257, 1031, 0.9)), (np.float64, (1031, 257, 0.9)), (np.float32, (41, 121, 0.25))], ids=IDS)
def test_exact_gradient_in_the_three_launch_form(bz, ref, case, monkeypatch):
    """BZ_SPLS_FUSED=0 on the exact data (x = X0 * integers): the plain product over A_f' and k_algrad_elem in its mode 1, bit
    for bit too"""
    dtype, shape = case
    monkeypatch.setenv("BZ_SPLS_FUSED", "0")
    pr, _, (Lt, _, seg_t) = exact_identity(bz, ref, dtype, shape, "box", "far")
    assert pr["gemv"]["form"] == f"k_spmv_ls_t<L={Lt},SEG={int(seg_t)}>", pr["gemv"]["form"]
    assert pr["gemv"]["launches"] == 2 and pr["al_gradient"]["launches"] == 1


# ---- 3. the general gradient, and 5. the forms
def real_inputs(m, n, p, ny, dtype):
    rng = np.random.default_rng(m * 11 + n)
    A = structured(m, n, p, rng, False, dtype)
    return (A, labels_of(rng, m, dtype), rng.standard_normal(n).astype(dtype), rng.standard_normal(ny).astype(dtype),
            (10.0 ** rng.uniform(-2, 0, ny)).astype(dtype), rng)


def general_runs(bz, ref, dtype, shape, D, monkeypatch):
    m, n, p = shape
    A, b, x, y, mu, _ = real_inputs(m, n, p, n, dtype)
    Dd, Dr = sets(bz, ref, D, dtype)
    out = {}
    for kind in ("fused", "three"):
        monkeypatch.setenv("BZ_SPLS_FUSED", "0" if kind == "three" else "1")
        f = sparse_logit(bz, A, b, seed=2)[0]
        out[kind], pr = one_gradient(bz, (f, bz.NormL1(1.0), bz.IdentityFunction(), Dd), n, n, dtype, mu, y, x)
        assert (pr["gemv"]["launches"], pr["al_gradient"]["launches"]) == ((2, 0) if kind == "fused" else (2, 1))
    al = ref.AugLagFun(LogisticOracle(A, b), ref.IdentityFunction(), Dr, mu.copy(), y.copy(), x)
    g_ref = np.empty(n, dtype)
    lx = float(al.gradient(g_ref, x))
    return out, g_ref, lx, float(al.fx), TOL[dtype], np.max(np.abs(g_ref))


GENERAL = TYPED + [(np.float32, c) for c in CUT32]


@pytest.mark.parametrize("D", ["zero", "box"])
@pytest.mark.parametrize("case", GENERAL, ids=IDS)
def test_general_gradient_against_the_oracle_and_between_the_forms(bz, ref, case, D, monkeypatch):
    """random real data against the numpy oracle: 1e-12 / 2e-5 of the gradient's largest entry, of max(1, |L|) for the value
    (the rule and the numbers of tests/test_gpu_sparse_least_squares.py).  And the gradient under BZ_SPLS_FUSED=0 equals the
    default's BIT FOR BIT (the same row sums, the same element operations); f comes from the first launch in both forms."""
    dtype, shape = case
    out, g_ref, lx, fx, tol, scale = general_runs(bz, ref, dtype, shape, D, monkeypatch)
    (g_dev, vals), (g3, vals3) = out["fused"], out["three"]
    print(f"max|g - g_ref| / max|g_ref| = {np.max(np.abs(g_dev.astype(np.float64) - g_ref)) / scale:.3e}, "
          f"value {abs(vals[0] - lx) / max(1.0, abs(lx)):.3e}, f {abs(vals[1] - fx) / max(1.0, abs(fx)):.3e}, "
          f"forms equal {np.array_equal(g_dev, g3)}")
    assert np.max(np.abs(g_dev.astype(np.float64) - g_ref)) <= tol * scale
    assert abs(vals[0] - lx) <= tol * max(1.0, abs(lx))
    assert abs(vals[1] - fx) <= tol * max(1.0, abs(fx))
    assert np.array_equal(g_dev, g3)
    assert abs(vals3[0] - lx) <= tol * max(1.0, abs(lx)) and vals[1] == vals3[1]


def test_pairwise_D_takes_the_three_launch_form(bz, ref):
    """XOR pairs, c = Identity, n even: the projection of an element needs its partner, so the gradient is k_spmv_logit_r, the
    plain product and k_algrad_elem whatever BZ_SPLS_FUSED says; within the tolerance of the general test"""
    m, n = 41, 120
    A, b, x, y, mu, _ = real_inputs(m, n, 0.1, n, np.float64)
    f = sparse_logit(bz, A, b)[0]
    (g_dev, vals), pr = one_gradient(bz, (f, bz.Zero(), bz.IdentityFunction(), bz.XorPairs()), n, n, np.float64, mu, y, x)
    assert pr["gemv"]["launches"] == 2 and pr["gemv"]["form"].startswith("k_spmv_ls_t<L=") and pr["al_gradient"]["launches"] == 1
    al = ref.AugLagFun(LogisticOracle(A, b), ref.IdentityFunction(), ref.PairwiseSet("xor"), mu.copy(), y.copy(), x)
    g_ref = np.empty(n)
    lx = float(al.gradient(g_ref, x))
    assert np.max(np.abs(g_dev - g_ref)) <= 1e-12 * np.max(np.abs(g_ref)) and abs(vals[0] - lx) <= 1e-12 * max(1.0, abs(lx))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_launches_of_two_gradients_and_identical_runs(bz, ref, dtype):
    """c = Identity, two gradients: four row launches and no k_algrad_elem launch; the same bits on both runs; the bytes of
    the model are those of the least-squares kind (per row of A_f the label and r)"""
    m, n = 257, 500
    A, b, x, y, mu, _ = real_inputs(m, n, 0.03, n, dtype)
    f, indptr, indices, nnz = sparse_logit(bz, A, b)
    runs, pr = one_gradient(bz, (f, bz.NormL1(1.0), bz.IdentityFunction(), bz.ZeroSet()), n, n, dtype, mu, y, x, times=2)
    assert pr["gemv"]["launches"] == 4 and pr["al_gradient"]["launches"] == 0 and pr["misc"]["launches"] == 0
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    sz = np.dtype(dtype).itemsize
    La, nva, _ = plan(indptr, nnz)
    Lt, nvt, _ = plan(transpose_ptr(indices, n), nnz)
    model = 2 * nnz * (sz + 4) + (nva + 1) * 8 + (nvt + 1) * 8 + (n + m) * sz + 2 * m * sz + 4 * n * sz
    assert pr["gemv"]["bytes"] == 2 * model, (pr["gemv"], model)


# ---- 4. the epilogue element by element
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_epilogue_element_by_element(bz, ref, dtype):
    """A_f diagonal, n = 1024, x = ones: row i has u = b_i t_i.  t: 1000 points of linspace(-90, 90), +-700, +-1e3, +-1e30 /
    +-1e300, two NaN, the smallest normal number (and +-1 up to n).  mu = 1, y = 0, D = free: the penalty part of the gradient
    is zero and grad_i = t_i r_i, so r_i = grad_i / t_i.  Against the oracle's r relative per element, 1e-12 / 2e-5; NaN and
    the infinities of the gradient in the oracle's places.  (A naive log(1 + exp(-u)) or 1 / (1 + exp(u)) loses r at
    |u| beyond about 40 and overflows beyond 710 / 88.)"""
    n = 1024
    big = 1e300 if dtype == np.float64 else 1e30
    special = [700.0, -700.0, 1e3, -1e3, big, -big, np.nan, np.nan, float(np.finfo(dtype).tiny)]
    t = np.concatenate((np.linspace(-90.0, 90.0, 1000), special, np.resize([1.0, -1.0], n - 1000 - len(special)))).astype(dtype)
    b = np.resize(np.array([1.0, 1.0, -1.0], dtype), n)                      # both signs of u at both signs of t
    f = bz.SparseLogistic(np.arange(n + 1), np.arange(n), t, b, n)
    x, y, mu = np.ones(n, dtype), np.zeros(n, dtype), np.ones(n, dtype)
    (g_dev, vals), pr = one_gradient(bz, (f, bz.Zero(), bz.IdentityFunction(), bz.FreeSet()), n, n, dtype, mu, y, x)
    loss_ref, r_ref = LogisticOracle(np.diag(t), b).loss_r(x)
    g_ref = t * r_ref
    assert g_dev.dtype == dtype
    assert np.array_equal(np.isnan(g_dev), np.isnan(g_ref)) and np.count_nonzero(np.isnan(g_ref)) == 2
    assert np.array_equal(np.isinf(g_dev), np.isinf(g_ref)) and np.array_equal(np.sign(g_dev[np.isinf(g_ref)]), np.sign(g_ref[np.isinf(g_ref)]))
    ok = np.isfinite(g_ref)
    with np.errstate(invalid="ignore"):
        r_dev = g_dev / t
    err = np.abs(r_dev[ok].astype(np.float64) - r_ref[ok].astype(np.float64))
    bound = TOL[dtype] * np.abs(r_ref[ok].astype(np.float64))
    worst = int(np.argmax(err - bound))
    print(f"worst element: t = {t[ok][worst]!r}, r_dev = {r_dev[ok][worst]!r}, r_ref = {r_ref[ok][worst]!r}; "
          f"max relative error over r_ref != 0: {np.max(err[bound > 0] / np.abs(r_ref[ok][bound > 0].astype(np.float64))):.3e}")
    assert np.all(err <= bound)
    # the edge values: u = 0 is not in t; far out, sigma is exactly 0 or 1
    far = ok & (np.abs(t) >= 1e3)
    assert np.array_equal(r_dev[far], np.where(b[far] * t[far] > 0, 0.0, -b[far]).astype(dtype))
    assert np.isnan(vals[0]) and np.isnan(vals[1])                           # the two NaN rows reach the value too


def test_epilogue_edge_values(bz, ref):
    """u = +inf: loss 0, s 0 ; u = -inf: loss +inf, s 1 ; u = 0: loss log 2, s 1/2 — through a diagonal A_f whose entries are
    +-DBL_MAX with x = 2 (the row sum overflows to +-inf) and 0"""
    dtype = np.float64
    n = 4
    top = float(np.finfo(dtype).max)
    b = np.array([1.0, 1.0, 1.0, -1.0])
    x, y, mu = np.full(n, 2.0), np.zeros(n), np.ones(n)
    # rows 0 and 2 alone (u = +inf, 0): the value is log 2 and r = (0, -1/2)
    f = bz.SparseLogistic(np.array([0, 1, 1, 2, 2]), np.array([0, 2]), np.array([top, 0.0]), b, n)
    (g, vals), _ = one_gradient(bz, (f, bz.Zero(), bz.IdentityFunction(), bz.FreeSet()), n, n, dtype, mu, y, x)
    assert abs(vals[1] - 3 * np.log(2.0)) <= 1e-12 * 3 * np.log(2.0)          # (rows 1 and 3 are empty: u = 0 too)
    assert g[0] == 0.0 and g[2] == 0.0 and not np.any(g[[1, 3]])
    # u = -inf in rows 0 (b = 1, t = -inf) and 3 (b = -1, t = +inf): loss +inf, r = -b, so grad = a * r = +inf in both
    f = bz.SparseLogistic(np.array([0, 1, 1, 1, 2]), np.array([0, 3]), np.array([-top, top]), b, n)
    (g, vals), _ = one_gradient(bz, (f, bz.Zero(), bz.IdentityFunction(), bz.FreeSet()), n, n, dtype, mu, y, x)
    assert vals[1] == np.inf and g[0] == top and g[3] == top and not np.any(g[[1, 2]])


# ---- 6. the empty matrix
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_empty_matrix_is_m_log_2(bz, ref, dtype):
    """nnz = 0 is accepted: every u is 0, f = m log 2 within the tolerance and the gradient is the penalty part alone, bit for
    bit on integer data"""
    m, n = 23, 37
    rng = np.random.default_rng(8)
    b = labels_of(rng, m, dtype)
    x, y = (rng.integers(-3, 4, k).astype(dtype) for k in (n, n))
    mu = np.full(n, 0.25, dtype)
    f = bz.SparseLogistic(np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, dtype), b, n)
    Dd, Dr = sets(bz, ref, "box", dtype)
    (g_dev, vals), _ = one_gradient(bz, (f, bz.NormL1(1.0), bz.IdentityFunction(), Dd), n, n, dtype, mu, y, x)
    al = ref.AugLagFun(LogisticOracle(np.zeros((m, n), dtype), b), ref.IdentityFunction(), Dr, mu.copy(), y.copy(), x)
    g_ref = np.empty(n, dtype)
    lx = float(al.gradient(g_ref, x))
    assert np.array_equal(g_dev, g_ref) and np.array_equal(g_dev, al.yupd)
    assert abs(vals[1] - m * np.log(2.0)) <= TOL[dtype] * m * np.log(2.0)
    assert abs(vals[0] - lx) <= TOL[dtype] * max(1.0, abs(lx))


# ---- 7. beside a sparse c
def beside_sparse_c(bz, ref, dtype, pair, integer):
    (m, n, pf), (ny, pc) = pair
    A, b, x, y, mu, rng = integer_inputs(m, n, pf, ny, dtype, "zero") if integer else real_inputs(m, n, pf, ny, dtype)
    Ac = structured(ny, n, pc, rng, integer, dtype)
    bc = (rng.integers(-3, 4, ny) if integer else rng.standard_normal(ny)).astype(dtype)
    c_ptr, c_idx, c_val = csr_of(Ac, np.random.default_rng(3))
    f = sparse_logit(bz, A, b)[0]
    dev = (f, bz.NormL1(1.0), bz.SparseAffine(c_ptr, c_idx, c_val, bc, n), sets(bz, ref, "box", dtype)[0])
    runs, pr = one_gradient(bz, dev, n, ny, dtype, mu, y, x, times=2)

    def make_al(dt):
        al = ref.AugLagFun(LogisticOracle(A.astype(dt), b.astype(dt)), CsrOracle(c_ptr, c_idx, c_val.astype(dt), bc.astype(dt), n),
                           sets(bz, ref, "box", dt)[1], mu.astype(dt), y.astype(dt), x.astype(dt))
        g = np.empty(n, dt)
        return al, al.gradient(g, x.astype(dt)), g
    # two gradients: k_spmv_logit_r, k_spmv_ls_t, k_spmv_yupd, k_spmv_t_finish each, no element-wise kernel; the same bits
    assert pr["gemv"]["launches"] == 8 and pr["al_gradient"]["launches"] == 0
    assert pr["gemv"]["form"].startswith("k_spmv_t_finish<L="), pr["gemv"]["form"]
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    return runs[0], make_al, (A, b, x, y, Ac, bc)


@pytest.mark.parametrize("case", [(t, c) for t in (np.float64, np.float32) for c in PAIRS], ids=PAIR_IDS)
def test_general_gradient_beside_a_sparse_c(bz, ref, case):
    dtype, pair = case
    (g_dev, vals), make_al, _ = beside_sparse_c(bz, ref, dtype, pair, False)
    al, lx, g_ref = make_al(dtype)
    lx = float(lx)
    tol = TOL[dtype]
    scale = np.max(np.abs(g_ref))
    print(f"max|g - g_ref| / max|g_ref| = {np.max(np.abs(g_dev.astype(np.float64) - g_ref)) / scale:.3e}, "
          f"value {abs(vals[0] - lx) / max(1.0, abs(lx)):.3e}")
    assert np.max(np.abs(g_dev.astype(np.float64) - g_ref)) <= tol * scale
    assert abs(vals[0] - lx) <= tol * max(1.0, abs(lx))


@pytest.mark.parametrize("case", [(t, c) for t in (np.float64, np.float32) for c in PAIRS], ids=PAIR_IDS)
def test_exact_gradient_beside_a_sparse_c(bz, ref, case):
    """integer data and x = 0 beside c(x) = A_c x - b_c in CSR with another row count: the gradient bit for bit the oracle's"""
    dtype, pair = case
    (g_dev, vals), make_al, (A, b, x, y, Ac, bc) = beside_sparse_c(bz, ref, dtype, pair, True)
    al, lx, g_ref = make_al(dtype)
    assert_exact_in(dtype, A, b, x, y, make_al, g_ref, Ac, bc)
    assert g_dev.dtype == dtype and np.array_equal(g_dev, g_ref)
    lx = float(lx)
    assert abs(vals[0] - lx) <= TOL[dtype] * max(1.0, abs(lx))


# ---- 8. the iterates, 9. whole solves
def logistic_problem(bz, ref, dtype, beside_c):
    """sparse_logistic(256, 64, 5): NormL1(0.5), c = Identity, D = box(-5, 5) ; or beside the constraints of budget_bands(64, 10)
    with g = IndBox(0, 1)"""
    m, n = 256, 64
    d = bz.synth.sparse_logistic(m, n, 5, dtype)
    f = bz.SparseLogistic(d["indptr"], d["indices"], d["data"], d["labels"], n)
    fo = LogisticOracle(f.toarray(), d["labels"])
    if not beside_c:
        dev = (f, bz.NormL1(0.5), bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(-5.0, 5.0)))
        orc = (fo, ref.NormL1(0.5), ref.IdentityFunction(), ref.ClosedSet(ref.IndBox(dtype(-5), dtype(5))))
        return n, n, dev, orc
    bb = bz.synth.budget_bands(n, 10, dtype)
    csr = (bb["indptr"], bb["indices"], bb["data"], bb["b"], n)
    dev = (f, bz.IndBox(0.0, 1.0), bz.SparseAffine(*csr), bz.ClosedSet(bz.IndBox(bb["lo"], bb["hi"])))
    orc = (fo, ref.IndBox(dtype(0), dtype(1)), CsrOracle(*csr), ref.ClosedSet(ref.IndBox(bb["lo"], bb["hi"])))
    return n, 11, dev, orc


@pytest.mark.parametrize("beside_c,dtype", [(False, np.float64), (False, np.float32), (True, np.float64)])
def test_iterates_follow_the_oracle(bz, ref, beside_c, dtype):
    """30 states: x and z inside max(base, 100 * sens) — base 1e-9 / 5e-5, sens the oracle's own extended-precision
    envelope — and gamma equal to 1e-12 / 1e-5 relative: the rule and the numbers of tests/test_gpu_sparse_least_squares.py.
    The curvature of this f changes with x: the gamma halvings and tau backtracks that occurred are printed."""
    n, ny, dev, orc = logistic_problem(bz, ref, dtype, beside_c)
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
    print(f"gamma halvings {halv}, tau backtracks {bt} in 30 states" + (": NONE occurred" if not halv and not bt else ""))
    for k, ex, ez, g_d, g_r, sn_d, sn_r, fused, sens in rows:
        assert abs(g_d - g_r) <= (1e-12 if dtype == np.float64 else 1e-5) * g_r, k
        assert ex <= max(base, 100 * sens) and ez <= max(base, 100 * sens), (k, ex, ez, sens)
    assert pr["gemv"]["form"].startswith("k_spmv_"), pr["gemv"]["form"]
    assert pr["k_fused_iterates"]["launches"] == 0 and pr["k_fused_sep"]["launches"] == 0


@pytest.mark.parametrize("beside_c", [False, True])
def test_whole_solves(bz, ref, beside_c):
    """bz.alps, resident and through the host outer loop, against ref.alps: first_order on both sides, feasibility <= 1e-5,
    objective within 1e-4 relative, x within 1e-4 (the bounds of tests/test_gpu_sparse_least_squares.py).  Iteration counts
    are printed."""
    n, ny, dev, orc = logistic_problem(bz, ref, np.float64, beside_c)
    fo = orc[0]
    lo, hi = orc[3].f.lb, orc[3].f.ub
    obj = (lambda x: float(fo(x))) if beside_c else (lambda x: float(fo(x) + 0.5 * np.sum(np.abs(x))))

    def feas_of(x):
        cx = np.empty(ny)
        orc[2].eval(cx, x)
        return float(np.max(np.abs(cx - np.clip(cx, lo, hi))))
    sub = lambda **kw: bz.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
    subr = lambda **kw: ref.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
    o = ref.alps(*orc, np.zeros(n), np.zeros(ny), subsolver=subr, subsolver_maxit=100000)
    assert o[5] == "first_order"
    for resident in (True, False):
        a = bz.alps(*dev, np.zeros(n), np.zeros(ny), subsolver=sub, subsolver_maxit=100000, resident=resident)
        feas = feas_of(a[0])
        print(f"beside_c={beside_c} resident={resident}: status {a[5]} outer {a[2]}/{o[2]} inner {a[3]}/{o[3]} feas {feas:.3e} "
              f"obj {obj(a[0]):.9g}/{obj(o[0]):.9g} max|x - x_ref| {np.max(np.abs(a[0] - o[0])):.3e}")
        assert a[5] == "first_order"
        assert feas <= 1e-5
        assert abs(obj(a[0]) - obj(o[0])) <= 1e-4 * abs(obj(o[0]))
        assert np.max(np.abs(a[0] - o[0])) <= 1e-4
