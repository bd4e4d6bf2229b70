"""f(x) = sum_i log(1 + exp(-b_i a_i'x)) with a sparse A in CSR (bz.SparseLogistic, BZ_F_SPARSE_LOGISTIC), everything that needs no
GPU: the class's validation and host mirrors, its lowering to the C descriptor, the generator bz.synth.sparse_logistic, and the
launch plans that the case lists of tests/test_gpu_sparse_logistic.py take."""
import ctypes as C

import numpy as np
import pytest

from bazinga_jl_amd.oracles import lower
from tests.test_gpu_sparse import CASES32, CASES64, csr_of, plan, structured, transpose_ptr
from tests.test_sparse_least_squares_host import CUT32


def small():
    indptr, indices, data = np.array([0, 2, 3, 5]), np.array([0, 3, 1, 2, 3]), np.arange(1.0, 6.0)
    return indptr, indices, data, np.array([1.0, -1.0, 1.0]), 4


def dense_logistic(A, b, x):
    """the dense formula in float64: (sum_i softplus(-u_i), A'r) with u = b * (A x), r = -b sigma(-u)"""
    A, b, x = (np.asarray(v, np.float64) for v in (A, b, x))
    u = b * (A @ x)
    loss = np.logaddexp(0.0, -u)
    s = np.where(u >= 0, np.exp(-np.abs(u)), 1.0) / (1.0 + np.exp(-np.abs(u)))
    return float(np.sum(loss)), A.T @ (-b * s)


def test_validation_errors(bz):
    indptr, indices, data, b, n = small()
    f = bz.SparseLogistic(indptr, indices, data, b, n)
    assert f.nnz == 5 and f.n == 4 and f.m == 3
    with pytest.raises(ValueError, match="indptr"):
        bz.SparseLogistic(np.array([0, 3, 2, 5]), indices, data, b, n)
    with pytest.raises(ValueError, match="indptr"):
        bz.SparseLogistic(np.array([1, 2, 3, 5]), indices, data, b, n)
    with pytest.raises(ValueError, match="indptr"):
        bz.SparseLogistic(np.array([0, 2, 3, 4]), indices, data, b, n)               # does not end at nnz
    with pytest.raises(ValueError, match="indptr"):
        bz.SparseLogistic(np.array([0, 2, 5]), indices, data, b, n)                  # not m + 1 long
    with pytest.raises(ValueError, match="column indices"):
        bz.SparseLogistic(indptr, np.array([0, 3, 1, 4, 3]), data, b, n)
    with pytest.raises(ValueError, match="column indices"):
        bz.SparseLogistic(indptr, np.array([0, -1, 1, 2, 3]), data, b, n)
    with pytest.raises(ValueError, match="same length"):
        bz.SparseLogistic(indptr, indices, data[:4], b, n)
    with pytest.raises(ValueError, match="integer"):
        bz.SparseLogistic(indptr.astype(np.float64), indices, data, b, n)
    with pytest.raises(ValueError, match="float64 or float32"):
        bz.SparseLogistic(indptr, indices, data.astype(np.int64), b, n)
    with pytest.raises(ValueError, match="2\\^31"):
        bz.SparseLogistic(indptr, indices, data, b, 2 ** 31)
    with pytest.raises(ValueError, match="2\\^31"):
        bz.SparseLogistic(np.array([0]), indices[:0], data[:0], b[:0], n)            # no rows
    # labels other than -1 / +1
    for bad in (np.array([1.0, 0.0, 1.0]), np.array([1.0, -1.0, 2.0]), np.array([1.0, np.nan, -1.0]), np.array([0.5, -1.0, 1.0])):
        with pytest.raises(ValueError, match="labels"):
            bz.SparseLogistic(indptr, indices, data, bad, n)
    # integer labels are taken in the type of the data
    g = bz.SparseLogistic(indptr, indices, data.astype(np.float32), np.array([1, -1, 1]), n)
    assert g.b.dtype == np.float32 and np.array_equal(g.b, b)
    # a duplicated index contributes twice; nnz = 0 is accepted: every u is 0, f = m log 2 and the gradient is zero
    g = bz.SparseLogistic(np.array([0, 2, 3]), np.array([1, 1, 0]), np.array([2.0, 3.0, 5.0]), np.array([1.0, -1.0]), 2)
    assert np.array_equal(g.toarray(), np.array([[0.0, 5.0], [5.0, 0.0]]))
    e = bz.SparseLogistic(np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0), b, n)
    dfx = np.ones(n)
    assert e.gradient(dfx, np.ones(n)) == 3 * np.log1p(1.0) and not np.any(dfx)


def test_from_dense_round_trip(bz):
    for m, n, p in CASES64[:5]:
        A = structured(m, n, p, np.random.default_rng(m + n), False, np.float64)
        f = bz.SparseLogistic.from_dense(A, np.ones(m))
        assert np.array_equal(f.toarray(), A) and f.nnz == np.count_nonzero(A) and (f.m, f.n) == (m, n)
        assert f.indptr.dtype == np.int64 and f.indices.dtype == np.int32


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_value_and_gradient_against_the_dense_formula(bz, dtype):
    """real data, unsorted rows and a duplicated entry included: within a few roundings of the dtype of the dense float64
    formula (the gradient relative to its largest entry: its entries are sums of about m p terms of either sign)"""
    rng = np.random.default_rng(11)
    m, n = 41, 121
    A = structured(m, n, 0.1, rng, False, dtype)
    indptr, indices, data = csr_of(A, np.random.default_rng(1))
    k = indptr[2]                                             # duplicate the first entry of row 2: 2 a = a + a
    indices, data = np.insert(indices, k, indices[k]), np.insert(data, k, data[k])
    indptr[3:] += 1
    A[2, indices[k]] *= 2
    b = np.where(rng.random(m) < 0.5, -1.0, 1.0).astype(dtype)
    f = bz.SparseLogistic(indptr, indices, data, b, n)
    assert np.array_equal(f.toarray(), A)
    tol = 64 * float(np.finfo(dtype).eps)
    for scale in (1.0, 30.0):
        x = (scale * rng.standard_normal(n)).astype(dtype)
        g = np.empty(n, dtype)
        fx = f.gradient(g, x)
        f_ref, g_ref = dense_logistic(A, b, x)
        assert g.dtype == dtype and type(fx) is dtype and fx == f(x)
        assert abs(float(fx) - f_ref) <= tol * max(1.0, f_ref)
        assert np.max(np.abs(g - g_ref)) <= tol * np.max(np.abs(g_ref))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_formula_at_its_edges(bz, dtype):
    """a diagonal A and x = 1: u_i = b_i t_i.  +-inf, 0, NaN and arguments far beyond where exp overflows"""
    big = 1e300 if dtype == np.float64 else 1e30
    t = np.array([0.0, 1000.0, -1000.0, big, -big, np.inf, -np.inf, np.nan], dtype)
    m = t.shape[0]
    f = bz.SparseLogistic(np.arange(m + 1), np.arange(m), t, np.ones(m), m)
    loss, r = f._loss_r(np.ones(m, dtype))
    assert loss.dtype == r.dtype == dtype
    assert loss[0] == dtype(np.log1p(dtype(1))) and r[0] == -0.5
    assert np.array_equal(loss[1:7], np.array([0, 1000, 0, big, 0, np.inf], dtype))
    assert np.array_equal(r[1:7], np.array([0, -1, 0, -1, 0, -1], dtype))
    assert np.isnan(loss[7]) and np.isnan(r[7])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lower_fills_the_descriptor(bz, dtype):
    L = bz._lib
    indptr, indices, data, b, n = small()
    m, ny = 3, 2
    f = bz.SparseLogistic(indptr, indices, data.astype(dtype), b.astype(dtype), n)
    A = np.zeros((ny, n), dtype)
    A[0, :] = 1
    A[1, 3] = 2
    cs = bz.SparseAffine.from_dense(A, np.zeros(ny, dtype))
    for c, rows in ((bz.IdentityFunction(), n), (cs, ny)):
        desc, keep = lower(f, bz.NormL1(0.1), c, bz.ZeroSet(), n, rows, dtype)
        assert desc.f_kind == L.BZ_F_SPARSE_LOGISTIC == 8 and desc.f_sp_nnz == f.nnz == 5 and desc.f_rows == m
        assert desc.c_kind == (L.BZ_C_SPARSE_AFFINE if c is cs else L.BZ_C_IDENTITY)
        rp = np.ctypeslib.as_array(C.cast(desc.f_sp_rowptr, C.POINTER(C.c_int64)), shape=(m + 1,))
        col = np.ctypeslib.as_array(C.cast(desc.f_sp_col, C.POINTER(C.c_int32)), shape=(f.nnz,))
        ct = C.c_double if dtype == np.float64 else C.c_float
        val = np.ctypeslib.as_array(C.cast(desc.f_sp_val, C.POINTER(ct)), shape=(f.nnz,))
        bb = np.ctypeslib.as_array(C.cast(desc.f_b, C.POINTER(ct)), shape=(m,))
        assert np.array_equal(rp, f.indptr) and np.array_equal(col, f.indices) and np.array_equal(val, f.data)
        assert np.array_equal(bb, b) and not desc.f_A and not desc.f_q
    # a float64 object lowered to a float32 problem: the values and the labels are converted
    f64 = bz.SparseLogistic(indptr, indices, data, b, n)
    desc, keep = lower(f64, bz.NormL1(0.1), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float32)
    val = np.ctypeslib.as_array(C.cast(desc.f_sp_val, C.POINTER(C.c_float)), shape=(5,))
    bb = np.ctypeslib.as_array(C.cast(desc.f_b, C.POINTER(C.c_float)), shape=(m,))
    assert np.array_equal(val, data.astype(np.float32)) and np.array_equal(bb, b.astype(np.float32))


def test_lower_refuses_before_any_device_call(bz):
    indptr, indices, data, b, n = small()
    f = bz.SparseLogistic(indptr, indices, data, b, n)
    A = np.ones((2, n))
    with pytest.raises(bz.UnsupportedOracle, match="SparseLogistic.*slack"):
        lower(f, bz.NormL1(0.1), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64, slack=True)
    with pytest.raises(bz.UnsupportedOracle, match="SparseLogistic.*DenseAffine"):
        lower(f, bz.NormL1(0.1), bz.DenseAffine(A, np.zeros(2)), bz.ZeroSet(), n, 2, np.float64)
    with pytest.raises(bz.UnsupportedOracle, match="pairwise"):
        cs = bz.SparseAffine.from_dense(A, np.zeros(2))
        lower(f, bz.NormL1(0.1), cs, bz.XorPairs(), n, 2, np.float64)
    with pytest.raises(ValueError, match="columns"):
        lower(f, bz.NormL1(0.1), bz.IdentityFunction(), bz.ZeroSet(), n + 1, n + 1, np.float64)
    # the same through bz.Problem, which lowers before it opens a context
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(f, bz.NormL1(1.0), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64, slack=True)
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(f, bz.NormL1(1.0), bz.DenseAffine(A, np.zeros(2)), bz.ZeroSet(), n, 2, np.float64)
    # a g that is not lowered sends the same object through the callback kinds
    class MyL1:
        def prox(self, z, x, gamma):
            z[...] = x
            return 0.0
    desc, keep = lower(f, MyL1(), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64)
    assert desc.f_kind == bz._lib.BZ_F_CALLBACK


def test_sparse_logistic_is_reproducible(bz):
    m, n, k = 256, 64, 5
    a, b = bz.synth.sparse_logistic(m, n, k), bz.synth.sparse_logistic(m, n, k)
    assert all(np.array_equal(a[key], b[key]) for key in a)
    assert not np.array_equal(a["data"], bz.synth.sparse_logistic(m, n, k, seed=7)["data"])
    # sparse_lasso's matrix and planted x*
    las = bz.synth.sparse_lasso(m, n, k)
    assert all(np.array_equal(a[key], las[key]) for key in ("indptr", "indices", "data", "xstar"))
    lab = a["labels"]
    assert lab.dtype == np.float64 and set(np.unique(lab)) == {-1.0, 1.0}
    f = bz.SparseLogistic(a["indptr"], a["indices"], a["data"], lab, n)
    margin = f.toarray() @ a["xstar"]
    want = np.where(margin + 0.1 * (2.0 * bz.synth.uniform(9, m) - 1.0) >= 0, 1.0, -1.0)
    near = np.abs(np.abs(margin) - 0.1) < 1e-9               # (the margin is summed in another order here)
    assert np.array_equal(lab[~near], want[~near])
    assert np.all(lab[np.abs(margin) > 0.1 + 1e-9] == np.sign(margin[np.abs(margin) > 0.1 + 1e-9]))
    c = bz.synth.sparse_logistic(m, n, k, np.float32)
    assert c["data"].dtype == c["labels"].dtype == np.float32 and np.array_equal(c["indices"], a["indices"])
    with pytest.raises(ValueError):
        bz.synth.sparse_logistic(4, 3, 5)


def test_case_lists_take_every_lane_count_and_cut_rows_on_both_matrices():
    """the (m, n, density) lists of tests/test_gpu_sparse.py as A_f, with the generator seeds of tests/test_gpu_sparse_logistic.py:
    L = 1 .. 64 on A_f and on A_f'; in fp64 cut rows on each side; the two extra fp32 shapes (real data) are cut on each side"""
    for cases in (CASES64, CASES32):
        la, lt, cut_a, cut_t = set(), set(), False, False
        for m, n, p in cases:
            A = structured(m, n, p, np.random.default_rng(m * 7 + n), True, np.float64)
            indptr, indices, data = csr_of(A, np.random.default_rng(1))
            a, t = plan(indptr, data.shape[0]), plan(transpose_ptr(indices, n), data.shape[0])
            la.add(a[0]); lt.add(t[0]); cut_a, cut_t = cut_a or a[2], cut_t or t[2]
        assert la == lt == {1, 2, 4, 8, 16, 32, 64}, (la, lt)
        assert (cut_a and cut_t) or cases is CASES32
    for (m, n, p), side in zip(CUT32, (0, 1)):
        A = structured(m, n, p, np.random.default_rng(m * 11 + n), False, np.float32)
        indptr, indices, data = csr_of(A, np.random.default_rng(2))
        cuts = (plan(indptr, data.shape[0])[2], plan(transpose_ptr(indices, n), data.shape[0])[2])
        assert cuts[side] and not cuts[1 - side]
