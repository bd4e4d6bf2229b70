"""c(x) = A x - b with A in CSR (bz.SparseAffine, BZ_C_SPARSE_AFFINE): what can be checked without a GPU — the
constructor, the numpy eval! / jtprod! (the host outer loop and the generic-oracle protocol use them), the lowering into
the problem descriptor, the refused combinations and the two generators of bz.synth."""
import ctypes as C

import numpy as np
import pytest


def tricky(dtype=np.float64):
    """4 x 5: row 0 unsorted, row 1 empty, row 2 with a duplicated entry, column 3 empty"""
    indptr = np.array([0, 3, 3, 6, 8], np.int64)
    indices = np.array([4, 0, 2, 1, 1, 0, 2, 4], np.int32)
    data = np.array([1.5, -2.0, 0.25, 3.0, -1.0, 0.5, 2.0, -4.0], dtype)
    b = np.array([0.5, -1.0, 2.0, 0.0], dtype)
    A = np.zeros((4, 5), dtype)
    for r in range(4):
        for k in range(indptr[r], indptr[r + 1]):
            A[r, indices[k]] += data[k]
    return indptr, indices, data, b, A


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_eval_and_jtprod_on_empty_rows_columns_unsorted_and_duplicated_entries(bz, dtype):
    indptr, indices, data, b, A = tricky(dtype)
    c = bz.SparseAffine(indptr, indices, data, b, 5)
    assert (c.ny, c.n, c.nnz) == (4, 5, 8)
    assert np.array_equal(c.toarray(), A)
    x = np.array([1.0, -2.0, 3.0, 0.5, -1.5], dtype)
    v = np.array([2.0, -1.0, 0.5, 3.0], dtype)
    cx, jtv = np.empty(4, dtype), np.empty(5, dtype)
    c.eval(cx, x)
    c.jtprod(jtv, x, v)
    assert cx.dtype == dtype and jtv.dtype == dtype
    assert np.array_equal(cx, A @ x - b)            # (small dyadic numbers: every sum is exact)
    assert np.array_equal(jtv, A.T @ v)
    assert cx[1] == -b[1] and jtv[3] == 0           # the empty row and the empty column


def test_from_dense_round_trip(bz):
    rng = np.random.default_rng(0)
    A = rng.standard_normal((7, 11)) * (rng.random((7, 11)) < 0.3)
    A[3] = 0
    A[:, 5] = 0
    b = rng.standard_normal(7)
    c = bz.SparseAffine.from_dense(A, b)
    assert c.nnz == np.count_nonzero(A) and c.indptr.dtype == np.int64 and c.indices.dtype == np.int32
    assert np.array_equal(c.toarray(), A)
    x, v = rng.standard_normal(11), rng.standard_normal(7)
    cx, jtv = np.empty(7), np.empty(11)
    c.eval(cx, x)
    c.jtprod(jtv, x, v)
    assert np.allclose(cx, A @ x - b, rtol=0, atol=1e-14) and np.allclose(jtv, A.T @ v, rtol=0, atol=1e-14)


def test_constructor_errors(bz):
    indptr, indices, data, b, _ = tricky()
    S = bz.SparseAffine
    S(indptr, indices, data, b, 5)
    with pytest.raises(ValueError):
        S(indptr[:-1], indices, data, b, 5)                                   # indptr too short
    with pytest.raises(ValueError):
        S(indptr, indices[:-1], data, b, 5)                                   # indices / data lengths differ
    with pytest.raises(ValueError):
        S(np.array([0, 3, 2, 6, 8]), indices, data, b, 5)                     # decreasing
    with pytest.raises(ValueError):
        S(np.array([0, 3, 3, 6, 7]), indices, data, b, 5)                     # indptr[ny] != nnz
    with pytest.raises(ValueError):
        S(np.array([1, 3, 3, 6, 8]), indices, data, b, 5)                     # indptr[0] != 0
    with pytest.raises(ValueError):
        S(indptr, indices, data, b, 4)                                        # a column = n
    with pytest.raises(ValueError):
        S(indptr, -indices, data, b, 5)                                       # a negative column
    with pytest.raises(ValueError):
        S(indptr.astype(np.float64), indices, data, b, 5)                     # dtypes
    with pytest.raises(ValueError):
        S(indptr, indices, data.astype(np.int64), b, 5)
    with pytest.raises(ValueError):
        S(indptr, indices, data, b, 0)
    with pytest.raises(ValueError):
        S(indptr, indices, data.reshape(2, 4), b, 5)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lower_fills_the_kind_and_the_four_fields(bz, dtype):
    from bazinga_jl_amd.oracles import lower
    L = bz._lib
    indptr, indices, data, b, _ = tricky(np.float64)
    c = bz.SparseAffine(indptr, indices, data, b, 5)
    d, keep = lower(bz.DiagQuadratic(np.ones(5), np.zeros(5)), bz.NormL1(1.0), c, bz.ClosedSet(bz.IndBox(-1.0, 2.0)), 5, 4, dtype)
    assert L.BZ_C_SPARSE_AFFINE == 3 and d.c_kind == L.BZ_C_SPARSE_AFFINE
    assert (d.n, d.ny, d.slack, d.c_sp_nnz) == (5, 4, 0, 8)
    rp = np.ctypeslib.as_array(C.cast(d.c_sp_rowptr, C.POINTER(C.c_int64)), shape=(5,))
    col = np.ctypeslib.as_array(C.cast(d.c_sp_col, C.POINTER(C.c_int32)), shape=(8,))
    ct = C.c_double if dtype == np.float64 else C.c_float
    val = np.ctypeslib.as_array(C.cast(d.c_sp_val, C.POINTER(ct)), shape=(8,))
    bb = np.ctypeslib.as_array(C.cast(d.c_b, C.POINTER(ct)), shape=(4,))
    assert np.array_equal(rp, indptr) and np.array_equal(col, indices)
    assert np.array_equal(val, data.astype(dtype)) and np.array_equal(bb, b.astype(dtype))
    assert not d.c_A
    # the new fields sit behind every older one
    names = [f[0] for f in L.ProblemDesc._fields_]
    assert names[-4:] == ["c_sp_rowptr", "c_sp_col", "c_sp_val", "c_sp_nnz"]
    with pytest.raises(ValueError):
        lower(bz.Zero(), bz.Zero(), c, bz.ZeroSet(), 6, 4, dtype)            # shape mismatch


def test_refused_combinations_raise_before_any_device_call(bz):
    from bazinga_jl_amd.oracles import lower
    indptr, indices, data, b, _ = tricky()
    c = bz.SparseAffine(indptr, indices, data, b, 5)
    U = bz.UnsupportedOracle
    with pytest.raises(U):
        lower(bz.Zero(), bz.NormL1(1.0), c, bz.ZeroSet(), 5, 4, np.float64, slack=True)
    with pytest.raises(U):
        lower(bz.Zero(), bz.NormL1(1.0), c, bz.ComplementarityPairs(), 5, 4, np.float64)
    with pytest.raises(U):
        lower(bz.LeastSquares(np.ones((3, 5)), np.ones(3)), bz.NormL1(1.0), c, bz.ZeroSet(), 5, 4, np.float64)
    with pytest.raises(U):
        lower(bz.Quadratic(np.eye(5), np.ones(5)), bz.NormL1(1.0), c, bz.ZeroSet(), 5, 4, np.float64)
    # ... and through the public entry points: UnsupportedOracle, not the error of a missing device
    with pytest.raises(U):
        bz.Problem(bz.Zero(), bz.NormL1(1.0), c, bz.ZeroSet(), 5, 4, np.float64, slack=True)
    with pytest.raises(U):
        bz.als(bz.Zero(), bz.NormL1(1.0), c, bz.ZeroSet(), np.zeros(5), np.zeros(4))
    with pytest.raises(U):
        bz.alps(bz.Zero(), bz.NormL1(1.0), c, bz.XorPairs(), np.zeros(5), np.zeros(4))


def test_host_outer_loop_evaluates_a_sparse_c(bz):
    from bazinga_jl_amd.solvers import _eval_c_host
    indptr, indices, data, b, A = tricky()
    c = bz.SparseAffine(indptr, indices, data, b, 5)
    x = np.arange(5.0)
    assert np.array_equal(_eval_c_host(c, x, 4), A @ x - b)
    assert np.array_equal(_eval_c_host(c, x), A @ x - b)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_synth_obstacle_1d(bz, dtype):
    N = 7
    d = bz.synth.obstacle_1d(N, dtype)
    c = bz.SparseAffine(d["indptr"], d["indices"], d["data"], d["b"], d["n"])
    T = 2 * np.eye(N) - np.eye(N, k=1) - np.eye(N, k=-1)
    assert (c.ny, c.n) == (N, 3 * N) and d["data"].dtype == dtype
    assert np.array_equal(c.toarray(), np.hstack([np.eye(N), T, -np.eye(N)]).astype(dtype))
    assert c.nnz == 5 * N - 2 and np.max(np.diff(c.indptr)) == 5
    assert d["q"].shape == (3 * N,) and np.all(d["q"] > 0)


def test_synth_budget_bands(bz):
    n, m = 40, 9
    d = bz.synth.budget_bands(n, m)
    c = bz.SparseAffine(d["indptr"], d["indices"], d["data"], d["b"], n)
    A = c.toarray()
    assert A.shape == (m + 1, n) and np.array_equal(A[0], np.ones(n))                 # the budget row
    assert np.all(np.count_nonzero(A[1:], axis=1) == 4) and np.all(A[1:, n - 1] != 0)  # band rows + the shared column
    for k in range(1, m + 1):
        nz = np.nonzero(A[k, :n - 1])[0]
        assert nz[-1] - nz[0] == 2
    # consistent: xfeas satisfies g = IndBox(0, 1) and c(xfeas) in D
    cx = np.empty(m + 1)
    c.eval(cx, d["xfeas"])
    assert np.all(d["xfeas"] >= 0) and np.all(d["xfeas"] <= 1) and abs(cx[0]) <= 1e-12
    assert np.all(cx[1:] >= d["lo"][1:]) and np.all(cx[1:] <= d["hi"][1:]) and d["lo"][0] == d["hi"][0] == 0
    assert np.array_equal(bz.synth.budget_bands(n, m)["data"], d["data"])             # seeded: the same bits every call
