"""Multinomial (softmax) regression on a sparse A in CSR (bz.SparseMultinomial, BZ_F_SPARSE_MULTINOMIAL), everything that needs no
GPU: the class's validation and host mirrors, its numpy value and gradient, its lowering to the C descriptor (the new field
f_classes directly behind f_rows) and the generator bz.synth.sparse_multinomial."""
import ctypes as C

import numpy as np
import pytest

from bazinga_jl_amd.oracles import lower
from tests.test_gpu_sparse import csr_of, structured


def small():
    """3 x 4, five entries, labels of K = 3"""
    indptr, indices, data = np.array([0, 2, 3, 5]), np.array([0, 3, 1, 2, 3]), np.arange(1.0, 6.0)
    return indptr, indices, data, np.array([2.0, 0.0, 1.0]), 4, 3


def test_validation_errors(bz):
    indptr, indices, data, lab, nf, K = small()
    f = bz.SparseMultinomial(indptr, indices, data, lab, nf, K)
    assert (f.nnz, f.n_features, f.n_classes, f.n, f.m, f.scale, f.weights) == (5, 4, 3, 12, 3, 1.0, None)
    for bad in (1, 0, 65, -3):
        with pytest.raises(ValueError, match="n_classes"):
            bz.SparseMultinomial(indptr, indices, data, np.zeros(3), nf, bad)
    assert bz.SparseMultinomial(indptr, indices, data, np.array([63, 0, 1]), nf, 64).b.dtype == np.float64
    # the matrix checks of SparseLeastSquares, with n_features columns
    with pytest.raises(ValueError, match="indptr"):
        bz.SparseMultinomial(np.array([0, 3, 2, 5]), indices, data, lab, nf, K)
    with pytest.raises(ValueError, match="indptr"):
        bz.SparseMultinomial(np.array([0, 2, 5]), indices, data, lab, nf, K)
    with pytest.raises(ValueError, match="column indices"):
        bz.SparseMultinomial(indptr, np.array([0, 3, 1, 4, 3]), data, lab, nf, K)
    with pytest.raises(ValueError, match="same length"):
        bz.SparseMultinomial(indptr, indices, data[:4], lab, nf, K)
    with pytest.raises(ValueError, match="integer"):
        bz.SparseMultinomial(indptr.astype(np.float64), indices, data, lab, nf, K)
    with pytest.raises(ValueError, match="float64 or float32"):
        bz.SparseMultinomial(indptr, indices, data.astype(np.int64), lab, nf, K)
    with pytest.raises(ValueError, match="2\\^31"):
        bz.SparseMultinomial(indptr, indices, data, lab, 2 ** 30, K)                  # n_features * K is beyond 2^31 - 1
    # labels: finite, integral, in [0, K)
    for bad in (np.array([0.0, 3.0, 1.0]), np.array([0.0, -1.0, 1.0]), np.array([0.5, 0.0, 1.0]), np.array([0.0, np.nan, 1.0]),
                np.array([0.0, np.inf, 1.0]), np.array([0, 1, 3])):
        with pytest.raises(ValueError, match="labels"):
            bz.SparseMultinomial(indptr, indices, data, bad, nf, K)
    with pytest.raises(ValueError, match="one-dimensional"):
        bz.SparseMultinomial(indptr, indices, data, np.zeros((3, 1)), nf, K)
    # weights, scale: SparseGLM's rules
    for bad in (np.array([1.0, -0.5, 1.0]), np.array([1.0, np.nan, 1.0]), np.array([1.0, np.inf, 1.0]), np.ones(2), np.ones((3, 1))):
        with pytest.raises(ValueError, match="weights"):
            bz.SparseMultinomial(indptr, indices, data, lab, nf, K, weights=bad)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="scale"):
            bz.SparseMultinomial(indptr, indices, data, lab, nf, K, scale=bad)
    w = np.array([1.0 / 3.0, 0.1, 7.0])
    h = bz.SparseMultinomial(indptr, indices, data, lab, nf, K, weights=w, scale=1.0 / 3.0)
    assert np.array_equal(h.row_weights(np.float32), ((1.0 / 3.0) * w).astype(np.float32))          # one rounding
    assert type(f.row_weights(np.float32)) is np.float32 and f.row_weights(np.float32) == 1
    # coef: the (n_features, K) view of the flat variable, class fastest
    x = np.arange(12.0)
    assert f.coef(x).shape == (4, 3) and f.coef(x)[2, 1] == x[2 * 3 + 1] and np.shares_memory(f.coef(x), x)


def test_from_dense_round_trip(bz):
    for m, nf, p in ((120, 40, 0.02), (3, 70, 0.5), (41, 121, 0.1)):
        A = structured(m, nf, p, np.random.default_rng(m + nf), False, np.float64)
        f = bz.SparseMultinomial.from_dense(A, np.zeros(m), 5, weights=np.ones(m), scale=1.0 / m)
        assert np.array_equal(f.toarray(), A) and f.nnz == np.count_nonzero(A) and (f.m, f.n_features, f.n) == (m, nf, 5 * nf)
        assert f.indptr.dtype == np.int64 and f.indices.dtype == np.int32 and f.scale == 1.0 / m


def dense_value(A, lab, X, w):
    """sum_i w_i (logsumexp(t_i) - t_{i,b_i}) in float64, written independently of the class"""
    t = A.astype(np.float64) @ X.astype(np.float64)
    return float(np.sum(w * (np.logaddexp.reduce(t, axis=1) - t[np.arange(t.shape[0]), lab])))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", [2, 3, 5])
def test_numpy_gradient_against_central_differences(bz, K, weighted):
    """the class's gradient against central differences of the class's own value, element by element (h = 1e-5: the
    truncation error h^2 f''' / 6 and the rounding error eps f / h both stay below 1e-7 of the gradient's largest entry),
    and the value against the dense float64 formula; unsorted rows and a duplicated entry included"""
    rng = np.random.default_rng(5 + K)
    m, nf = 17, 9
    A = structured(m, nf, 0.4, rng, False, np.float64)
    indptr, indices, data = csr_of(A, np.random.default_rng(1))
    k = indptr[2]                                             # duplicate the first entry of row 2: 2 a = a + a
    indices, data = np.insert(indices, k, indices[k]), np.insert(data, k, data[k])
    indptr[3:] += 1
    A[2, indices[k]] *= 2
    lab = rng.integers(0, K, m)
    w = rng.uniform(0.0, 2.0, m) if weighted else None
    scale = 1.0 / m if weighted else 1.0
    f = bz.SparseMultinomial(indptr, indices, data, lab, nf, K, weights=w, scale=scale)
    assert np.array_equal(f.toarray(), A)
    x = rng.standard_normal(nf * K)
    g = np.empty(nf * K)
    fx = f.gradient(g, x)
    assert type(fx) is np.float64 and fx == f(x)
    w64 = f.row_weights(np.float64) * np.ones(m)
    ref_value = dense_value(A, lab, f.coef(x), w64)
    assert abs(fx - ref_value) <= 1e-13 * max(1.0, abs(ref_value))
    h = 1e-5
    fd = np.empty_like(g)
    for i in range(x.shape[0]):
        e = np.zeros_like(x)
        e[i] = h
        fd[i] = (f(x + e) - f(x - e)) / (2 * h)
    assert np.max(np.abs(fd - g)) <= 1e-7 * np.max(np.abs(g)), np.max(np.abs(fd - g)) / np.max(np.abs(g))
    # every row of R sums to zero: the gradient's K classes of a feature sum to (almost) nothing
    assert np.max(np.abs(f.coef(g).sum(axis=1))) <= 1e-14 * np.max(np.abs(g)) * K * m
    # float32 runs in float32
    x32, g32 = x.astype(np.float32), np.empty(nf * K, np.float32)
    f32 = f.gradient(g32, x32)
    assert type(f32) is np.float32 and abs(float(f32) - fx) <= 1e-5 * max(1.0, abs(fx)) and np.max(np.abs(g32 - g)) <= 1e-5 * np.max(np.abs(g))


def test_numpy_edge_values(bz):
    """an empty row: loss w log K and p = 1 / K; a NaN in one class of one row reaches that row's K entries of R and the
    value, and no other row; t = +inf gives NaN (inf - inf)"""
    K, nf = 3, 2
    f = bz.SparseMultinomial(np.array([0, 1, 1, 2]), np.array([0, 1]), np.array([1.0, 1.0]), np.array([0, 1, 2]), nf, K)
    x = np.array([1.0, 2.0, 3.0, 0.0, 0.0, 0.0])
    loss, R = f._loss_r(x)
    assert loss[1] == np.log(3.0) and np.array_equal(R[1], [1.0 / 3, 1.0 / 3 - 1, 1.0 / 3])
    x[1] = np.nan
    loss, R = f._loss_r(x)
    assert np.isnan(loss[0]) and np.all(np.isnan(R[0])) and np.all(np.isfinite(R[1:])) and np.all(np.isfinite(loss[1:]))
    x[1] = np.inf
    loss, R = f._loss_r(x)
    assert np.isnan(loss[0]) and np.isnan(R[0, 1])
    x[:3] = [0.0, -1e4, -1e4]                                       # very negative in all but one class: exactly one-hot
    loss, R = f._loss_r(x)
    assert np.array_equal(R[0], [0.0, 0.0, 0.0]) and loss[0] == 0.0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lower_fills_the_descriptor(bz, dtype):
    L = bz._lib
    indptr, indices, data, lab, nf, K = small()
    m, n, ny = 3, nf * K, 2
    ct = C.c_double if dtype == np.float64 else C.c_float
    A = np.zeros((ny, n), dtype)
    A[0, :] = 1
    A[1, 3] = 2
    cs = bz.SparseAffine.from_dense(A, np.zeros(ny, dtype))
    w = np.array([0.5, 0.0, 2.0])
    for weights, scale in ((None, 1.0), (w, 1.0 / m)):
        f = bz.SparseMultinomial(indptr, indices, data.astype(dtype), lab, nf, K, weights=weights, scale=scale)
        for c, rows in ((bz.IdentityFunction(), n), (cs, ny)):
            desc, keep = lower(f, bz.NormL1(0.1), c, bz.ZeroSet(), n, rows, dtype)
            assert desc.f_kind == L.BZ_F_SPARSE_MULTINOMIAL == 10 and desc.f_classes == K and desc.f_rows == m
            assert desc.n == n and desc.f_sp_nnz == f.nnz == 5 and desc.f_scale == scale
            assert desc.c_kind == (L.BZ_C_SPARSE_AFFINE if c is cs else L.BZ_C_IDENTITY)
            rp = np.ctypeslib.as_array(C.cast(desc.f_sp_rowptr, C.POINTER(C.c_int64)), shape=(m + 1,))
            col = np.ctypeslib.as_array(C.cast(desc.f_sp_col, C.POINTER(C.c_int32)), shape=(f.nnz,))
            val = np.ctypeslib.as_array(C.cast(desc.f_sp_val, C.POINTER(ct)), shape=(f.nnz,))
            bb = np.ctypeslib.as_array(C.cast(desc.f_b, C.POINTER(ct)), shape=(m,))
            assert np.array_equal(rp, f.indptr) and np.array_equal(col, f.indices) and np.array_equal(val, f.data)
            assert np.array_equal(bb, lab) and bb.dtype == dtype and not desc.f_A and not desc.f_q
            if weights is None:
                assert not desc.f_w
            else:                                           # the weights as given: the library folds the scale in
                ww = np.ctypeslib.as_array(C.cast(desc.f_w, C.POINTER(ct)), shape=(m,))
                assert np.array_equal(ww, w.astype(dtype))
    # the other kinds leave f_classes zero
    pm = np.array([1.0, -1.0, 1.0])
    for other in (bz.SparseLogistic(indptr, indices, data, pm, nf), bz.SparseLeastSquares(indptr, indices, data, pm, nf),
                  bz.SparseGLM(indptr, indices, data, pm, nf, "squared_hinge"), bz.DiagQuadratic(np.ones(nf), np.ones(nf))):
        desc, keep = lower(other, bz.NormL1(0.1), bz.IdentityFunction(), bz.ZeroSet(), nf, nf, dtype)
        assert desc.f_classes == 0
    # the field sits directly behind f_rows; the pinned neighbourhoods are where they were
    names = [nm for nm, _ in L.ProblemDesc._fields_]
    assert names[names.index("f_rows") + 1] == "f_classes" and names[names.index("f_classes") + 1] == "g_lambda"
    assert L.ProblemDesc.f_classes.offset == L.ProblemDesc.f_rows.offset + 8 and L.ProblemDesc.f_classes.size == 8
    assert names[-8:-4] == ["f_loss", "f_loss_delta", "f_w", "f_scale"] and names[-9] == "f_sp_nnz"
    assert names[names.index("g_lambda_vec") - 1] == "g_hi_vec" and names[names.index("g_lambda_vec") + 1] == "c_A"


def test_lower_refuses_or_reroutes_before_any_device_call(bz):
    """what lower() itself can see: it raises for the slack form and for a dense c, for a variable that is not n_features * K
    long and for numbers that are not finite in float32; a mix with an oracle that is not lowered goes through the callback
    kinds, all four together, so the library never sees kind 10 beside a callback"""
    indptr, indices, data, lab, nf, K = small()
    n = nf * K
    f = bz.SparseMultinomial(indptr, indices, data, lab, nf, K)
    for kw in ({"scale": 1e300}, {"weights": np.array([1.0, 1e30, 1.0]), "scale": 1e30}):
        big = bz.SparseMultinomial(indptr, indices, data, lab, nf, K, **kw)
        lower(big, bz.NormL1(0.1), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64)
        with pytest.raises(ValueError, match="finite in float32"):
            lower(big, bz.NormL1(0.1), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float32)
    A = np.ones((2, n))
    with pytest.raises(bz.UnsupportedOracle, match="SparseMultinomial.*slack"):
        lower(f, bz.NormL1(0.1), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64, slack=True)
    with pytest.raises(bz.UnsupportedOracle, match="SparseMultinomial.*DenseAffine"):
        lower(f, bz.NormL1(0.1), bz.DenseAffine(A, np.zeros(2)), bz.ZeroSet(), n, 2, np.float64)
    with pytest.raises(bz.UnsupportedOracle, match="pairwise"):
        cs = bz.SparseAffine.from_dense(A, np.zeros(2))
        lower(f, bz.NormL1(0.1), cs, bz.XorPairs(), n, 2, np.float64)
    for bad_n in (nf, n + 1, n + K):
        with pytest.raises(ValueError, match="n_features \\* n_classes"):
            lower(f, bz.NormL1(0.1), bz.IdentityFunction(), bz.ZeroSet(), bad_n, bad_n, np.float64)
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(f, bz.NormL1(1.0), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64, slack=True)
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(f, bz.NormL1(1.0), bz.DenseAffine(A, np.zeros(2)), bz.ZeroSet(), n, 2, np.float64)

    class MyL1:
        def prox(self, z, x, gamma):
            z[...] = x
            return 0.0
    desc, keep = lower(f, MyL1(), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64)
    assert (desc.f_kind, desc.g_kind, desc.c_kind, desc.D_kind) == (bz._lib.BZ_F_CALLBACK, bz._lib.BZ_G_CALLBACK,
                                                                    bz._lib.BZ_C_CALLBACK, bz._lib.BZ_D_CALLBACK)
    # ... and the callback the library would call is the class's numpy gradient
    x = np.linspace(-1.0, 1.0, n)
    out = np.empty(n)
    fx = desc.cb_f_gradient(None, x.ctypes.data, out.ctypes.data, n)
    g = np.empty(n)
    assert fx == float(f.gradient(g, x)) and np.array_equal(out, g)


def test_sparse_multinomial_is_reproducible(bz):
    m, nf, K, k = 256, 16, 4, 5
    las = bz.synth.sparse_lasso(m, nf, k)
    a, b = bz.synth.sparse_multinomial(m, nf, K, k), bz.synth.sparse_multinomial(m, nf, K, k)
    assert all(np.array_equal(a[key], b[key]) for key in ("indptr", "indices", "data", "labels", "xstar"))
    assert not np.array_equal(a["data"], bz.synth.sparse_multinomial(m, nf, K, k, seed=7)["data"])
    assert all(np.array_equal(a[key], las[key]) for key in ("indptr", "indices", "data"))           # sparse_lasso's matrix
    assert (a["m"], a["n_f"], a["K"], a["n"]) == (m, nf, K, nf * K) and a["xstar"].shape == (nf * K,) and a["labels"].dtype == np.float64
    c = bz.synth.sparse_multinomial(m, nf, K, k, np.float32)
    assert c["data"].dtype == c["labels"].dtype == np.float32 and np.array_equal(c["indices"], a["indices"])
    f = bz.SparseMultinomial(a["indptr"], a["indices"], a["data"], a["labels"], nf, K)               # the data pass the validation
    # every class occurs, and the planted X* explains the labels better than X = 0 does
    assert set(np.unique(a["labels"])) == set(range(K))
    assert abs(f(np.zeros(nf * K)) - m * np.log(K)) < 1e-9 and f(a["xstar"]) < f(np.zeros(nf * K))
    assert np.count_nonzero(f.coef(a["xstar"]).any(axis=1)) == max(1, nf // 20)
    with pytest.raises(ValueError):
        bz.synth.sparse_multinomial(4, 3, 3, 5)
    with pytest.raises(ValueError):
        bz.synth.sparse_multinomial(4, 8, 1)
    with pytest.raises(ValueError):
        bz.synth.sparse_multinomial(4, 8, 65)
