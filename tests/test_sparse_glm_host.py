"""f(x) = sum_i w_i l(b_i, a_i'x) with a sparse A in CSR (bz.SparseGLM, BZ_F_SPARSE_GLM), everything that needs no GPU: the
class's validation and host mirrors, the formulas of the five losses at their edges, its lowering to the C descriptor and
the generator bz.synth.sparse_glm."""
import ctypes as C

import numpy as np
import pytest

from bazinga_jl_amd.oracles import lower
from tests.test_gpu_sparse import CASES64, csr_of, structured

LOSSES = ("least_squares", "logistic", "huber", "squared_hinge", "poisson")


def small():
    indptr, indices, data = np.array([0, 2, 3, 5]), np.array([0, 3, 1, 2, 3]), np.arange(1.0, 6.0)
    return indptr, indices, data, np.array([1.0, -1.0, 1.0]), 4


def b_of(loss, rng, m, dtype):
    if loss in ("logistic", "squared_hinge"):
        return np.where(rng.random(m) < 0.5, -1.0, 1.0).astype(dtype)
    if loss == "poisson":
        return rng.integers(0, 6, m).astype(dtype)
    return rng.standard_normal(m).astype(dtype)


def dense_glm(A, b, x, loss, delta, w):
    """the dense formula in float64, written independently of the class: (sum_i w_i l_i, A'(w l'))"""
    A, b, x, w = (np.asarray(v, np.float64) for v in (A, b, x, w))
    t = A @ x
    if loss == "least_squares":
        l, dl = 0.5 * (t - b) ** 2, t - b
    elif loss == "logistic":
        l, dl = np.logaddexp(0.0, -b * t), -b / (1.0 + np.exp(b * t))
    elif loss == "huber":
        v = t - b
        l = np.where(np.abs(v) <= delta, 0.5 * v * v, delta * (np.abs(v) - 0.5 * delta))
        dl = np.clip(v, -delta, delta)
    elif loss == "squared_hinge":
        h = np.maximum(0.0, 1.0 - b * t)
        l, dl = 0.5 * h * h, -b * h
    else:
        l, dl = np.exp(t) - b * t, np.exp(t) - b
    return float(np.sum(w * l)), A.T @ (w * dl)


def test_validation_errors(bz):
    indptr, indices, data, b, n = small()
    f = bz.SparseGLM(indptr, indices, data, b, n, "huber", delta=1.5)
    assert f.nnz == 5 and f.n == 4 and f.m == 3 and f.delta == 1.5 and f.scale == 1.0 and f.weights is None
    with pytest.raises(ValueError, match="unknown loss"):
        bz.SparseGLM(indptr, indices, data, b, n, "hinge")
    # the matrix checks of SparseLeastSquares
    with pytest.raises(ValueError, match="indptr"):
        bz.SparseGLM(np.array([0, 3, 2, 5]), indices, data, b, n, "least_squares")
    with pytest.raises(ValueError, match="indptr"):
        bz.SparseGLM(np.array([0, 2, 5]), indices, data, b, n, "least_squares")
    with pytest.raises(ValueError, match="column indices"):
        bz.SparseGLM(indptr, np.array([0, 3, 1, 4, 3]), data, b, n, "least_squares")
    with pytest.raises(ValueError, match="same length"):
        bz.SparseGLM(indptr, indices, data[:4], b, n, "least_squares")
    with pytest.raises(ValueError, match="integer"):
        bz.SparseGLM(indptr.astype(np.float64), indices, data, b, n, "least_squares")
    with pytest.raises(ValueError, match="float64 or float32"):
        bz.SparseGLM(indptr, indices, data.astype(np.int64), b, n, "least_squares")
    with pytest.raises(ValueError, match="2\\^31"):
        bz.SparseGLM(indptr, indices, data, b, 2 ** 31, "least_squares")
    # labels, counts
    for loss in ("logistic", "squared_hinge"):
        for bad in (np.array([1.0, 0.0, 1.0]), np.array([1.0, -1.0, 2.0]), np.array([1.0, np.nan, -1.0])):
            with pytest.raises(ValueError, match="labels"):
                bz.SparseGLM(indptr, indices, data, bad, n, loss)
    for bad in (np.array([1.0, -1.0, 2.0]), np.array([1.0, np.nan, 0.0]), np.array([1.0, np.inf, 0.0])):
        with pytest.raises(ValueError, match="counts"):
            bz.SparseGLM(indptr, indices, data, bad, n, "poisson")
    assert bz.SparseGLM(indptr, indices, data, np.array([0, 3, 1]), n, "poisson").b.dtype == np.float64
    # delta
    for bad in (None, 0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="delta"):
            bz.SparseGLM(indptr, indices, data, b, n, "huber", delta=bad)
    for loss in ("least_squares", "logistic", "squared_hinge", "poisson"):
        with pytest.raises(ValueError, match="delta"):
            bz.SparseGLM(indptr, indices, data, np.ones(3), n, loss, delta=1.0)
    # weights, scale
    for bad in (np.array([1.0, -0.5, 1.0]), np.array([1.0, np.nan, 1.0]), np.array([1.0, np.inf, 1.0]), np.ones(2), np.ones((3, 1))):
        with pytest.raises(ValueError, match="weights"):
            bz.SparseGLM(indptr, indices, data, b, n, "least_squares", weights=bad)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="scale"):
            bz.SparseGLM(indptr, indices, data, b, n, "least_squares", scale=bad)
    g = bz.SparseGLM(indptr, indices, data.astype(np.float32), b, n, "least_squares", weights=np.array([1, 0, 2]), scale=0.5)
    assert g.weights.dtype == np.float32 and np.array_equal(g.row_weights(np.float32), np.array([0.5, 0.0, 1.0], np.float32))
    # the product scale * w is taken in float64 and rounded once
    w = np.array([1.0 / 3.0, 0.1, 7.0])
    h = bz.SparseGLM(indptr, indices, data, b, n, "least_squares", weights=w, scale=1.0 / 3.0)
    assert np.array_equal(h.row_weights(np.float32), ((1.0 / 3.0) * w).astype(np.float32))
    assert type(f.row_weights(np.float32)) is np.float32 and f.row_weights(np.float32) == 1


def test_from_dense_round_trip(bz):
    for m, n, p in CASES64[:5]:
        A = structured(m, n, p, np.random.default_rng(m + n), False, np.float64)
        f = bz.SparseGLM.from_dense(A, np.ones(m), "squared_hinge", weights=np.ones(m), scale=1.0 / m)
        assert np.array_equal(f.toarray(), A) and f.nnz == np.count_nonzero(A) and (f.m, f.n) == (m, n)
        assert f.indptr.dtype == np.int64 and f.indices.dtype == np.int32 and f.scale == 1.0 / m


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_value_and_gradient_against_the_dense_formula(bz, dtype, loss, weighted):
    """real data, unsorted rows and a duplicated entry included: within a few roundings of the dtype of the dense float64
    formula (the gradient relative to its largest entry)"""
    rng = np.random.default_rng(11)
    m, n = 41, 121
    A = structured(m, n, 0.1, rng, False, dtype)
    indptr, indices, data = csr_of(A, np.random.default_rng(1))
    k = indptr[2]                                             # duplicate the first entry of row 2: 2 a = a + a
    indices, data = np.insert(indices, k, indices[k]), np.insert(data, k, data[k])
    indptr[3:] += 1
    A[2, indices[k]] *= 2
    b = b_of(loss, rng, m, dtype)
    delta = 0.75 if loss == "huber" else None
    w = rng.uniform(0.0, 2.0, m).astype(dtype) if weighted else None
    if weighted:
        w[::7] = 0
    scale = 1.0 / m if weighted else 1.0
    f = bz.SparseGLM(indptr, indices, data, b, n, loss, delta=delta, weights=w, scale=scale)
    assert np.array_equal(f.toarray(), A)
    w64 = f.row_weights(dtype).astype(np.float64) * np.ones(m)
    tol = 64 * float(np.finfo(dtype).eps)
    for xs in (1.0, 3.0):
        x = (xs * rng.standard_normal(n)).astype(dtype)
        g = np.empty(n, dtype)
        fx = f.gradient(g, x)
        f_ref, g_ref = dense_glm(A, b, x, loss, delta, w64)
        assert g.dtype == dtype and type(fx) is dtype and fx == f(x)
        assert abs(float(fx) - f_ref) <= tol * max(1.0, abs(f_ref))
        assert np.max(np.abs(g - g_ref)) <= tol * np.max(np.abs(g_ref))


def loss_dl(bz, loss, b, t, delta=None):
    dtype = t.dtype
    l, dl = bz.SparseGLM.loss_and_derivative(loss, delta, np.asarray(b, dtype), t)
    assert l.dtype == dl.dtype == dtype
    return l, dl


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_formulas_at_their_edges(bz, dtype):
    inf, nan = np.inf, np.nan
    # Huber, delta = 2, b = 1: v = +-delta exactly is inside; beyond: linear; +-inf: +inf and +-delta; NaN reaches both
    t = np.array([3.0, -1.0, 3.5, -1.5, 1.0, inf, -inf, nan], dtype)
    l, dl = loss_dl(bz, "huber", np.ones(8), t, 2.0)
    assert np.array_equal(l[:7], np.array([2.0, 2.0, 3.0, 3.0, 0.0, inf, inf], dtype))
    assert np.array_equal(dl[:7], np.array([2.0, -2.0, 2.0, -2.0, 0.0, 2.0, -2.0], dtype))
    assert np.isnan(l[7]) and np.isnan(dl[7])
    # squared hinge, b = (1, -1, ...): u = 1 and u = +inf give 0 and 0; u = -inf gives +inf and -b inf; NaN reaches both
    b = np.array([1.0, -1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 1.0], dtype)
    t = np.array([1.0, -1.0, 0.0, inf, inf, -inf, -3.0, nan], dtype)
    l, dl = loss_dl(bz, "squared_hinge", b, t)
    assert np.array_equal(l[:7], np.array([0.0, 0.0, 0.5, 0.0, inf, inf, 0.0], dtype))
    assert np.array_equal(dl[:7], np.array([0.0, 0.0, -1.0, 0.0, inf, -inf, 0.0], dtype))
    assert np.isnan(l[7]) and np.isnan(dl[7])
    # Poisson: t = 100 overflows exp in fp32 alone: +inf there, never inf - inf; b = 0 at t = -inf gives 0, b > 0 gives +inf
    b = np.array([3.0, 0.0, 0.0, 2.0, 2.0, 0.0, 1.0], dtype)
    t = np.array([100.0, 100.0, -inf, -inf, 0.0, 0.0, nan], dtype)
    l, dl = loss_dl(bz, "poisson", b, t)
    with np.errstate(over="ignore"):
        e100 = np.exp(dtype(100.0))
    if dtype == np.float32:
        assert e100 == inf and l[0] == inf and l[1] == inf and dl[0] == inf
    else:
        assert l[0] == e100 - dtype(300.0) and l[1] == e100 and dl[0] == e100 - 3
    assert np.array_equal(l[2:6], np.array([0.0, inf, 1.0, 1.0], dtype))
    assert np.array_equal(dl[2:6], np.array([0.0, -2.0, -1.0, 1.0], dtype))
    assert np.isnan(l[6]) and np.isnan(dl[6])
    # least squares and logistic: SparseLeastSquares' and SparseLogistic's numbers on the same matrix, bit for bit (the fp32
    # host mirror of SparseLeastSquares subtracts b before it rounds A x to fp32, the device and this class after: within
    # a few roundings there)
    rng = np.random.default_rng(3)
    A = structured(41, 121, 0.1, rng, False, dtype)
    indptr, indices, data = csr_of(A, np.random.default_rng(1))
    x = rng.standard_normal(121).astype(dtype)
    for loss, old, bb in (("least_squares", bz.SparseLeastSquares, rng.standard_normal(41).astype(dtype)),
                          ("logistic", bz.SparseLogistic, b_of("logistic", rng, 41, dtype))):
        g0, g1, g2 = np.empty(121, dtype), np.empty(121, dtype), np.empty(121, dtype)
        f0 = old(indptr, indices, data, bb, 121).gradient(g0, x)
        f1 = bz.SparseGLM(indptr, indices, data, bb, 121, loss).gradient(g1, x)
        f2 = bz.SparseGLM(indptr, indices, data, bb, 121, loss, weights=np.ones(41, dtype)).gradient(g2, x)
        assert np.array_equal(g1, g2)
        if loss == "logistic" or dtype == np.float64:
            assert np.array_equal(g0, g1)
        else:
            assert np.max(np.abs(g0 - g1)) <= 8 * float(np.finfo(dtype).eps) * np.max(np.abs(g0))
        assert f1 == f2 and abs(float(f0) - float(f1)) <= 8 * float(np.finfo(dtype).eps) * abs(float(f0))
    # an empty row has t = 0: nnz = 0 gives the loss at 0 times the sum of the weights, and a zero gradient
    w = np.array([0.5, 0.0, 2.0], dtype)
    for loss, bb, at0 in (("huber", [1.0, -1.0, 3.0], [0.5, 0.5, 4.0]), ("squared_hinge", [1.0, -1.0, 1.0], [0.5, 0.5, 0.5]),
                          ("poisson", [0.0, 2.0, 5.0], [1.0, 1.0, 1.0])):
        e = bz.SparseGLM(np.zeros(4, np.int64), np.zeros(0, np.int32), np.zeros(0, dtype), np.array(bb, dtype), 4, loss,
                         delta=2.0 if loss == "huber" else None, weights=w)
        dfx = np.ones(4, dtype)
        assert e.gradient(dfx, np.ones(4, dtype)) == dtype(np.dot(w, np.array(at0, dtype))) and not np.any(dfx)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lower_fills_the_descriptor(bz, dtype):
    L = bz._lib
    indptr, indices, data, _, n = small()
    m, ny = 3, 2
    ct = C.c_double if dtype == np.float64 else C.c_float
    A = np.zeros((ny, n), dtype)
    A[0, :] = 1
    A[1, 3] = 2
    cs = bz.SparseAffine.from_dense(A, np.zeros(ny, dtype))
    w = np.array([0.5, 0.0, 2.0])
    for code, (loss, b) in enumerate(zip(LOSSES, ([1.0, 2.0, 3.0], [1.0, -1.0, 1.0], [1.0, 2.0, 3.0], [1.0, -1.0, 1.0], [0.0, 2.0, 5.0]))):
        b = np.array(b, dtype)
        delta = 1.5 if loss == "huber" else None
        for weights, scale in ((None, 1.0), (w, 1.0 / m)):
            f = bz.SparseGLM(indptr, indices, data.astype(dtype), b, n, loss, delta=delta, weights=weights, scale=scale)
            for c, rows in ((bz.IdentityFunction(), n), (cs, ny)):
                desc, keep = lower(f, bz.NormL1(0.1), c, bz.ZeroSet(), n, rows, dtype)
                assert desc.f_kind == L.BZ_F_SPARSE_GLM == 9 and desc.f_sp_nnz == f.nnz == 5 and desc.f_rows == m
                assert desc.f_loss == code == getattr(L, "BZ_LOSS_" + loss.upper())
                assert desc.f_loss_delta == (1.5 if loss == "huber" else 0.0) and desc.f_scale == scale
                assert desc.c_kind == (L.BZ_C_SPARSE_AFFINE if c is cs else L.BZ_C_IDENTITY)
                rp = np.ctypeslib.as_array(C.cast(desc.f_sp_rowptr, C.POINTER(C.c_int64)), shape=(m + 1,))
                col = np.ctypeslib.as_array(C.cast(desc.f_sp_col, C.POINTER(C.c_int32)), shape=(f.nnz,))
                val = np.ctypeslib.as_array(C.cast(desc.f_sp_val, C.POINTER(ct)), shape=(f.nnz,))
                bb = np.ctypeslib.as_array(C.cast(desc.f_b, C.POINTER(ct)), shape=(m,))
                assert np.array_equal(rp, f.indptr) and np.array_equal(col, f.indices) and np.array_equal(val, f.data)
                assert np.array_equal(bb, b) and not desc.f_A and not desc.f_q
                if weights is None:
                    assert not desc.f_w
                else:                                           # the weights as given: the library folds the scale in
                    ww = np.ctypeslib.as_array(C.cast(desc.f_w, C.POINTER(ct)), shape=(m,))
                    assert np.array_equal(ww, w.astype(dtype))
    # the other kinds leave the new fields zero
    desc, keep = lower(bz.SparseLogistic(indptr, indices, data, np.ones(3), n), bz.NormL1(0.1), bz.IdentityFunction(), bz.ZeroSet(),
                       n, n, dtype)
    assert (desc.f_loss, desc.f_loss_delta, desc.f_w, desc.f_scale) == (0, 0.0, None, 0.0)
    names = [nm for nm, _ in L.ProblemDesc._fields_]
    assert names[-8:-4] == ["f_loss", "f_loss_delta", "f_w", "f_scale"] and names[-9] == "f_sp_nnz"


def test_lower_refuses_or_reroutes_before_any_device_call(bz):
    """what lower() itself can see: it raises for the slack form and for a dense c, and sends a mix with an oracle that is not
    lowered through the callback kinds, all four together, so the library never sees kind 9 beside a callback.  More than one
    rank is a property of the context, which lower() does not get: bz_problem_create refuses it (tests/test_gpu_sparse_glm.py)."""
    indptr, indices, data, b, n = small()
    f = bz.SparseGLM(indptr, indices, data, b, n, "squared_hinge")
    # numbers that are finite in float64 and not in the float32 problem they are lowered to
    for kw in ({"scale": 1e300}, {"weights": np.array([1.0, 1e30, 1.0]), "scale": 1e30}):
        big = bz.SparseGLM(indptr, indices, data, b, n, "squared_hinge", **kw)
        lower(big, bz.NormL1(0.1), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64)
        with pytest.raises(ValueError, match="finite in float32"):
            lower(big, bz.NormL1(0.1), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float32)
    A = np.ones((2, n))
    with pytest.raises(bz.UnsupportedOracle, match="SparseGLM.*slack"):
        lower(f, bz.NormL1(0.1), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64, slack=True)
    with pytest.raises(bz.UnsupportedOracle, match="SparseGLM.*DenseAffine"):
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
    # callbacks mixed in: a g that is not lowered sends the same object through the callback kinds, all four together
    class MyL1:
        def prox(self, z, x, gamma):
            z[...] = x
            return 0.0
    desc, keep = lower(f, MyL1(), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64)
    assert (desc.f_kind, desc.g_kind, desc.c_kind, desc.D_kind) == (bz._lib.BZ_F_CALLBACK, bz._lib.BZ_G_CALLBACK,
                                                                    bz._lib.BZ_C_CALLBACK, bz._lib.BZ_D_CALLBACK)


def test_sparse_glm_is_reproducible(bz):
    m, n, k = 256, 64, 5
    las, log = bz.synth.sparse_lasso(m, n, k), bz.synth.sparse_logistic(m, n, k)
    for loss in LOSSES:
        a, b = bz.synth.sparse_glm(m, n, k, loss), bz.synth.sparse_glm(m, n, k, loss)
        assert all(np.array_equal(a[key], b[key]) for key in ("indptr", "indices", "data", "b", "xstar"))
        assert not np.array_equal(a["data"], bz.synth.sparse_glm(m, n, k, loss, seed=7)["data"])
        assert all(np.array_equal(a[key], las[key]) for key in ("indptr", "indices", "data"))
        assert a["loss"] == loss and a["delta"] == (1.0 if loss == "huber" else None) and a["b"].dtype == np.float64
        c = bz.synth.sparse_glm(m, n, k, loss, np.float32)
        assert c["data"].dtype == c["b"].dtype == np.float32 and np.array_equal(c["indices"], a["indices"])
        f = bz.SparseGLM(a["indptr"], a["indices"], a["data"], a["b"], n, loss, delta=a["delta"])     # the data pass the validation
        if loss in ("logistic", "squared_hinge"):
            assert np.array_equal(a["b"], log["labels"]) and np.array_equal(a["xstar"], las["xstar"])
        elif loss == "least_squares":
            assert np.array_equal(a["b"], las["b"])
        elif loss == "huber":
            out = np.arange(m) % 16 == 15
            assert np.array_equal(a["b"][~out], las["b"][~out]) and np.all(np.abs(a["b"][out] - las["b"][out]) >= 5.0)
        else:
            t = f.toarray() @ a["xstar"]
            assert np.max(np.abs(t)) <= 2.0 + 1e-12 and abs(np.max(np.abs(t)) - 2.0) <= 1e-12
            assert np.all(a["b"] == np.round(a["b"])) and a["b"].min() == 0 and 0.5 < a["b"].mean() / np.exp(t).mean() < 2.0
    with pytest.raises(ValueError):
        bz.synth.sparse_glm(4, 3, 5, "huber")
    with pytest.raises(ValueError, match="loss"):
        bz.synth.sparse_glm(m, n, k, "hinge")
