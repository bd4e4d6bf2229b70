"""K independent row losses of a sparse A in CSR (bz.SparseMultiGLM, BZ_F_SPARSE_MULTI_GLM), everything that needs no GPU: the
class's validation, its numpy value and gradient against a dense float64 formula and against K SparseGLM problems, its lowering
to the C descriptor (no new field: f_classes, f_loss, f_loss_delta, f_w, f_scale; f_b holds B row-major), the generator
bz.synth.sparse_multiresponse, and the Julia shim's lower_f! line."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bazinga_jl_amd.oracles import lower
from tests.test_gpu_sparse import csr_of, structured

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSSES = ("least_squares", "logistic", "huber", "squared_hinge", "poisson")


def small():
    """3 x 4, five entries, B 3 x 3"""
    indptr, indices, data = np.array([0, 2, 3, 5]), np.array([0, 3, 1, 2, 3]), np.arange(1.0, 6.0)
    B = np.array([[1.0, -1.0, 1.0], [-1.0, -1.0, 1.0], [1.0, 1.0, -1.0]])
    return indptr, indices, data, B, 4


def B_of(loss, rng, m, K, dtype=np.float64):
    if loss in ("logistic", "squared_hinge"):
        return np.where(rng.random((m, K)) < 0.5, -1.0, 1.0).astype(dtype)
    if loss == "poisson":
        return rng.integers(0, 4, (m, K)).astype(dtype)
    return rng.standard_normal((m, K)).astype(dtype)


def test_validation_errors(bz):
    indptr, indices, data, B, nf = small()
    f = bz.SparseMultiGLM(indptr, indices, data, B, nf, "logistic")
    assert (f.nnz, f.n_features, f.n_classes, f.n, f.m, f.scale, f.weights, f.delta) == (5, 4, 3, 12, 3, 1.0, None, None)
    assert f.b.shape == (9,) and np.array_equal(f.b, B.reshape(-1)) and f.B.shape == (3, 3)
    # B's shape: (m, K), 2 <= K <= 64; a vector points to SparseGLM
    with pytest.raises(ValueError, match="SparseGLM"):
        bz.SparseMultiGLM(indptr, indices, data, B[:, 0], nf, "logistic")
    with pytest.raises(ValueError, match="two-dimensional"):
        bz.SparseMultiGLM(indptr, indices, data, B[:, :, None], nf, "logistic")
    for bad_k in (1, 65, 0):
        with pytest.raises(ValueError, match="2 \\.\\. 64"):
            bz.SparseMultiGLM(indptr, indices, data, np.ones((3, bad_k)), nf, "least_squares")
    assert bz.SparseMultiGLM(indptr, indices, data, np.ones((3, 64), np.int64), nf, "least_squares").B.dtype == np.float64
    assert bz.SparseMultiGLM(indptr, indices, data, np.ones((3, 2)), nf, "least_squares").n == 8
    with pytest.raises(ValueError, match="indptr"):                                   # a row of B too many
        bz.SparseMultiGLM(indptr, indices, data, np.ones((4, 3)), nf, "least_squares")
    # the loss, and the label / count / delta checks of SparseGLM on every entry of B
    with pytest.raises(ValueError, match="unknown loss"):
        bz.SparseMultiGLM(indptr, indices, data, B, nf, "hinge")
    for loss in ("logistic", "squared_hinge"):
        for i, k, v in ((0, 0, 0.0), (2, 2, 2.0), (1, 1, np.nan)):
            bad = B.copy()
            bad[i, k] = v
            with pytest.raises(ValueError, match="labels"):
                bz.SparseMultiGLM(indptr, indices, data, bad, nf, loss)
    for v in (-1.0, np.inf, np.nan):
        bad = np.abs(B)
        bad[2, 1] = v
        with pytest.raises(ValueError, match="counts"):
            bz.SparseMultiGLM(indptr, indices, data, bad, nf, "poisson")
    for bad in (None, 0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="delta"):
            bz.SparseMultiGLM(indptr, indices, data, B, nf, "huber", delta=bad)
    with pytest.raises(ValueError, match="delta"):
        bz.SparseMultiGLM(indptr, indices, data, B, nf, "logistic", delta=1.0)
    assert bz.SparseMultiGLM(indptr, indices, data, B, nf, "huber", delta=2).delta == 2.0
    # the matrix checks of SparseLeastSquares, with n_features columns; the 2^31 limits
    with pytest.raises(ValueError, match="indptr"):
        bz.SparseMultiGLM(np.array([0, 3, 2, 5]), indices, data, B, nf, "logistic")
    with pytest.raises(ValueError, match="column indices"):
        bz.SparseMultiGLM(indptr, np.array([0, 3, 1, 4, 3]), data, B, nf, "logistic")
    with pytest.raises(ValueError, match="same length"):
        bz.SparseMultiGLM(indptr, indices, data[:4], B, nf, "logistic")
    with pytest.raises(ValueError, match="integer"):
        bz.SparseMultiGLM(indptr.astype(np.float64), indices, data, B, nf, "logistic")
    with pytest.raises(ValueError, match="float64 or float32"):
        bz.SparseMultiGLM(indptr, indices, data.astype(np.int64), B, nf, "logistic")
    with pytest.raises(ValueError, match="2\\^31"):
        bz.SparseMultiGLM(indptr, indices, data, B, 2 ** 30, "logistic")              # n_features * K is beyond 2^31 - 1
    with pytest.raises(ValueError, match="2\\^31"):
        bz.SparseMultiGLM(indptr, indices, data, B, 0, "logistic")
    assert bz.SparseMultiGLM(indptr, indices, data, np.ones((3, 2)), (2 ** 31 - 1) // 2, "least_squares").n == 2 ** 31 - 2
    # weights (one per ROW), scale: SparseGLM's rules
    for bad in (np.array([1.0, -0.5, 1.0]), np.array([1.0, np.nan, 1.0]), np.array([1.0, np.inf, 1.0]), np.ones(2), np.ones((3, 3)), np.ones(9)):
        with pytest.raises(ValueError, match="weights"):
            bz.SparseMultiGLM(indptr, indices, data, B, nf, "logistic", weights=bad)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="scale"):
            bz.SparseMultiGLM(indptr, indices, data, B, nf, "logistic", scale=bad)
    w = np.array([1.0 / 3.0, 0.1, 7.0])
    h = bz.SparseMultiGLM(indptr, indices, data, B, nf, "logistic", weights=w, scale=1.0 / 3.0)
    assert np.array_equal(h.row_weights(np.float32), ((1.0 / 3.0) * w).astype(np.float32))          # one rounding
    x = np.arange(12.0)
    assert f.coef(x).shape == (4, 3) and f.coef(x)[2, 1] == x[2 * 3 + 1] and np.shares_memory(f.coef(x), x)
    assert bz.SparseMultiGLM.LOSSES == bz.SparseGLM.LOSSES == LOSSES


def test_from_dense_round_trip(bz):
    for m, nf, p in ((120, 40, 0.02), (3, 70, 0.5)):
        A = structured(m, nf, p, np.random.default_rng(m + nf), False, np.float64)
        f = bz.SparseMultiGLM.from_dense(A, np.zeros((m, 5)), "least_squares", weights=np.ones(m), scale=1.0 / m)
        assert np.array_equal(f.toarray(), A) and f.nnz == np.count_nonzero(A) and (f.m, f.n_features, f.n) == (m, nf, 5 * nf)
        assert f.indptr.dtype == np.int64 and f.indices.dtype == np.int32 and f.scale == 1.0 / m


def dense_value_and_gradient(A, B, X, w, loss, delta):
    """sum_i w_i sum_k l(B_ik, t_ik) and A'(w l') in float64, written independently of the class"""
    t = A @ X
    if loss == "least_squares":
        l, dl = 0.5 * (t - B) ** 2, t - B
    elif loss == "logistic":
        l, dl = np.logaddexp(0.0, -B * t), -B / (1.0 + np.exp(B * t))
    elif loss == "huber":
        v = t - B
        l = np.where(np.abs(v) <= delta, 0.5 * v * v, delta * (np.abs(v) - 0.5 * delta))
        dl = np.clip(v, -delta, delta)
    elif loss == "squared_hinge":
        h = np.maximum(0.0, 1.0 - B * t)
        l, dl = 0.5 * h * h, -B * h
    else:
        l, dl = np.exp(t) - B * t, np.exp(t) - B
    return float(np.sum(w[:, None] * l)), A.T @ (w[:, None] * dl)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("loss", LOSSES)
def test_numpy_class_against_a_dense_formula_and_K_scalar_problems(bz, loss, K, weighted):
    """value and gradient against the dense float64 formula (1e-13 of max(1, |value|) and of the gradient's largest entry: a
    few ulps per sum of at most 17 terms), and column k of the gradient against SparseGLM(A, B[:, k]).gradient within 1e-13
    relative; unsorted rows and a duplicated entry included.  float32 runs in float32."""
    rng = np.random.default_rng(5 + K)
    m, nf = 17, 9
    A = structured(m, nf, 0.4, rng, False, np.float64)
    indptr, indices, data = csr_of(A, np.random.default_rng(1))
    k0 = indptr[2]                                            # duplicate the first entry of row 2: 2 a = a + a
    indices, data = np.insert(indices, k0, indices[k0]), np.insert(data, k0, data[k0])
    indptr[3:] += 1
    A[2, indices[k0]] *= 2
    B = B_of(loss, rng, m, K)
    delta = 0.7 if loss == "huber" else None
    w = rng.uniform(0.0, 2.0, m) if weighted else None
    scale = 1.0 / m if weighted else 1.0
    f = bz.SparseMultiGLM(indptr, indices, data, B, nf, loss, delta=delta, weights=w, scale=scale)
    assert np.array_equal(f.toarray(), A)
    x = 0.5 * rng.standard_normal(nf * K)
    g = np.empty(nf * K)
    fx = f.gradient(g, x)
    assert type(fx) is np.float64 and fx == f(x)
    w64 = f.row_weights(np.float64) * np.ones(m)
    v_ref, G_ref = dense_value_and_gradient(A, B, f.coef(x), w64, loss, delta)
    assert abs(fx - v_ref) <= 1e-13 * max(1.0, abs(v_ref))
    assert np.max(np.abs(f.coef(g) - G_ref)) <= 1e-13 * np.max(np.abs(G_ref))
    total = 0.0
    for k in range(K):
        fk = bz.SparseGLM(indptr, indices, data, B[:, k], nf, loss, delta=delta, weights=w, scale=scale)
        gk = np.empty(nf)
        total += float(fk.gradient(gk, np.ascontiguousarray(f.coef(x)[:, k])))
        assert np.max(np.abs(f.coef(g)[:, k] - gk)) <= 1e-13 * np.max(np.abs(gk))
    assert abs(fx - total) <= 1e-13 * max(1.0, abs(total))
    x32, g32 = x.astype(np.float32), np.empty(nf * K, np.float32)
    f32 = f.gradient(g32, x32)
    assert type(f32) is np.float32 and abs(float(f32) - fx) <= 1e-5 * max(1.0, abs(fx)) and np.max(np.abs(g32 - g)) <= 1e-5 * np.max(np.abs(g))


def test_numpy_responses_are_isolated(bz):
    """a NaN or an infinity in one t_ik reaches r_ik and the value, and leaves the row's other entries of R as they were"""
    K, m = 3, 4
    ident = (np.arange(m + 1), np.arange(m), np.ones(m))
    B = np.array([[1.0, 0.0, 2.0]] * m)
    f = bz.SparseMultiGLM(*ident, B, m, "poisson", scale=0.5)
    x = np.linspace(-1.0, 1.0, m * K)
    _, R0 = f._loss_r(x)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[1 * K + 2] = bad
        terms, R = f._loss_r(y)
        same = np.ones((m, K), bool)
        same[1, 2] = False
        assert np.array_equal(R[same], R0[same])
        assert (np.isnan(R[1, 2]) if bad != bad else R[1, 2] == (np.inf if bad > 0 else 0.5 * (0.0 - 2.0)))
        assert np.isnan(terms[1, 2]) if bad != bad else terms[1, 2] == np.inf           # (b = 2, t = -inf: e - b t = +inf)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lower_fills_the_descriptor(bz, dtype):
    L = bz._lib
    indptr, indices, data, B, nf = small()
    K = B.shape[1]
    m, n, ny = 3, nf * K, 2
    ct = C.c_double if dtype == np.float64 else C.c_float
    A = np.zeros((ny, n), dtype)
    A[0, :] = 1
    A[1, 3] = 2
    cs = bz.SparseAffine.from_dense(A, np.zeros(ny, dtype))
    w = np.array([0.5, 0.0, 2.0])
    Bv = B + np.arange(9.0).reshape(3, 3)                          # (distinct values: the order of f_b is visible)
    for loss, delta, BB in (("logistic", None, B), ("huber", 1.5, Bv), ("least_squares", None, Bv), ("poisson", None, np.abs(Bv))):
        for weights, scale in ((None, 1.0), (w, 1.0 / m)):
            f = bz.SparseMultiGLM(indptr, indices, data.astype(dtype), BB, nf, loss, delta=delta, weights=weights, scale=scale)
            for c, rows in ((bz.IdentityFunction(), n), (cs, ny)):
                desc, keep = lower(f, bz.NormL1(0.1), c, bz.ZeroSet(), n, rows, dtype)
                assert desc.f_kind == L.BZ_F_SPARSE_MULTI_GLM == 11 and desc.f_classes == K and desc.f_rows == m
                assert desc.f_loss == LOSSES.index(loss) and desc.f_loss_delta == (delta or 0.0)
                assert desc.n == n and desc.f_sp_nnz == f.nnz == 5 and desc.f_scale == scale
                assert desc.c_kind == (L.BZ_C_SPARSE_AFFINE if c is cs else L.BZ_C_IDENTITY)
                rp = np.ctypeslib.as_array(C.cast(desc.f_sp_rowptr, C.POINTER(C.c_int64)), shape=(m + 1,))
                col = np.ctypeslib.as_array(C.cast(desc.f_sp_col, C.POINTER(C.c_int32)), shape=(f.nnz,))
                val = np.ctypeslib.as_array(C.cast(desc.f_sp_val, C.POINTER(ct)), shape=(f.nnz,))
                bb = np.ctypeslib.as_array(C.cast(desc.f_b, C.POINTER(ct)), shape=(m * K,))
                assert np.array_equal(rp, f.indptr) and np.array_equal(col, f.indices) and np.array_equal(val, f.data)
                # m K values, row-major: f_b[i K + k] = B[i, k]
                assert bb.dtype == dtype and np.array_equal(bb.reshape(m, K), BB) and bb[1 * K + 2] == BB[1, 2]
                assert not desc.f_A and not desc.f_q
                if weights is None:
                    assert not desc.f_w
                else:                                           # the weights as given, one per row: the library folds the scale in
                    ww = np.ctypeslib.as_array(C.cast(desc.f_w, C.POINTER(ct)), shape=(m,))
                    assert np.array_equal(ww, w.astype(dtype))
    # no descriptor field was added: the pinned neighbourhoods are where they were
    names = [nm for nm, _ in L.ProblemDesc._fields_]
    assert names[names.index("f_rows") + 1] == "f_classes" and names[names.index("f_classes") + 1] == "g_lambda"
    assert names[-8:-4] == ["f_loss", "f_loss_delta", "f_w", "f_scale"] and names[-9] == "f_sp_nnz"
    header = open(os.path.join(ROOT, "include", "bazinga_hip.h")).read()
    assert re.search(r"#define BZ_F_SPARSE_MULTI_GLM\s+11\b", header)


def test_lower_refuses_or_reroutes_before_any_device_call(bz):
    """lower() raises UnsupportedOracle for the slack form and for a dense c, ValueError for a variable that is not
    n_features * K long and for numbers that are not finite in float32; a mix with an oracle that is not lowered goes through
    the callback kinds, all four together, and the callback is the class's numpy gradient"""
    indptr, indices, data, B, nf = small()
    n = nf * B.shape[1]
    f = bz.SparseMultiGLM(indptr, indices, data, B, nf, "squared_hinge")
    for kw in ({"scale": 1e300}, {"weights": np.array([1.0, 1e30, 1.0]), "scale": 1e30}, {"loss": "huber", "delta": 1e300}):
        big = bz.SparseMultiGLM(indptr, indices, data, B, nf, kw.pop("loss", "squared_hinge"), **kw)
        lower(big, bz.NormL1(0.1), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64)
        with pytest.raises(ValueError, match="finite in float32"):
            lower(big, bz.NormL1(0.1), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float32)
    A = np.ones((2, n))
    with pytest.raises(bz.UnsupportedOracle, match="SparseMultiGLM.*slack"):
        lower(f, bz.NormL1(0.1), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64, slack=True)
    with pytest.raises(bz.UnsupportedOracle, match="SparseMultiGLM.*DenseAffine"):
        lower(f, bz.NormL1(0.1), bz.DenseAffine(A, np.zeros(2)), bz.ZeroSet(), n, 2, np.float64)
    for bad_n in (nf, n + 1, n + 3):
        with pytest.raises(ValueError, match="n_features \\* K"):
            lower(f, bz.NormL1(0.1), bz.IdentityFunction(), bz.ZeroSet(), bad_n, bad_n, np.float64)
    # the multi-task Lasso's g lowers beside it
    desc, keep = lower(f, bz.NormL21(0.1, 3), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64)
    assert desc.g_kind == bz._lib.BZ_G_NORM_L21 and desc.g_group == 3 and desc.f_kind == 11

    class MyL1:
        def prox(self, z, x, gamma):
            z[...] = x
            return 0.0
    desc, keep = lower(f, MyL1(), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64)
    assert (desc.f_kind, desc.g_kind, desc.c_kind, desc.D_kind) == (bz._lib.BZ_F_CALLBACK, bz._lib.BZ_G_CALLBACK,
                                                                    bz._lib.BZ_C_CALLBACK, bz._lib.BZ_D_CALLBACK)
    x = np.linspace(-1.0, 1.0, n)
    out, g = np.empty(n), np.empty(n)
    fx = desc.cb_f_gradient(None, x.ctypes.data, out.ctypes.data, n)
    assert fx == float(f.gradient(g, x)) and np.array_equal(out, g)


@pytest.mark.parametrize("loss", LOSSES)
def test_sparse_multiresponse_is_reproducible(bz, loss):
    m, nf, K, k = 256, 16, 4, 5
    mn = bz.synth.sparse_multinomial(m, nf, K, k)
    a, b = bz.synth.sparse_multiresponse(m, nf, K, k, np.float64, loss), bz.synth.sparse_multiresponse(m, nf, K, k, loss=loss)
    assert all(np.array_equal(a[key], b[key]) for key in ("indptr", "indices", "data", "B", "xstar"))
    assert all(np.array_equal(a[key], mn[key]) for key in ("indptr", "indices", "data"))            # sparse_multinomial's matrix
    assert (a["m"], a["n_f"], a["K"], a["n"], a["loss"]) == (m, nf, K, nf * K, loss) and a["B"].shape == (m, K) and a["B"].dtype == np.float64
    assert a["delta"] == (1.0 if loss == "huber" else None)
    c = bz.synth.sparse_multiresponse(m, nf, K, k, np.float32, loss)
    assert c["data"].dtype == c["B"].dtype == np.float32 and np.array_equal(c["indices"], a["indices"])
    f = bz.SparseMultiGLM(a["indptr"], a["indices"], a["data"], a["B"], nf, loss, delta=a["delta"])  # the data pass the validation
    # X* is row-sparse: a tenth of the features, active in all K responses; it explains B better than X = 0 does
    Xs = f.coef(a["xstar"])
    assert np.count_nonzero(Xs.any(axis=1)) == np.count_nonzero(Xs.all(axis=1)) == max(1, nf // 10)
    assert f(a["xstar"]) < f(np.zeros(nf * K))
    if loss in ("logistic", "squared_hinge"):
        assert set(np.unique(a["B"])) == {-1.0, 1.0}
    if loss == "poisson":
        assert np.array_equal(a["B"], np.floor(a["B"])) and a["B"].min() == 0 and a["B"].max() >= 2
    for bad in ((4, 3, 3, 5), (4, 8, 1), (4, 8, 65)):
        with pytest.raises(ValueError):
            bz.synth.sparse_multiresponse(*bad)
    with pytest.raises(ValueError):
        bz.synth.sparse_multiresponse(m, nf, K, k, loss="hinge")


def test_the_julia_shim_lowers_the_kind():
    src = open(os.path.join(ROOT, "julia", "BazingaHIP.jl")).read()
    assert re.search(r"^struct SparseMultiGLM\{T\} <: Bazinga\.ProximableFunction", src, re.M)
    m = re.search(r"function lower_f!\(d, f::SparseMultiGLM\)\n(.*?)\nend", src, re.S)
    body = m.group(1)
    assert re.search(r"d\.f_kind = 11; d\.f_rows = size\(f\.B, 1\); d\.f_classes = f\.K;", body)
    assert re.search(r"d\.f_b = pointer\(f\.b\)", body) and re.search(r"d\.f_loss = f\.loss; d\.f_loss_delta = f\.delta; d\.f_scale = f\.scale", body)
    assert re.search(r"d\.f_w = f\.w === nothing \? C_NULL : pointer\(f\.w\)", body)
    assert re.search(r"vec\(permutedims\(B\)\)", src)                                  # B goes to the library row-major
