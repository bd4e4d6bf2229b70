"""f(x) = 0.5 x'Qx + q'x with a sparse symmetric Q (bz.SparseQuadratic, BZ_F_SPARSE_QUADRATIC), everything that needs no GPU:
the class's validation and host mirrors, its lowering to the C descriptor, the generators of bz.synth, and the launch plans
that the case list of tests/test_gpu_sparse_quadratic.py takes."""
import ctypes as C

import numpy as np
import pytest

from bazinga_jl_amd.oracles import lower
from tests.test_gpu_sparse import csr_of, plan

# (n, density) of tests/test_gpu_sparse_quadratic.py and the lanes per row each one takes
CASES = [(3, 1.0), (70, 0.03), (121, 0.05), (257, 0.1), (257, 0.2), (303, 0.35), (521, 0.5), (1031, 0.9), (1031, 0.012)]
LANES = [1, 2, 4, 8, 16, 32, 64, 64, 4]


def sym_structured(n, p, integer, dtype, rng=None):
    """symmetric, density p, with a full row / column 0 and an empty row / column 1: M with entries of {-2, -1, 1, 2}
    (integer) or normal ones under a density-p mask, Q = triu(M) + triu(M, 1)'"""
    rng = np.random.default_rng(n * 7 + int(p * 1000)) if rng is None else rng
    pick = lambda size: rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), size)
    M = pick((n, n)) if integer else rng.standard_normal((n, n)) / np.sqrt(max(1.0, p * n))
    M = M * (rng.random((n, n)) < p)
    Q = np.triu(M) + np.triu(M, 1).T
    full = pick(n) if integer else rng.standard_normal(n) / np.sqrt(n)
    Q[0, :] = full
    Q[:, 0] = full
    if n > 2:
        Q[1, :] = 0
        Q[:, 1] = 0
    return Q.astype(dtype)


def test_validation_errors(bz):
    indptr, indices, data, q = np.array([0, 2, 3, 5]), np.array([0, 2, 1, 0, 2]), np.array([1.0, 5.0, 2.0, 5.0, 3.0]), np.zeros(3)
    f = bz.SparseQuadratic(indptr, indices, data, q)
    assert f.nnz == 5 and f.n == 3
    with pytest.raises(ValueError, match="indptr"):
        bz.SparseQuadratic(np.array([0, 3, 2, 5]), indices, data, q)
    with pytest.raises(ValueError, match="indptr"):
        bz.SparseQuadratic(np.array([0, 2, 3]), indices, data, q)
    with pytest.raises(ValueError, match="column indices"):
        bz.SparseQuadratic(indptr, np.array([0, 3, 1, 0, 2]), data, q)
    skew = np.array([1.0, 5.0, 2.0, 4.0, 3.0])
    with pytest.raises(ValueError, match="symmetric"):
        bz.SparseQuadratic(indptr, indices, skew, q)
    g = bz.SparseQuadratic(indptr, indices, skew, q, check_symmetric=False)
    assert g.toarray()[2, 0] == 4.0 and g.toarray()[0, 2] == 5.0
    # an entry stored on one side of the diagonal only is not symmetric either
    with pytest.raises(ValueError, match="symmetric"):
        bz.SparseQuadratic(np.array([0, 1, 1]), np.array([1]), np.array([1.0]), np.zeros(2))
    # a duplicated index contributes twice: 2 + 3 on one side equals 5 on the other
    bz.SparseQuadratic(np.array([0, 2, 3]), np.array([1, 1, 0]), np.array([2.0, 3.0, 5.0]), np.zeros(2))


def test_from_dense_round_trip(bz):
    for n, p in CASES[:4]:
        Q = sym_structured(n, p, False, np.float64)
        f = bz.SparseQuadratic.from_dense(Q, np.zeros(n))
        assert np.array_equal(f.toarray(), Q) and f.nnz == np.count_nonzero(Q)
        assert f.indptr.dtype == np.int64 and f.indices.dtype == np.int32


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_host_mirrors_agree_with_the_dense_oracle(bz, ref, dtype):
    """unsorted rows and a duplicated entry included; 1e-13 relative in fp64 (fp32: the same bound in units of its eps)"""
    rng = np.random.default_rng(11)
    n = 97
    Q = sym_structured(n, 0.15, False, dtype, rng)
    indptr, indices, data = csr_of(Q, np.random.default_rng(1))
    # duplicate the first entry of row 2 (and of column 2, to stay symmetric): half of it twice
    r, k = 2, indptr[2]
    c = indices[k]
    assert c != r
    kt = indptr[c] + int(np.flatnonzero(indices[indptr[c]:indptr[c + 1]] == r)[0])
    for at in sorted((k, kt), reverse=True):
        row = np.searchsorted(indptr, at, side="right") - 1
        data[at] = data[at] / 2
        indices = np.insert(indices, at, indices[at])
        data = np.insert(data, at, data[at])
        indptr[row + 1:] += 1
    q = rng.standard_normal(n).astype(dtype)
    f = bz.SparseQuadratic(indptr, indices, data, q)
    assert np.array_equal(f.toarray(), Q)
    o = ref.Quadratic(f.toarray(), q)
    tol = 1e-13 * (np.finfo(dtype).eps / np.finfo(np.float64).eps)
    for _ in range(3):
        x = rng.standard_normal(n).astype(dtype)
        ga, gb = np.empty(n, dtype), np.empty(n, dtype)
        fa, fb = f.gradient(ga, x), o.gradient(gb, x)
        assert ga.dtype == dtype
        print(f"gradient {np.max(np.abs(ga - gb)) / np.max(np.abs(gb)):.3e} value {abs(fa - fb) / abs(fb):.3e} (f = {fb:.6g})")
        assert np.max(np.abs(ga - gb)) <= tol * np.max(np.abs(gb))
        assert abs(fa - fb) <= tol * abs(fb)
        assert abs(f(x) - o(x)) <= tol * abs(fb)
        assert f(x) == fa


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_lower_fills_the_descriptor(bz, dtype):
    L = bz._lib
    n, ny = 6, 4
    d2 = bz.synth.laplacian_2d(2, 3, dtype)
    q = np.arange(6).astype(dtype)
    f = bz.SparseQuadratic(d2["indptr"], d2["indices"], d2["data"], q)
    A = np.zeros((ny, n), dtype)
    A[0, :] = 1
    A[2, 3] = 2
    cs = bz.SparseAffine.from_dense(A, np.zeros(ny, dtype))
    for c, m in ((bz.IdentityFunction(), n), (cs, ny)):
        desc, keep = lower(f, bz.NormL1(0.1), c, bz.ZeroSet(), n, m, dtype)
        assert desc.f_kind == L.BZ_F_SPARSE_QUADRATIC == 6 and desc.f_sp_nnz == f.nnz == 20
        assert desc.c_kind == (L.BZ_C_SPARSE_AFFINE if c is cs else L.BZ_C_IDENTITY)
        rp = np.ctypeslib.as_array(C.cast(desc.f_sp_rowptr, C.POINTER(C.c_int64)), shape=(n + 1,))
        col = np.ctypeslib.as_array(C.cast(desc.f_sp_col, C.POINTER(C.c_int32)), shape=(f.nnz,))
        ct = C.c_double if dtype == np.float64 else C.c_float
        val = np.ctypeslib.as_array(C.cast(desc.f_sp_val, C.POINTER(ct)), shape=(f.nnz,))
        qq = np.ctypeslib.as_array(C.cast(desc.f_b, C.POINTER(ct)), shape=(n,))
        assert np.array_equal(rp, f.indptr) and np.array_equal(col, f.indices) and np.array_equal(val, f.data)
        assert np.array_equal(qq, q) and not desc.f_A and not desc.f_q
    with pytest.raises(bz.UnsupportedOracle, match="slack"):
        lower(f, bz.NormL1(0.1), bz.IdentityFunction(), bz.ZeroSet(), n, n, dtype, slack=True)
    with pytest.raises(bz.UnsupportedOracle, match="DenseAffine"):
        lower(f, bz.NormL1(0.1), bz.DenseAffine(A, np.zeros(ny, dtype)), bz.ZeroSet(), n, ny, dtype)
    # the message of the sparse c for any other f stays as worded
    with pytest.raises(bz.UnsupportedOracle, match=r"element-wise f \(Zero, DiagQuadratic\), not Quadratic"):
        lower(bz.Quadratic(f.toarray(), q), bz.NormL1(0.1), cs, bz.ZeroSet(), n, ny, dtype)


def test_generators(bz, ref):
    nx, ny = 12, 20
    a, b = bz.synth.laplacian_2d(nx, ny), bz.synth.laplacian_2d(nx, ny)
    assert all(np.array_equal(a[k], b[k]) for k in ("indptr", "indices", "data")) and a["n"] == nx * ny
    f = bz.SparseQuadratic(a["indptr"], a["indices"], a["data"], np.zeros(nx * ny))      # (symmetric: the check passes)
    x = np.random.default_rng(0).integers(-5, 6, nx * ny).astype(np.float64)
    assert np.array_equal(f.toarray() @ x, ref.Stencil5ptQuadratic(nx, ny, np.zeros(nx * ny))._Ax(x))
    assert f.nnz == 5 * nx * ny - 2 * nx - 2 * ny
    n, m = 300, 100
    s, t = bz.synth.sparse_qp(n, m, 7), bz.synth.sparse_qp(n, m, 7)
    assert all(np.array_equal(s[k], t[k]) for k in s)
    assert not np.array_equal(s["Q_data"], bz.synth.sparse_qp(n, m, 8)["Q_data"])
    F = bz.SparseQuadratic(s["Q_indptr"], s["Q_indices"], s["Q_data"], s["fq"])
    Q = F.toarray()
    off = np.abs(Q).sum(axis=1) - np.abs(np.diag(Q))
    assert np.all(np.diag(Q) > off) and 6.0 < F.nnz / n <= 7.0
    bb = bz.synth.budget_bands(n, m)
    assert all(np.array_equal(s[k], bb[k]) for k in bb)


def test_case_list_takes_every_lane_count_and_cut_rows():
    lanes, cut = [], []
    for n, p in CASES:
        Q = sym_structured(n, p, True, np.float64)
        assert np.array_equal(Q, Q.T) and np.all(np.delete(Q[0], 1) != 0) and (n <= 2 or not np.any(Q[1]))
        indptr, indices, data = csr_of(Q, np.random.default_rng(1))
        L, nv, seg = plan(indptr, data.shape[0])
        lanes.append(L); cut.append(seg)
        assert n % 4 != 0
    assert lanes == LANES, lanes
    assert set(lanes) == {1, 2, 4, 8, 16, 32, 64}
    assert cut == [False] * 6 + [True] * 3, cut
