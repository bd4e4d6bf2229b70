"""f(x) = 0.5||A x - b||^2 with a sparse A in CSR on the device (BZ_F_SPARSE_LEAST_SQUARES): the row kernels over A_f and A_f'
(k_spmv_ls_r, then k_spmv_ls_t_algrad: the whole AL gradient of c = Identity in two launches; k_spmv_ls_t, the plain product
for the three-launch form and beside a sparse c), the iterates and whole solves against the oracle, creation-time validation.

The oracle is ref.LeastSquares on the densified matrix throughout; c is ref.IdentityFunction or the CSR duck-type below."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_parity import run_traces
from tests.test_gpu_sparse import CASES32, CASES64, csr_of, plan, sets, structured, transpose_ptr
from tests.test_sparse_least_squares_host import CUT32

pytestmark = pytest.mark.gpu

IDS = lambda c: f"{'f64' if c[0] == np.float64 else 'f32'}-{c[1][0]}x{c[1][1]}-{c[1][2]}"
TYPED = [(np.float64, c) for c in CASES64] + [(np.float32, c) for c in CASES32]
# a sparse c beside the sparse f: (m, n, density) of A_f and (ny, density) of A_c on the same n, the row counts different
PAIRS = [((41, 121, 0.1), (30, 0.2)), ((257, 1031, 0.03), (41, 0.1))]
PAIR_IDS = lambda c: f"{'f64' if c[0] == np.float64 else 'f32'}-{c[1][0][0]}x{c[1][0][1]}+{c[1][1][0]}"


class CsrOracle:
    """eval!(cx, c, x) = A x - b, jtprod!(jtv, c, x, v) = A'v over CSR arrays, in the arrays' stored order (the duck-type of
    tests/test_gpu_sparse.py, restated)"""

    def __init__(self, indptr, indices, data, b, n):
        self.indices, self.data, self.b, self.n = np.asarray(indices), np.asarray(data), np.asarray(b), n
        self.ny = self.b.shape[0]
        self.rows = np.repeat(np.arange(self.ny), np.diff(indptr))

    def eval(self, cx, x):
        cx[...] = np.bincount(self.rows, weights=self.data * x[self.indices], minlength=self.ny) - self.b

    def jtprod(self, jtv, x, v):
        jtv[...] = np.bincount(self.indices, weights=self.data * v[self.rows], minlength=self.n)


def sparse_ls(bz, A, b, seed=1):
    indptr, indices, data = csr_of(A, np.random.default_rng(seed))
    return bz.SparseLeastSquares(indptr, indices, data, b, A.shape[1]), indptr, indices, data.shape[0]


def one_gradient(bz, dev, n, ny, dtype, mu, y, x, times=1):
    prob = bz.Problem(*dev, n, ny, dtype)
    prob.set_multipliers(mu, y)
    prob.profile_reset()
    prob.profile_enable(True)
    runs = [prob.eval_al_gradient(x) for _ in range(times)]
    pr = prob.profile2()
    prob.close()
    return runs[0] if times == 1 else runs, pr


def integer_inputs(m, n, p, ny, dtype):
    """A_f of {-2, -1, 1, 2} under a density-p mask (structured), b in [-3, 3], x in [-4, 4], y in [-3, 3], mu = 1/4"""
    rng = np.random.default_rng(m * 7 + n)
    A = structured(m, n, p, rng, True, dtype)
    return (A, rng.integers(-3, 4, m).astype(dtype), rng.integers(-4, 5, n).astype(dtype), rng.integers(-3, 4, ny).astype(dtype),
            np.full(ny, 0.25, dtype), rng)


def assert_exact_in(dtype, A, b, x, y, make_al, al, lx, g_ref, Ac=None, bc=None):
    """Exactness, whatever the order of any sum, asserted on the oracle's float64 recomputation (make_al(np.float64)): the
    sums of magnitudes that bound every partial sum — of a row of A_f x - b, of a row of A_f' r plus the penalty part of
    the gradient (beside a sparse c: of a row of A_c x - b_c in quarters and of A_c' yhat), and of the value in units of
    its finest granularity (1/8: mu y^2 / 2) — stay below a tenth of 2^24 (fp32) / 2^53 (fp64).  Then the oracle in dtype
    has returned the float64 values."""
    lim = 2.0 ** (24 if dtype == np.float32 else 53) / 10
    x64, y64, absA = x.astype(np.float64), y.astype(np.float64), np.abs(A.astype(np.float64))
    al64, lx64, g64 = make_al(np.float64)
    r = A.astype(np.float64) @ x64 - b
    yhat = al64.yupd
    t = yhat * 0.25
    assert np.max(absA @ np.abs(x64) + np.abs(b)) < lim
    pen_part = np.max(np.abs(yhat))
    if Ac is not None:
        absC = np.abs(Ac.astype(np.float64))
        assert 4 * np.max(absC @ np.abs(x64) + np.abs(bc)) < lim
        pen_part = np.max(absC.T @ np.abs(yhat))
    assert np.max(absA.T @ np.abs(r)) + pen_part < lim
    assert 8 * (0.5 * np.sum(r * r) + 0.5 * np.sum(t * t / 0.25) + 0.5 * np.sum(0.25 * y64 ** 2)) < lim
    assert float(lx) == float(lx64) and float(al.fx) == float(al64.fx) == 0.5 * np.sum(r * r)
    assert np.array_equal(g_ref.astype(np.float64), g64)


def exact_identity(bz, ref, dtype, case, D_name):
    m, n, p = case
    A, b, x, y, mu, _ = integer_inputs(m, n, p, n, dtype)
    f, indptr, indices, nnz = sparse_ls(bz, A, b)
    (g_dev, vals), pr = one_gradient(bz, (f, bz.NormL1(1.0), bz.IdentityFunction(), sets(bz, ref, D_name, dtype)[0]), n, n, dtype, mu, y, x)

    def make_al(dt):
        al = ref.AugLagFun(ref.LeastSquares(A.astype(dt), b.astype(dt)), ref.IdentityFunction(), sets(bz, ref, D_name, dt)[1],
                           mu.astype(dt), y.astype(dt), x.astype(dt))
        g = np.empty(n, dt)
        return al, al.gradient(g, x.astype(dt)), g
    al, lx, g_ref = make_al(dtype)
    assert_exact_in(dtype, A, b, x, y, make_al, al, lx, g_ref)
    assert g_dev.dtype == dtype and np.array_equal(g_dev, g_ref)
    assert vals[0] == float(lx) and vals[1] == float(al.fx)
    return pr, plan(indptr, nnz), plan(transpose_ptr(indices, n), nnz)


@pytest.mark.parametrize("D", ["zero", "free", "box"])
@pytest.mark.parametrize("case", TYPED, ids=IDS)
def test_exact_gradient_bit_for_bit(bz, ref, case, D):
    """Integer data, mu = 1/4: every product and every sum is exact in the number format, so no summation order can change
    a bit: gradient, Lagrangian and f equal the oracle's BIT FOR BIT.  Two row launches, no element-wise kernel."""
    dtype, shape = case
    pr, (La, _, seg_a), (Lt, _, seg_t) = exact_identity(bz, ref, dtype, shape, D)
    assert pr["gemv"]["form"] == f"k_spmv_ls_t_algrad<L={Lt},SEG={int(seg_t)}>", pr["gemv"]["form"]
    assert pr["gemv"]["launches"] == 2 and pr["al_gradient"]["launches"] == 0
    assert pr["misc"]["launches"] == int(seg_a) + int(seg_t)                  # a fold launch per cut matrix


@pytest.mark.parametrize("case", [(np.float64, (257, 1031, 0.9)), (np.float64, (1031, 257, 0.9)), (np.float32, (41, 121, 0.25))], ids=IDS)
def test_exact_gradient_in_the_three_launch_form(bz, ref, case, monkeypatch):
    """BZ_SPLS_FUSED=0 on integer data: the plain product over A_f' and k_algrad_elem in its mode 1, bit for bit too"""
    dtype, shape = case
    monkeypatch.setenv("BZ_SPLS_FUSED", "0")
    pr, _, (Lt, _, seg_t) = exact_identity(bz, ref, dtype, shape, "box")
    assert pr["gemv"]["form"] == f"k_spmv_ls_t<L={Lt},SEG={int(seg_t)}>", pr["gemv"]["form"]
    assert pr["gemv"]["launches"] == 2 and pr["al_gradient"]["launches"] == 1


def real_inputs(m, n, p, ny, dtype):
    rng = np.random.default_rng(m * 11 + n)
    A = structured(m, n, p, rng, False, dtype)
    return (A, rng.standard_normal(m).astype(dtype), rng.standard_normal(n).astype(dtype), rng.standard_normal(ny).astype(dtype),
            (10.0 ** rng.uniform(-2, 0, ny)).astype(dtype), rng)


def general_runs(bz, ref, dtype, shape, D, monkeypatch):
    m, n, p = shape
    A, b, x, y, mu, _ = real_inputs(m, n, p, n, dtype)
    Dd, Dr = sets(bz, ref, D, dtype)
    out = {}
    for kind in ("fused", "three", "dense"):
        monkeypatch.setenv("BZ_SPLS_FUSED", "0" if kind == "three" else "1")
        f = bz.LeastSquares(A, b) if kind == "dense" else sparse_ls(bz, A, b, seed=2)[0]
        out[kind], pr = one_gradient(bz, (f, bz.NormL1(1.0), bz.IdentityFunction(), Dd), n, n, dtype, mu, y, x)
        if kind != "dense":
            assert (pr["gemv"]["launches"], pr["al_gradient"]["launches"]) == ((2, 0) if kind == "fused" else (2, 1))
    al = ref.AugLagFun(ref.LeastSquares(A, b), ref.IdentityFunction(), Dr, mu.copy(), y.copy(), x)
    g_ref = np.empty(n, dtype)
    lx = float(al.gradient(g_ref, x))
    return out, g_ref, lx, 1e-12 if dtype == np.float64 else 2e-5, np.max(np.abs(g_ref))


GENERAL = TYPED + [(np.float32, c) for c in CUT32]


@pytest.mark.parametrize("D", ["zero", "box"])
@pytest.mark.parametrize("case", GENERAL, ids=IDS)
def test_general_gradient_against_oracle_and_dense_kind(bz, ref, case, D, monkeypatch):
    """random real data: the rule and the numbers of tests/test_gpu_sparse.py's test of the same name (1e-12 / 2e-5 of the
    gradient's largest entry; of max(1, |L|) for the value) — the same chain of two products — against the oracle and
    against the device's dense LeastSquares on the same matrix"""
    dtype, shape = case
    out, g_ref, lx, tol, scale = general_runs(bz, ref, dtype, shape, D, monkeypatch)
    g_dev, vals = out["fused"]
    print(f"max|g - g_ref| / max|g_ref| = {np.max(np.abs(g_dev.astype(np.float64) - g_ref)) / scale:.3e}, "
          f"vs dense kind {np.max(np.abs(g_dev.astype(np.float64) - out['dense'][0])) / scale:.3e}, "
          f"value {abs(vals[0] - lx) / max(1.0, abs(lx)):.3e}")
    assert np.max(np.abs(g_dev.astype(np.float64) - g_ref)) <= tol * scale
    assert abs(vals[0] - lx) <= tol * max(1.0, abs(lx))
    assert np.max(np.abs(g_dev.astype(np.float64) - out["dense"][0])) <= tol * scale
    assert abs(vals[0] - out["dense"][1][0]) <= tol * max(1.0, abs(lx))


@pytest.mark.parametrize("D", ["zero", "box"])
@pytest.mark.parametrize("case", GENERAL, ids=IDS)
def test_two_forms_give_the_same_gradient_bits(bz, ref, case, D, monkeypatch):
    """the same real data: the gradient under BZ_SPLS_FUSED=0 equals the default's BIT FOR BIT (the same row sums, the same
    element operations); the values differ in summation order only: inside the tolerance of the test above"""
    dtype, shape = case
    out, g_ref, lx, tol, scale = general_runs(bz, ref, dtype, shape, D, monkeypatch)
    (g_dev, vals), (g3, vals3) = out["fused"], out["three"]
    print(f"gradient equal {np.array_equal(g_dev, g3)}, scalars {vals} / {vals3}")
    assert np.array_equal(g_dev, g3)
    assert abs(vals[0] - vals3[0]) <= tol * max(1.0, abs(lx)) and abs(vals3[0] - lx) <= tol * max(1.0, abs(lx))
    assert vals[1] == vals3[1]                                          # (f comes from the first launch in both forms)


def test_pairwise_D_takes_the_three_launch_form(bz, ref):
    """XOR pairs, c = Identity, n even: the projection of an element needs its partner, so the gradient is k_spmv_ls_r, the
    plain product and k_algrad_elem whatever BZ_SPLS_FUSED says; within the tolerance of the general test"""
    m, n = 41, 120
    A, b, x, y, mu, _ = real_inputs(m, n, 0.1, n, np.float64)
    f = sparse_ls(bz, A, b)[0]
    (g_dev, vals), pr = one_gradient(bz, (f, bz.Zero(), bz.IdentityFunction(), bz.XorPairs()), n, n, np.float64, mu, y, x)
    assert pr["gemv"]["launches"] == 2 and pr["gemv"]["form"].startswith("k_spmv_ls_t<L=") and pr["al_gradient"]["launches"] == 1
    al = ref.AugLagFun(ref.LeastSquares(A, b), ref.IdentityFunction(), ref.PairwiseSet("xor"), mu.copy(), y.copy(), x)
    g_ref = np.empty(n)
    lx = float(al.gradient(g_ref, x))
    assert np.max(np.abs(g_dev - g_ref)) <= 1e-12 * np.max(np.abs(g_ref)) and abs(vals[0] - lx) <= 1e-12 * max(1.0, abs(lx))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_launches_of_two_gradients_and_identical_runs(bz, ref, dtype):
    """c = Identity, two gradients: four row launches and no k_algrad_elem launch; the same bits on both runs"""
    m, n = 257, 500
    A, b, x, y, mu, _ = real_inputs(m, n, 0.03, n, dtype)
    f, indptr, indices, nnz = sparse_ls(bz, A, b)
    runs, pr = one_gradient(bz, (f, bz.NormL1(1.0), bz.IdentityFunction(), bz.ZeroSet()), n, n, dtype, mu, y, x, times=2)
    assert pr["gemv"]["launches"] == 4 and pr["al_gradient"]["launches"] == 0 and pr["misc"]["launches"] == 0
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    # the bytes of the model: per pass both CSR arrays, the row pointers, one read of the gathered vector, and per row b and
    # r (A_f) / x, mu, mu*y and the gradient (A_f')
    sz = np.dtype(dtype).itemsize
    La, nva, _ = plan(indptr, nnz)
    Lt, nvt, _ = plan(transpose_ptr(indices, n), nnz)
    model = 2 * nnz * (sz + 4) + (nva + 1) * 8 + (nvt + 1) * 8 + (n + m) * sz + 2 * m * sz + 4 * n * sz
    assert pr["gemv"]["bytes"] == 2 * model, (pr["gemv"], model)


def beside_sparse_c(bz, ref, dtype, pair, integer):
    (m, n, pf), (ny, pc) = pair
    A, b, x, y, mu, rng = (integer_inputs if integer else real_inputs)(m, n, pf, ny, dtype)
    Ac = structured(ny, n, pc, rng, integer, dtype)
    bc = (rng.integers(-3, 4, ny) if integer else rng.standard_normal(ny)).astype(dtype)
    c_ptr, c_idx, c_val = csr_of(Ac, np.random.default_rng(3))
    f = sparse_ls(bz, A, b)[0]
    dev = (f, bz.NormL1(1.0), bz.SparseAffine(c_ptr, c_idx, c_val, bc, n), sets(bz, ref, "box", dtype)[0])
    runs, pr = one_gradient(bz, dev, n, ny, dtype, mu, y, x, times=2)

    def make_al(dt):
        al = ref.AugLagFun(ref.LeastSquares(A.astype(dt), b.astype(dt)), CsrOracle(c_ptr, c_idx, c_val.astype(dt), bc.astype(dt), n),
                           sets(bz, ref, "box", dt)[1], mu.astype(dt), y.astype(dt), x.astype(dt))
        g = np.empty(n, dt)
        return al, al.gradient(g, x.astype(dt)), g
    # two gradients: k_spmv_ls_r, k_spmv_ls_t, k_spmv_yupd, k_spmv_t_finish each, no element-wise kernel; the same bits
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
    tol = 1e-12 if dtype == np.float64 else 2e-5
    scale = np.max(np.abs(g_ref))
    print(f"max|g - g_ref| / max|g_ref| = {np.max(np.abs(g_dev.astype(np.float64) - g_ref)) / scale:.3e}, "
          f"value {abs(vals[0] - lx) / max(1.0, abs(lx)):.3e}")
    assert np.max(np.abs(g_dev.astype(np.float64) - g_ref)) <= tol * scale
    assert abs(vals[0] - lx) <= tol * max(1.0, abs(lx))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_exact_gradient_beside_a_sparse_c(bz, ref, dtype):
    """integer data beside c(x) = A_c x - b_c in CSR with another row count: bit for bit the oracle's"""
    (g_dev, vals), make_al, (A, b, x, y, Ac, bc) = beside_sparse_c(bz, ref, dtype, PAIRS[0], True)
    al, lx, g_ref = make_al(dtype)
    assert_exact_in(dtype, A, b, x, y, make_al, al, lx, g_ref, Ac, bc)
    assert g_dev.dtype == dtype and np.array_equal(g_dev, g_ref)
    assert vals[0] == float(lx) and vals[1] == float(al.fx)


def lasso(bz, ref, dtype, beside_c):
    """sparse_lasso(60, 128, 5): NormL1(0.1), c = Identity, D = box(-1, 1) ; or beside the constraints of budget_bands(128, 20)
    with g = IndBox(0, 1)"""
    m, n = 60, 128
    d = bz.synth.sparse_lasso(m, n, 5, dtype)
    f = bz.SparseLeastSquares(d["indptr"], d["indices"], d["data"], d["b"], n)
    fo = ref.LeastSquares(f.toarray(), d["b"])
    if not beside_c:
        dev = (f, bz.NormL1(0.1), bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(-1.0, 1.0)))
        orc = (fo, ref.NormL1(0.1), ref.IdentityFunction(), ref.ClosedSet(ref.IndBox(dtype(-1), dtype(1))))
        return n, n, dev, orc
    bb = bz.synth.budget_bands(n, 20, dtype)
    csr = (bb["indptr"], bb["indices"], bb["data"], bb["b"], n)
    dev = (f, bz.IndBox(0.0, 1.0), bz.SparseAffine(*csr), bz.ClosedSet(bz.IndBox(bb["lo"], bb["hi"])))
    orc = (fo, ref.IndBox(dtype(0), dtype(1)), CsrOracle(*csr), ref.ClosedSet(ref.IndBox(bb["lo"], bb["hi"])))
    return n, 21, dev, orc


@pytest.mark.parametrize("beside_c,dtype", [(False, np.float64), (False, np.float32), (True, np.float64)])
def test_iterates_follow_the_oracle(bz, ref, beside_c, dtype):
    """30 states: x and z inside max(base, 100 * sens) — base 1e-9 / 5e-5, sens the oracle's own extended-precision
    envelope — and gamma equal to 1e-12 / 1e-5 relative: the rule and the numbers of tests/test_gpu_sparse.py"""
    n, ny, dev, orc = lasso(bz, ref, dtype, beside_c)
    mu, y = np.full(ny, 0.1, dtype), (0.1 * np.random.default_rng(2).standard_normal(ny)).astype(dtype)
    x0 = np.zeros(n, dtype)
    eps = float(np.finfo(dtype).eps)
    prob, st, rows = run_traces(bz, ref, dev, orc, n, mu, y, x0, 30, minimum_gamma=eps, dtype=dtype, ny=ny)
    pr = prob.profile2()
    prob.close()
    base = 1e-9 if dtype == np.float64 else 5e-5
    for k, ex, ez, g_d, g_r, sn_d, sn_r, fused, sens in rows:
        print(f"k={k} ex={ex:.3e} ez={ez:.3e} gamma {g_d:.9g} / {g_r:.9g} sens={sens:.3e}")
    for k, ex, ez, g_d, g_r, sn_d, sn_r, fused, sens in rows:
        assert abs(g_d - g_r) <= (1e-12 if dtype == np.float64 else 1e-5) * g_r, k
        assert ex <= max(base, 100 * sens) and ez <= max(base, 100 * sens), (k, ex, ez, sens)
    assert pr["gemv"]["form"].startswith("k_spmv_"), pr["gemv"]["form"]
    assert pr["k_fused_iterates"]["launches"] == 0 and pr["k_fused_sep"]["launches"] == 0


@pytest.mark.parametrize("beside_c", [False, True])
def test_whole_solves(bz, ref, beside_c):
    """bz.alps, resident and through the host outer loop, against ref.alps: first_order on both sides, feasibility <= 1e-5,
    objective within 1e-4 relative, x within 1e-4 (the bounds of tests/test_gpu_sparse.py).  Iteration counts are printed."""
    n, ny, dev, orc = lasso(bz, ref, np.float64, beside_c)
    fo = orc[0]
    lo, hi = orc[3].f.lb, orc[3].f.ub
    obj = (lambda x: float(fo(x))) if beside_c else (lambda x: float(fo(x) + 0.1 * np.sum(np.abs(x))))

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


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_empty_matrix_is_half_the_norm_of_b(bz, ref, dtype):
    """nnz = 0 is accepted and behaves as f = 0.5||b||^2 with a zero gradient: bit for bit on integer data"""
    m, n = 23, 37
    rng = np.random.default_rng(8)
    b, x, y = (rng.integers(-3, 4, k).astype(dtype) for k in (m, n, n))
    mu = np.full(n, 0.25, dtype)
    f = bz.SparseLeastSquares(np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, dtype), b, n)
    Dd, Dr = sets(bz, ref, "box", dtype)
    (g_dev, vals), _ = one_gradient(bz, (f, bz.NormL1(1.0), bz.IdentityFunction(), Dd), n, n, dtype, mu, y, x)
    al = ref.AugLagFun(ref.LeastSquares(np.zeros((m, n), dtype), b), ref.IdentityFunction(), Dr, mu.copy(), y.copy(), x)
    g_ref = np.empty(n, dtype)
    lx = al.gradient(g_ref, x)
    assert np.array_equal(g_dev, g_ref) and np.array_equal(g_dev, al.yupd)
    assert vals[0] == float(lx) and vals[1] == 0.5 * float(np.dot(b.astype(np.float64), b))


def raw_desc(bz, indptr, indices, data, b, n, slack=0):
    from bazinga_jl_amd.oracles import lower
    m = b.shape[0]
    good = bz.SparseLeastSquares(np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), b, n)
    desc, keep = lower(good, bz.NormL1(1.0), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64)
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
    b, n = np.zeros(3), 4

    def create(desc, ctx=ctx):
        h = C.c_void_p()
        rc = lib.bz_problem_create(ctx._h, C.byref(desc), C.byref(h))
        msg = lib.bz_last_error().decode() if rc else ""
        if h.value:
            lib.bz_problem_destroy(h)
        return rc, bool(h.value), msg

    desc, keep = raw_desc(bz, indptr, indices, data, b, n)
    assert create(desc)[:2] == (0, True)
    for bad_ptr, row in ((np.array([0, 3, 2, 5]), "row 1"), (np.array([1, 2, 3, 5]), "row 0")):
        desc, keep = raw_desc(bz, bad_ptr, indices, data, b, n)
        rc, made, msg = create(desc)
        assert rc == L.BZ_ERR_ARG and not made and row in msg and "SparseLeastSquares" in msg, msg
    desc, keep = raw_desc(bz, np.array([0, 2, 3, 4]), indices, data, b, n)               # rowptr[m] != nnz
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_ARG and not made and "nnz" in msg and "row 2" in msg and "SparseLeastSquares" in msg, msg
    desc, keep = raw_desc(bz, indptr, np.array([0, 3, 1, 4, 3]), data, b, n)             # a column = n, in row 2
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_ARG and not made and "row 2" in msg and "SparseLeastSquares" in msg, msg
    desc, keep = raw_desc(bz, indptr, indices, data, b, n)
    desc.f_rows = 0
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_ARG and not made and "SparseLeastSquares" in msg, msg
    desc, keep = raw_desc(bz, indptr, indices, data, b, n)
    desc.f_b = None
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_ARG and not made and "SparseLeastSquares" in msg, msg
    # the four refusals
    desc, keep = raw_desc(bz, indptr, indices, data, b, n, slack=1)
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_UNSUPPORTED and not made and "slack" in msg and "SparseLeastSquares" in msg, msg
    desc, keep = raw_desc(bz, indptr, indices, data, b, n)
    A, b2 = np.ones((2, n)), np.zeros(2)
    desc.c_kind, desc.ny, desc.c_A, desc.c_b = L.BZ_C_DENSE_AFFINE, 2, A.ctypes.data, b2.ctypes.data
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_UNSUPPORTED and not made and "DenseAffine" in msg and "SparseLeastSquares" in msg, msg
    ctx2 = bz.Context(device=0, rank=0, nranks=2, comm_id=None)
    desc, keep = raw_desc(bz, indptr, indices, data, b, n)
    rc, made, msg = create(desc, ctx2)
    assert rc == L.BZ_ERR_UNSUPPORTED and not made and "one rank" in msg and "SparseLeastSquares" in msg, msg
    desc, keep = raw_desc(bz, indptr, indices, data, b, n)
    desc.g_kind = L.BZ_G_CALLBACK
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_UNSUPPORTED and not made and "callbacks" in msg and "SparseLeastSquares" in msg, msg
    # the Python layer raises before any device call
    f = bz.SparseLeastSquares(indptr, indices, data, b, n)
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(f, bz.NormL1(1.0), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64, slack=True)
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(f, bz.NormL1(1.0), bz.DenseAffine(A, np.zeros(2)), bz.ZeroSet(), n, 2, np.float64)
