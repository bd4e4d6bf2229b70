"""f(x) = 0.5 x'Qx + q'x with a sparse symmetric Q in CSR on the device (BZ_F_SPARSE_QUADRATIC): the row kernels over Q
(k_spmv_q_algrad, the whole AL gradient of c = Identity in one launch; k_spmv_q, the product for the two-launch form and
beside a sparse c), the iterates and whole solves against the oracle, creation-time validation and the byte accounting.

The oracle is ref.Quadratic on the densified matrix throughout."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_parity import run_traces
from tests.test_gpu_sparse import CsrOracle, csr_of, plan, sets, structured, transpose_ptr
from tests.test_sparse_quadratic_host import CASES, LANES, sym_structured

pytestmark = pytest.mark.gpu

IDS = lambda c: f"{'f64' if c[0] == np.float64 else 'f32'}-{c[1][0]}-{c[1][1]}"
# a sparse c beside the sparse f: (ny, n, density of A) with the case of Q on the same n
PAIRS = [((41, 121, 0.1), (121, 0.05)), ((257, 1031, 0.9), (1031, 0.012))]


def sparse_q(bz, Q, q, seed=1):
    indptr, indices, data = csr_of(Q, np.random.default_rng(seed))
    return bz.SparseQuadratic(indptr, indices, data, q), indptr, data.shape[0]


def integer_data(n, ny, dtype, rng):
    """integer q, y in [-3, 3], x in [-2, 2], mu = 1/4"""
    return (rng.integers(-3, 4, n).astype(dtype), rng.integers(-2, 3, n).astype(dtype), rng.integers(-3, 4, ny).astype(dtype),
            np.full(ny, 0.25, dtype))


def assert_exact_in(dtype, Q, q, x, y, make_al, al, lx, g_ref, absA=None, b=None):
    """Exactness, whatever the order of any sum, asserted on the oracle's float64 recomputation (make_al(np.float64)):
    - every vector entry and every row sum lives in dtype: the sums of magnitudes, in units of the entry's granularity,
      stay below 2^24 (fp32) / 2^53 (fp64);
    - the scalars: the device accumulates their partials in double whatever dtype is, so the sum of magnitudes in units of
      the finest granularity (1/8: mu y^2 / 2) has to stay below 2^53; dtype then holds the totals and the three steps of
      L = 0.5 pen + f - mu/2 |y|^2 (the oracle's association and the library's), each of which must be a number of dtype.
      c = Identity: the sum of magnitudes stays below 2^24 too (fp32), so that not even a partial sum in fp32 could round.
    - the fp32 oracle itself (numpy sums in fp32) has returned the float64 values."""
    lim = 2.0 ** (24 if dtype == np.float32 else 53)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    d = np.abs(Q.astype(np.float64)) @ np.abs(x64)
    al64, lx64, g64 = make_al(np.float64)
    yhat = al64.yupd
    t = yhat * 0.25
    assert 2 * np.max(d + np.abs(q)) < lim                              # 0.5 (Qx)_i + q_i, in halves
    assert 2 * np.max(np.abs(x64) * (0.5 * d + np.abs(q))) < lim and 4 * np.max(t * t / 0.25) < lim
    fsum = np.sum(np.abs(x64) * (0.5 * d + np.abs(q)))
    total = 8 * (fsum + np.sum(t * t / 0.25) + np.sum(0.25 * y64 ** 2))
    assert total < 2.0 ** 53 and (absA is not None or total < lim)
    if absA is not None:
        assert np.max(absA @ np.abs(x64) + np.abs(b)) * 4 < lim
        assert np.max(absA.T @ np.abs(yhat)) + np.max(d + np.abs(q)) < lim
    assert np.max(np.abs(g64)) < 2.0 ** 20
    fx64, musqy64 = float(al64.fx), float(al64.musqy)
    half_pen = float(lx64) + musqy64 - fx64                             # (exact in float64: the bound above)
    for v in (2 * half_pen, half_pen, half_pen + fx64, float(lx64), fx64, musqy64):
        assert float(dtype(v)) == v, v
    assert float(lx) == float(lx64) and float(al.fx) == fx64 and np.array_equal(g_ref.astype(np.float64), g64)


def exact_identity(bz, ref, dtype, n, p, D_name):
    Q = sym_structured(n, p, True, dtype)
    rng = np.random.default_rng(n * 13 + 5)
    q, x, y, mu = integer_data(n, n, dtype, rng)
    f, indptr, nnz = sparse_q(bz, Q, q)
    Dd = sets(bz, ref, D_name, dtype)[0]
    prob = bz.Problem(f, bz.NormL1(1.0), bz.IdentityFunction(), Dd, n, n, dtype)
    prob.set_multipliers(mu, y)
    prob.profile_enable(True)
    g_dev, vals = prob.eval_al_gradient(x)
    pr = prob.profile2()
    prob.close()

    def make_al(dt):
        D = sets(bz, ref, D_name, dt)[1]
        al = ref.AugLagFun(ref.Quadratic(Q.astype(dt), q.astype(dt)), ref.IdentityFunction(), D, mu.astype(dt), y.astype(dt), x.astype(dt))
        g = np.empty(n, dt)
        return al, al.gradient(g, x.astype(dt)), g
    al, lx, g_ref = make_al(dtype)
    assert_exact_in(dtype, Q, q, x, y, make_al, al, lx, g_ref)
    assert g_dev.dtype == dtype and np.array_equal(g_dev, g_ref)
    assert vals[0] == float(lx) and vals[1] == float(al.fx)
    return pr, plan(indptr, nnz)


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("D", ["zero", "free", "box"])
@pytest.mark.parametrize("case", [(t, c) for t in (np.float64, np.float32) for c in CASES], ids=IDS)
def test_exact_gradient_bit_for_bit(bz, ref, case, D, fused, monkeypatch):
    """Integer data, mu = 1/4: every product and every sum is exact in the number format, so no summation order can change
    a bit: gradient and value equal the oracle's BIT FOR BIT, in the one-launch form and in the two-launch form."""
    dtype, (n, p) = case
    monkeypatch.setenv("BZ_SPQ_FUSED", str(fused))
    pr, (L, nv, seg) = exact_identity(bz, ref, dtype, n, p, D)
    assert L == LANES[CASES.index((n, p))]
    kernel = "k_spmv_q_algrad" if fused else "k_spmv_q"
    assert pr["gemv"]["form"] == f"{kernel}<L={L},SEG={int(seg)}>", pr["gemv"]["form"]
    assert pr["gemv"]["launches"] == 1 and pr["al_gradient"]["launches"] == 1 - fused


@pytest.mark.parametrize("lanes", [1, 64])
@pytest.mark.parametrize("case", [(t, c) for t in (np.float64, np.float32) for c in ((70, 0.03), (1031, 0.012))], ids=IDS)
def test_exact_gradient_with_forced_lane_counts(bz, ref, case, lanes, monkeypatch):
    dtype, (n, p) = case
    monkeypatch.setenv("BZ_SPMV_L", str(lanes))
    for D in ("zero", "free", "box"):
        pr, (L, nv, seg) = exact_identity(bz, ref, dtype, n, p, D)
        assert pr["gemv"]["form"] == f"k_spmv_q_algrad<L={lanes},SEG={int(seg)}>", pr["gemv"]["form"]


@pytest.mark.parametrize("D", ["zero", "free", "box"])
@pytest.mark.parametrize("case", [(t, c) for t in (np.float64, np.float32) for c in PAIRS],
                         ids=lambda c: f"{'f64' if c[0] == np.float64 else 'f32'}-{c[1][0][0]}x{c[1][0][1]}")
def test_exact_gradient_beside_a_sparse_c(bz, ref, case, D):
    """the same integer data with c(x) = A x - b in CSR: three row launches (Q, A, A'), bit for bit the oracle's.  (At
    257 x 1031 the penalty sum passes 2^24 quarter units: in fp32 the totals are exact because the device's partials are
    doubles and the totals are numbers of fp32 — assert_exact_in checks both, and that numpy's own fp32 sums were exact.)"""
    dtype, ((ny, n, pa), (nq, pq)) = case
    assert nq == n
    rng = np.random.default_rng(ny * 7 + n)
    A = structured(ny, n, pa, rng, True, dtype)
    a_ptr, a_idx, a_val = csr_of(A, np.random.default_rng(1))
    b = rng.integers(-3, 4, ny).astype(dtype)
    Q = sym_structured(n, pq, True, dtype)
    q, x, y, mu = integer_data(n, ny, dtype, rng)
    f, indptr, nnz = sparse_q(bz, Q, q)
    Dd, Dr = sets(bz, ref, D, dtype)
    prob = bz.Problem(f, bz.NormL1(1.0), bz.SparseAffine(a_ptr, a_idx, a_val, b, n), Dd, n, ny, dtype)
    prob.set_multipliers(mu, y)
    prob.profile_enable(True)
    g_dev, vals = prob.eval_al_gradient(x)
    pr = prob.profile2()
    prob.close()

    def make_al(dt):
        al = ref.AugLagFun(ref.Quadratic(Q.astype(dt), q.astype(dt)), CsrOracle(a_ptr, a_idx, a_val.astype(dt), b.astype(dt), n),
                           sets(bz, ref, D, dt)[1], mu.astype(dt), y.astype(dt), x.astype(dt))
        g = np.empty(n, dt)
        return al, al.gradient(g, x.astype(dt)), g
    al, lx, g_ref = make_al(dtype)
    assert_exact_in(dtype, Q, q, x, y, make_al, al, lx, g_ref, np.abs(A.astype(np.float64)), b)
    assert pr["gemv"]["launches"] == 3 and pr["al_gradient"]["launches"] == 0
    Lt, _, seg_t = plan(transpose_ptr(a_idx, n), a_val.shape[0])
    assert pr["gemv"]["form"] == f"k_spmv_t_finish<L={Lt},SEG={int(seg_t)}>", pr["gemv"]["form"]
    assert g_dev.dtype == dtype and np.array_equal(g_dev, g_ref)
    assert vals[0] == float(lx) and vals[1] == float(al.fx)


def real_data(n, ny, dtype, rng):
    return (rng.standard_normal(n).astype(dtype), rng.standard_normal(n).astype(dtype), rng.standard_normal(ny).astype(dtype),
            (10.0 ** rng.uniform(-2, 0, ny)).astype(dtype))


@pytest.mark.parametrize("D", ["zero", "box"])
@pytest.mark.parametrize("case", [(t, c) for t in (np.float64, np.float32) for c in CASES], ids=IDS)
def test_general_gradient_against_oracle_and_dense_kind(bz, ref, case, D, monkeypatch):
    """random real data: the tolerances of tests/test_gpu_sparse.py's test of the same name for order-dependent row sums
    (1e-12 / 2e-5 of the gradient's largest entry; of max(1, |L|) for the value), against the oracle and against the
    device's dense Quadratic on the densified matrix.  Two runs of the one-launch form give the same bits."""
    dtype, (n, p) = case
    g_dev, vals, out, g_ref, lx, tol, scale = general_runs(bz, ref, dtype, n, p, D, monkeypatch)
    print(f"max|g - g_ref| / max|g_ref| = {np.max(np.abs(g_dev.astype(np.float64) - g_ref)) / scale:.3e}, "
          f"vs dense kind {np.max(np.abs(g_dev.astype(np.float64) - out['dense'][0])) / scale:.3e}, "
          f"value {abs(vals[0] - lx) / max(1.0, abs(lx)):.3e}")
    assert np.max(np.abs(g_dev.astype(np.float64) - g_ref)) <= tol * scale
    assert abs(vals[0] - lx) <= tol * max(1.0, abs(lx))
    assert np.max(np.abs(g_dev.astype(np.float64) - out["dense"][0])) <= tol * scale
    assert abs(vals[0] - out["dense"][1][0]) <= tol * max(1.0, abs(lx))
    assert np.array_equal(g_dev, out["fused2"][0]) and vals == out["fused2"][1]


@pytest.mark.parametrize("D", ["zero", "box"])
@pytest.mark.parametrize("case", [(t, c) for t in (np.float64, np.float32) for c in CASES], ids=IDS)
def test_one_launch_and_two_launch_forms_agree_bit_for_bit(bz, ref, case, D, monkeypatch):
    """The same real data: the one-launch form and BZ_SPQ_FUSED=0 give the same gradient and the same two scalars BIT FOR
    BIT, in fp64 too, where a sum depends on its order: k_spmv_q_algrad runs on k_algrad_elem's grid and adds the element
    terms in k_algrad_elem's order (a row's terms go through LDS to the thread that owns the row's pack)."""
    dtype, (n, p) = case
    g_dev, vals, out, g_ref, lx, tol, scale = general_runs(bz, ref, dtype, n, p, D, monkeypatch)
    print(f"gradient equal {np.array_equal(g_dev, out['two'][0])}, scalars {vals} / {out['two'][1]}")
    assert np.array_equal(g_dev, out["two"][0])
    assert vals == out["two"][1]


def general_runs(bz, ref, dtype, n, p, D, monkeypatch):
    Q = sym_structured(n, p, False, dtype, np.random.default_rng(n * 11 + int(p * 1000)))
    rng = np.random.default_rng(n * 17 + 3)
    q, x, y, mu = real_data(n, n, dtype, rng)
    Dd, Dr = sets(bz, ref, D, dtype)
    out = {}
    for kind in ("fused", "fused2", "two", "dense"):
        monkeypatch.setenv("BZ_SPQ_FUSED", "0" if kind == "two" else "1")
        f = bz.Quadratic(Q, q) if kind == "dense" else sparse_q(bz, Q, q, seed=2)[0]
        prob = bz.Problem(f, bz.NormL1(1.0), bz.IdentityFunction(), Dd, n, n, dtype)
        prob.set_multipliers(mu, y)
        out[kind] = prob.eval_al_gradient(x)
        prob.close()
    al = ref.AugLagFun(ref.Quadratic(Q, q), ref.IdentityFunction(), Dr, mu.copy(), y.copy(), x)
    g_ref = np.empty(n, dtype)
    lx = float(al.gradient(g_ref, x))
    tol = 1e-12 if dtype == np.float64 else 2e-5
    g_dev, vals = out["fused"]
    return g_dev, vals, out, g_ref, lx, tol, np.max(np.abs(g_ref))


@pytest.mark.parametrize("case", [(t, c) for t in (np.float64, np.float32) for c in PAIRS],
                         ids=lambda c: f"{'f64' if c[0] == np.float64 else 'f32'}-{c[1][0][0]}x{c[1][0][1]}")
def test_general_gradient_beside_a_sparse_c(bz, ref, case):
    dtype, ((ny, n, pa), (nq, pq)) = case
    rng = np.random.default_rng(ny * 11 + n)
    A = structured(ny, n, pa, rng, False, dtype)
    a_ptr, a_idx, a_val = csr_of(A, np.random.default_rng(2))
    b = rng.standard_normal(ny).astype(dtype)
    Q = sym_structured(n, pq, False, dtype, np.random.default_rng(n * 11 + int(pq * 1000)))
    q, x, y, mu = real_data(n, ny, dtype, rng)
    Dd, Dr = sets(bz, ref, "box", dtype)
    runs = []
    for _ in range(2):
        prob = bz.Problem(sparse_q(bz, Q, q, seed=2)[0], bz.NormL1(1.0), bz.SparseAffine(a_ptr, a_idx, a_val, b, n), Dd, n, ny, dtype)
        prob.set_multipliers(mu, y)
        runs.append(prob.eval_al_gradient(x))
        prob.close()
    al = ref.AugLagFun(ref.Quadratic(Q, q), CsrOracle(a_ptr, a_idx, a_val, b, n), Dr, mu.copy(), y.copy(), x)
    g_ref = np.empty(n, dtype)
    lx = float(al.gradient(g_ref, x))
    tol = 1e-12 if dtype == np.float64 else 2e-5
    g_dev, vals = runs[0]
    scale = np.max(np.abs(g_ref))
    print(f"max|g - g_ref| / max|g_ref| = {np.max(np.abs(g_dev.astype(np.float64) - g_ref)) / scale:.3e}, "
          f"value {abs(vals[0] - lx) / max(1.0, abs(lx)):.3e}")
    assert np.max(np.abs(g_dev.astype(np.float64) - g_ref)) <= tol * scale
    assert abs(vals[0] - lx) <= tol * max(1.0, abs(lx))
    assert np.array_equal(g_dev, runs[1][0]) and vals == runs[1][1]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [(257, 0.1, "zero"), (1031, 0.9, "vecbox")])
def test_launches_and_bytes_of_one_gradient(bz, ref, shape, dtype, monkeypatch):
    """c = Identity: one AL gradient = ONE k_spmv_q_algrad launch (a cut matrix too: its cut rows are folded inside) and no
    element-wise kernel, moving both CSR arrays, the (virtual) row pointers, the virtual-row tables of a cut matrix, one
    gathered read of x, and per row x, q, mu, mu*y (the vector bounds of D) and the gradient.  BZ_SPQ_FUSED=0: the product
    and k_algrad_elem.  Beside a sparse c: three row launches."""
    n, p, D = shape
    rng = np.random.default_rng(3)
    Q = sym_structured(n, p, False, dtype, rng)
    q, x, y, _ = real_data(n, n, dtype, rng)
    sz = np.dtype(dtype).itemsize
    Dd = bz.ZeroSet() if D == "zero" else bz.ClosedSet(bz.IndBox(np.full(n, -1.0, dtype), np.full(n, 2.0, dtype)))

    def one_gradient(c, ny):
        f, indptr, nnz = sparse_q(bz, Q, q, seed=2)
        prob = bz.Problem(f, bz.NormL1(1.0), c, Dd if ny == n else bz.ZeroSet(), n, ny, dtype)
        prob.set_multipliers(np.full(ny, 0.5, dtype), y[:ny])
        prob.profile_reset()
        prob.profile_enable(True)
        prob.eval_al_gradient(x)
        pr = prob.profile2()
        prob.close()
        return pr, indptr, nnz

    pr, indptr, nnz = one_gradient(bz.IdentityFunction(), n)
    L, nv, seg = plan(indptr, nnz)
    assert seg == (n == 1031)
    model = nnz * (sz + 4) + (nv + 1) * 8 + (nv * 8 if seg else 0) + n * sz      # the matrix and one gathered read of x
    model += (5 + (2 if D == "vecbox" else 0)) * n * sz                          # x, q, mu, mu*y (the bounds of D), the gradient
    assert pr["gemv"]["launches"] == 1 and pr["gemv"]["bytes"] == model, (pr["gemv"], model)
    assert pr["gemv"]["form"] == f"k_spmv_q_algrad<L={L},SEG={int(seg)}>"
    assert pr["al_gradient"]["launches"] == 0 and pr["misc"]["launches"] == 0      # (a cut Q: no fold launch either)
    monkeypatch.setenv("BZ_SPQ_FUSED", "0")
    pr = one_gradient(bz.IdentityFunction(), n)[0]
    assert pr["gemv"]["launches"] == 1 and pr["al_gradient"]["launches"] == 1
    assert pr["gemv"]["form"] == f"k_spmv_q<L={L},SEG={int(seg)}>"
    monkeypatch.delenv("BZ_SPQ_FUSED")
    ny = 41
    A = structured(ny, n, 0.1, rng, False, dtype)
    a_ptr, a_idx, a_val = csr_of(A, np.random.default_rng(2))
    pr = one_gradient(bz.SparseAffine(a_ptr, a_idx, a_val, np.zeros(ny, dtype), n), ny)[0]
    assert pr["gemv"]["launches"] == 3 and pr["al_gradient"]["launches"] == 0


def trace_problem(bz, ref, which, dtype):
    if which in ("laplacian", "stencil"):
        nx, ny = 12, 20
        n = nx * ny
        lap = bz.synth.laplacian_2d(nx, ny, dtype)
        b = np.random.default_rng(4).standard_normal(n).astype(dtype)
        f = bz.SparseQuadratic(lap["indptr"], lap["indices"], lap["data"], -b)
        fd = f if which == "laplacian" else bz.Stencil5ptQuadratic(nx, ny, b)
        dev = (fd, bz.NormL1(0.1), bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(-0.5, 0.5)))
        orc = (ref.Quadratic(f.toarray(), -b), ref.NormL1(0.1), ref.IdentityFunction(), ref.ClosedSet(ref.IndBox(dtype(-0.5), dtype(0.5))))
        return n, n, dev, orc
    if which == "sparse_qp":
        n, m = 300, 100
        d = bz.synth.sparse_qp(n, m, dtype=dtype)
        f = bz.SparseQuadratic(d["Q_indptr"], d["Q_indices"], d["Q_data"], d["fq"])
        csr = (d["indptr"], d["indices"], d["data"], d["b"], n)
        dev = (f, bz.IndBox(0.0, 1.0), bz.SparseAffine(*csr), bz.ClosedSet(bz.IndBox(d["lo"], d["hi"])))
        orc = (ref.Quadratic(f.toarray(), d["fq"]), ref.IndBox(dtype(0), dtype(1)), CsrOracle(*csr), ref.ClosedSet(ref.IndBox(d["lo"], d["hi"])))
        return n, m + 1, dev, orc
    n = 120                                                             # nonconvex: an indefinite symmetric Q
    rng = np.random.default_rng(9)
    Q = sym_structured(n, 0.1, False, dtype, rng)
    ev = np.linalg.eigvalsh(Q.astype(np.float64))
    assert ev[0] < -0.1 and ev[-1] > 0.1
    q = rng.standard_normal(n).astype(dtype)
    dev = (sparse_q(bz, Q, q)[0], bz.IndBox(-1.0, 1.0), bz.IdentityFunction(), bz.FreeSet())
    orc = (ref.Quadratic(Q, q), ref.IndBox(dtype(-1), dtype(1)), ref.IdentityFunction(), ref.FreeSet())
    return n, n, dev, orc


@pytest.mark.parametrize("which,dtype", [("laplacian", np.float64), ("laplacian", np.float32), ("stencil", np.float64),
                                         ("stencil", np.float32), ("sparse_qp", np.float64), ("nonconvex", np.float64)])
def test_iterates_follow_the_oracle(bz, ref, which, dtype):
    """30 states: x and z inside max(base, 100 * sens) — base 1e-9 / 5e-5, sens the oracle's own extended-precision
    envelope — and gamma equal to 1e-12 / 1e-5 relative: the rule and the numbers of tests/test_gpu_sparse.py.
    ("stencil": the Laplacian problem with bz.Stencil5ptQuadratic on the device, against the same oracle.)"""
    n, ny, dev, orc = trace_problem(bz, ref, which, dtype)
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
    if which != "stencil":
        assert pr["gemv"]["form"].startswith("k_spmv_"), pr["gemv"]["form"]
        assert pr["k_fused_iterates"]["launches"] == 0 and pr["k_fused_sep"]["launches"] == 0


def check_solves(bz, ref, dev, orc, n, ny, obj, feas_of, label):
    sub = lambda **kw: bz.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
    subr = lambda **kw: ref.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
    o = ref.alps(*orc, np.zeros(n), np.zeros(ny), subsolver=subr, subsolver_maxit=100000)
    assert o[5] == "first_order"
    for resident in (True, False):
        a = bz.alps(*dev, np.zeros(n), np.zeros(ny), subsolver=sub, subsolver_maxit=100000, resident=resident)
        feas = feas_of(a[0])
        print(f"{label} resident={resident}: status {a[5]} outer {a[2]}/{o[2]} inner {a[3]}/{o[3]} feas {feas:.3e} "
              f"obj {obj(a[0]):.9g}/{obj(o[0]):.9g} max|x - x_ref| {np.max(np.abs(a[0] - o[0])):.3e}")
        assert a[5] == "first_order"
        assert feas <= 1e-5
        assert abs(obj(a[0]) - obj(o[0])) <= 1e-4 * abs(obj(o[0]))
        assert np.max(np.abs(a[0] - o[0])) <= 1e-4


@pytest.mark.parametrize("which", ["laplacian", "sparse_qp"])
def test_whole_solves(bz, ref, which):
    """bz.alps, resident and through the host outer loop, against ref.alps: first_order on both sides, feasibility <= 1e-5,
    objective within 1e-4 relative, x within 1e-4 (the bounds of tests/test_gpu_sparse.py).  Iteration counts are printed."""
    n, ny, dev, orc = trace_problem(bz, ref, which, np.float64)
    fo = orc[0]
    if which == "laplacian":
        obj = lambda x: float(fo(x) + 0.1 * np.sum(np.abs(x)))
        feas_of = lambda x: float(np.max(np.abs(x - np.clip(x, -0.5, 0.5))))
    else:
        lo, hi = orc[3].f.lb, orc[3].f.ub
        obj = lambda x: float(fo(x))

        def feas_of(x):
            cx = np.empty(ny)
            orc[2].eval(cx, x)
            return float(np.max(np.abs(cx - np.clip(cx, lo, hi))))
    check_solves(bz, ref, dev, orc, n, ny, obj, feas_of, which)


def test_pairwise_D_takes_the_two_launch_form(bz, ref):
    """XOR pairs, c = Identity, n = 64: the projection of an element needs its partner, so the gradient is the product and
    k_algrad_elem whatever BZ_SPQ_FUSED says; the whole solve stays within test_whole_solves' bounds against the oracle"""
    n = 64
    d = bz.synth.sparse_qp(n, 8)
    f = bz.SparseQuadratic(d["Q_indptr"], d["Q_indices"], d["Q_data"], d["fq"])
    dev = (f, bz.Zero(), bz.IdentityFunction(), bz.XorPairs())
    orc = (ref.Quadratic(f.toarray(), d["fq"]), ref.Zero(), ref.IdentityFunction(), ref.PairwiseSet("xor"))
    prob = bz.Problem(*dev, n, n, np.float64)
    rng = np.random.default_rng(6)
    mu, y, x = 10.0 ** rng.uniform(-2, 0, n), rng.standard_normal(n), rng.standard_normal(n)
    prob.set_multipliers(mu, y)
    prob.profile_enable(True)
    g_dev, vals = prob.eval_al_gradient(x)
    pr = prob.profile2()
    prob.close()
    assert pr["gemv"]["launches"] == 1 and pr["gemv"]["form"].startswith("k_spmv_q<L=") and pr["al_gradient"]["launches"] == 1
    al = ref.AugLagFun(orc[0], orc[2], orc[3], mu.copy(), y.copy(), x)
    g_ref = np.empty(n)
    lx = float(al.gradient(g_ref, x))
    assert np.max(np.abs(g_dev - g_ref)) <= 1e-12 * np.max(np.abs(g_ref)) and abs(vals[0] - lx) <= 1e-12 * max(1.0, abs(lx))

    def feas_of(x):
        z = np.empty(n)
        orc[3].proj(z, x)
        return float(np.max(np.abs(z - x)))
    check_solves(bz, ref, dev, orc, n, n, lambda x: float(orc[0](x)), feas_of, "xor pairs")


def raw_desc(bz, indptr, indices, data, n, slack=0, c=None, ny=None):
    from bazinga_jl_amd.oracles import lower
    good = bz.SparseQuadratic(np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), np.zeros(n))
    ny = n if ny is None else ny
    desc, keep = lower(good, bz.NormL1(1.0), bz.IdentityFunction() if c is None else c, bz.ZeroSet(), n, ny, np.float64)
    arrs = (np.ascontiguousarray(indptr, np.int64), np.ascontiguousarray(indices, np.int32), np.ascontiguousarray(data, np.float64))
    desc.f_sp_rowptr, desc.f_sp_col, desc.f_sp_val = (a.ctypes.data for a in arrs)
    desc.f_sp_nnz = arrs[1].shape[0]
    desc.slack = slack
    return desc, (keep, arrs)


def test_creation_validates_the_matrix_and_refuses_what_is_not_lowered(bz, ref):
    L = bz._lib
    lib = L.load()
    ctx = bz.default_context()
    indptr, indices, data, n = np.array([0, 2, 3, 5]), np.array([0, 2, 1, 0, 2]), np.array([1.0, 5.0, 2.0, 5.0, 3.0]), 3

    def create(desc, ctx=ctx):
        h = C.c_void_p()
        rc = lib.bz_problem_create(ctx._h, C.byref(desc), C.byref(h))
        msg = lib.bz_last_error().decode() if rc else ""
        if h.value:
            lib.bz_problem_destroy(h)
        return rc, bool(h.value), msg

    desc, keep = raw_desc(bz, indptr, indices, data, n)
    assert create(desc)[:2] == (0, True)
    for bad_ptr, row in ((np.array([0, 3, 2, 5]), "row 1"), (np.array([1, 2, 3, 5]), "row 0")):
        desc, keep = raw_desc(bz, bad_ptr, indices, data, n)
        rc, made, msg = create(desc)
        assert rc == L.BZ_ERR_ARG and not made and row in msg and "SparseQuadratic" in msg, msg
    desc, keep = raw_desc(bz, np.array([0, 2, 3, 4]), indices, data, n)                 # rowptr[n] != nnz
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_ARG and not made and "nnz" in msg and "row 2" in msg and "SparseQuadratic" in msg, msg
    desc, keep = raw_desc(bz, indptr, np.array([0, 2, 3, 0, 2]), data, n)               # a column = n, in row 1
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_ARG and not made and "row 1" in msg and "SparseQuadratic" in msg, msg
    desc, keep = raw_desc(bz, indptr, indices, data, n, slack=1)
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_UNSUPPORTED and not made and "slack" in msg and "SparseQuadratic" in msg, msg
    desc, keep = raw_desc(bz, indptr, indices, data, n)
    A, b2 = np.ones((2, n)), np.zeros(2)
    desc.c_kind, desc.ny, desc.c_A, desc.c_b = L.BZ_C_DENSE_AFFINE, 2, A.ctypes.data, b2.ctypes.data
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_UNSUPPORTED and not made and "DenseAffine" in msg and "SparseQuadratic" in msg, msg
    ctx2 = bz.Context(device=0, rank=0, nranks=2, comm_id=None)
    desc, keep = raw_desc(bz, indptr, indices, data, n)
    rc, made, msg = create(desc, ctx2)
    assert rc == L.BZ_ERR_UNSUPPORTED and not made and "one rank" in msg and "SparseQuadratic" in msg, msg
    # the Python layer raises before any device call
    f = bz.SparseQuadratic(indptr, indices, data, np.zeros(n))
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(f, bz.NormL1(1.0), bz.IdentityFunction(), bz.ZeroSet(), n, n, np.float64, slack=True)
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(f, bz.NormL1(1.0), bz.DenseAffine(A, np.zeros(2)), bz.ZeroSet(), n, 2, np.float64)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_empty_matrix_is_the_linear_cost(bz, ref, dtype):
    """nnz = 0 is accepted and behaves as f(x) = q'x: bit for bit on integer data"""
    n = 37
    rng = np.random.default_rng(8)
    q, x, y, mu = integer_data(n, n, dtype, rng)
    f = bz.SparseQuadratic(np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, dtype), q)
    Dd, Dr = sets(bz, ref, "box", dtype)
    prob = bz.Problem(f, bz.NormL1(1.0), bz.IdentityFunction(), Dd, n, n, dtype)
    prob.set_multipliers(mu, y)
    g_dev, vals = prob.eval_al_gradient(x)
    prob.close()
    al = ref.AugLagFun(ref.Quadratic(np.zeros((n, n), dtype), q), ref.IdentityFunction(), Dr, mu.copy(), y.copy(), x)
    g_ref = np.empty(n, dtype)
    lx = al.gradient(g_ref, x)
    assert np.array_equal(g_dev, g_ref) and vals[0] == float(lx) and vals[1] == float(np.dot(q, x))
