"""c(x) = A x - b with A in CSR on the device (BZ_C_SPARSE_AFFINE; the constraint shape of demo/obstacle.jl:93-113): the
two row kernels of its AL gradient (k_spmv_yupd over A, k_spmv_t_finish over A'), the cut of long rows, the iterates and
whole solves against the oracle, creation-time validation and the byte accounting.

The oracle duck-types c: it gets a small class of this file with eval! / jtprod! over the same CSR arrays (or
ref.DenseAffine of the densified matrix where the test says so)."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_parity import _err, make_cfg4, rel, run_traces

pytestmark = pytest.mark.gpu


class CsrOracle:
    """eval!(cx, c, x) = A x - b, jtprod!(jtv, c, x, v) = A'v over CSR arrays, in the arrays' stored order"""

    def __init__(self, indptr, indices, data, b, n):
        self.indices, self.data, self.b, self.n = np.asarray(indices), np.asarray(data), np.asarray(b), n
        self.ny = self.b.shape[0]
        self.rows = np.repeat(np.arange(self.ny), np.diff(indptr))

    def eval(self, cx, x):
        cx[...] = np.bincount(self.rows, weights=self.data * x[self.indices], minlength=self.ny) - self.b

    def jtprod(self, jtv, x, v):
        jtv[...] = np.bincount(self.indices, weights=self.data * v[self.rows], minlength=self.n)


def csr_of(A, rng):
    """CSR of a dense matrix with the entries of every row in a shuffled (unsorted) order"""
    ny, n = A.shape
    indptr, indices, data = [0], [], []
    for r in range(ny):
        cols = rng.permutation(np.nonzero(A[r])[0])
        indices.append(cols)
        data.append(A[r, cols])
        indptr.append(indptr[-1] + cols.shape[0])
    return (np.array(indptr, np.int64), np.concatenate(indices).astype(np.int32),
            np.concatenate(data).astype(A.dtype))


def structured(ny, n, p, rng, integer, dtype):
    """density-p matrix with a full row (0), a full column (0), an empty row (1) and an empty column (1)"""
    if integer:
        A = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), (ny, n))
    else:
        A = rng.standard_normal((ny, n)) / np.sqrt(max(1.0, p * n))
    A = A * (rng.random((ny, n)) < p)
    full_r = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), n) if integer else rng.standard_normal(n) / np.sqrt(n)
    full_c = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), ny) if integer else rng.standard_normal(ny) / np.sqrt(ny)
    A[0, :] = full_r
    A[:, 0] = full_c
    if ny > 2:
        A[1, :] = 0
    if n > 2:
        A[:, 1] = 0
    return A.astype(dtype)


# ---- DESIGN 4's plan rules, restated: segment length, lanes per row
def plan(indptr, nnz):
    S = max(512, ((nnz // (2048 * 4) // 4 + 63) // 64) * 64)
    lens = np.diff(indptr)
    segs = np.where(lens > S, -(-lens // S), 1)
    nv = int(segs.sum())
    mean = nnz / nv if nv else 0.0
    L = 1
    while L < 64 and mean > 4.0 * L:
        L *= 2
    return L, nv, bool(np.any(lens > S))


def transpose_ptr(indices, n):
    return np.concatenate(([0], np.cumsum(np.bincount(indices, minlength=n)))).astype(np.int64)


# (ny, n, density): not multiples of the pack width; between them L = 1 .. 64 on A and on A', and (257 x 1031 at 0.9)
# rows beyond the segment length
CASES64 = [(120, 40, 0.02), (40, 120, 0.02), (3, 70, 0.5), (41, 121, 0.1), (257, 1031, 0.012), (257, 1031, 0.03), (257, 1031, 0.06),
           (257, 1031, 0.12), (257, 1031, 0.3), (257, 1031, 0.9), (1031, 257, 0.02), (1031, 257, 0.9), (513, 131, 0.06)]
# fp32: shapes small enough that every partial sum stays below 2^24 (asserted on the oracle's result)
CASES32 = [(120, 40, 0.02), (40, 120, 0.02), (3, 70, 0.5), (41, 121, 0.1), (41, 121, 0.25), (41, 121, 0.6), (67, 303, 0.2), (67, 303, 0.45),
           (48, 301, 0.9), (161, 150, 0.9), (301, 48, 0.9), (303, 67, 0.3), (121, 41, 0.5)]


def test_case_lists_take_every_lane_count_on_both_matrices():
    for cases in (CASES64, CASES32):
        la, lt, seg = set(), set(), False
        for ny, n, p in cases:
            A = structured(ny, n, p, np.random.default_rng(ny * 7 + n), True, np.float64)
            indptr, indices, data = csr_of(A, np.random.default_rng(1))
            a = plan(indptr, data.shape[0])
            t = plan(transpose_ptr(indices, n), data.shape[0])
            la.add(a[0]); lt.add(t[0]); seg = seg or a[2] or t[2]
        assert la == lt == {1, 2, 4, 8, 16, 32, 64}, (la, lt)
        assert seg or cases is CASES32


def sets(bz, ref, D, dtype):
    return {"zero": (bz.ZeroSet(), ref.ZeroSet()), "free": (bz.FreeSet(), ref.FreeSet()),
            "box": (bz.ClosedSet(bz.IndBox(-1.0, 2.0)), ref.ClosedSet(ref.IndBox(dtype(-1), dtype(2))))}[D]


@pytest.mark.parametrize("D", ["zero", "free", "box"])
@pytest.mark.parametrize("case", [(np.float64, c) for c in CASES64] + [(np.float32, c) for c in CASES32],
                         ids=lambda c: f"{'f64' if c[0] == np.float64 else 'f32'}-{c[1][0]}x{c[1][1]}-{c[1][2]}")
def test_exact_gradient_bit_for_bit(bz, ref, case, D):
    """Integer data, mu = 1/4: every product and every sum is exact in the number format, so no summation order can change
    a bit: gradient and value equal the oracle's BIT FOR BIT."""
    dtype, (ny, n, p) = case
    rng = np.random.default_rng(ny * 7 + n)
    A = structured(ny, n, p, rng, True, dtype)
    indptr, indices, data = csr_of(A, np.random.default_rng(1))
    b = rng.integers(-3, 4, ny).astype(dtype)
    x = rng.integers(-4, 5, n).astype(dtype)
    y = rng.integers(-3, 4, ny).astype(dtype)
    mu = np.full(ny, 0.25, dtype)
    q, fb = rng.integers(1, 4, n).astype(dtype), rng.integers(-3, 4, n).astype(dtype)
    Dd, Dr = sets(bz, ref, D, dtype)
    prob = bz.Problem(bz.DiagQuadratic(q, fb), bz.NormL1(1.0), bz.SparseAffine(indptr, indices, data, b, n), Dd, n, ny, dtype)
    prob.set_multipliers(mu, y)
    prob.profile_enable(True)
    g_dev, vals = prob.eval_al_gradient(x)
    form = prob.profile2()["gemv"]["form"]
    prob.close()
    al = ref.AugLagFun(ref.DiagQuadratic(q, fb), CsrOracle(indptr, indices, data, b, n), Dr, mu.copy(), y.copy(), x)
    g_ref = np.empty(n, dtype)
    lx = al.gradient(g_ref, x)
    # exactness of every partial sum, whatever its order: the sums of magnitudes, in units of the finest granularity (1/8:
    # mu y^2 / 2), stay below 2^24 (fp32) / 2^53 (fp64)
    lim = 2.0 ** (24 if dtype == np.float32 else 53)
    absA = np.abs(A.astype(np.float64))
    yhat = al.yupd.astype(np.float64)
    t = yhat * 0.25
    assert np.max(absA @ np.abs(x.astype(np.float64)) + np.abs(b)) * 4 < lim
    assert np.max(absA.T @ np.abs(yhat)) + np.max(np.abs(q * x - fb)) < lim
    assert 8 * (np.sum(t * t / 0.25) + np.sum(np.abs(x * (0.5 * q * x - fb))) + np.sum(0.25 * y.astype(np.float64) ** 2)) < lim
    assert np.max(np.abs(g_ref)) < 2.0 ** 20
    Lt, _, seg_t = plan(transpose_ptr(indices, n), data.shape[0])
    assert form == f"k_spmv_t_finish<L={Lt},SEG={int(seg_t)}>", form
    assert g_dev.dtype == dtype and np.array_equal(g_dev, g_ref)
    assert vals[0] == float(lx) and vals[1] == float(al.fx)


@pytest.mark.parametrize("D", ["zero", "box"])
@pytest.mark.parametrize("case", [(np.float64, c) for c in CASES64] + [(np.float32, c) for c in CASES32],
                         ids=lambda c: f"{'f64' if c[0] == np.float64 else 'f32'}-{c[1][0]}x{c[1][1]}-{c[1][2]}")
def test_general_gradient_against_oracle_and_dense_kind(bz, ref, case, D):
    """random real data: the tolerances of test_dense_al_gradient for order-dependent sums (1e-12 / 2e-5 of the gradient's
    largest entry; of max(1, |L|) for the value), against the oracle and against the DenseAffine kind on the same matrix"""
    dtype, (ny, n, p) = case
    rng = np.random.default_rng(ny * 11 + n)
    A = structured(ny, n, p, rng, False, dtype)
    indptr, indices, data = csr_of(A, np.random.default_rng(2))
    b = rng.standard_normal(ny).astype(dtype)
    x = rng.standard_normal(n).astype(dtype)
    mu = (10.0 ** rng.uniform(-2, 0, ny)).astype(dtype)
    y = rng.standard_normal(ny).astype(dtype)
    q, fb = rng.uniform(0.5, 2.0, n).astype(dtype), rng.standard_normal(n).astype(dtype)
    Dd, Dr = sets(bz, ref, D, dtype)
    out = {}
    for kind, c in (("sparse", bz.SparseAffine(indptr, indices, data, b, n)), ("dense", bz.DenseAffine(A, b))):
        prob = bz.Problem(bz.DiagQuadratic(q, fb), bz.NormL1(1.0), c, Dd, n, ny, dtype)
        prob.set_multipliers(mu, y)
        out[kind] = prob.eval_al_gradient(x)
        prob.close()
    al = ref.AugLagFun(ref.DiagQuadratic(q, fb), CsrOracle(indptr, indices, data, b, n), Dr, mu.copy(), y.copy(), x)
    g_ref = np.empty(n, dtype)
    lx = float(al.gradient(g_ref, x))
    tol = 1e-12 if dtype == np.float64 else 2e-5
    g_dev, vals = out["sparse"]
    scale = np.max(np.abs(g_ref))
    print(f"max|g - g_ref| / max|g_ref| = {np.max(np.abs(g_dev.astype(np.float64) - g_ref)) / scale:.3e}, "
          f"vs dense kind {np.max(np.abs(g_dev.astype(np.float64) - out['dense'][0])) / scale:.3e}, "
          f"value {abs(vals[0] - lx) / max(1.0, abs(lx)):.3e}")
    assert np.max(np.abs(g_dev.astype(np.float64) - g_ref)) <= tol * scale
    assert abs(vals[0] - lx) <= tol * max(1.0, abs(lx))
    assert np.max(np.abs(g_dev.astype(np.float64) - out["dense"][0])) <= tol * scale
    assert abs(vals[0] - out["dense"][1][0]) <= tol * max(1.0, abs(lx))


def test_long_rows_are_cut_and_runs_are_identical(bz, ref):
    """a budget row over n = 1e6 and a column through 3e5 rows: both matrices take the segmented path; the result is
    within the tolerance of the general case, and the same bits on every run"""
    n, m = 10 ** 6, 3 * 10 ** 5
    d = bz.synth.budget_bands(n, m)
    ny = m + 1
    rng = np.random.default_rng(5)
    x = rng.standard_normal(n) / 100
    mu = 10.0 ** rng.uniform(-2, 0, ny)
    y = rng.standard_normal(ny)
    Dd, Dr = bz.ClosedSet(bz.IndBox(d["lo"], d["hi"])), ref.ClosedSet(ref.IndBox(d["lo"], d["hi"]))
    prob = bz.Problem(bz.DiagQuadratic(d["q"], d["fb"]), bz.IndBox(0.0, 1.0),
                      bz.SparseAffine(d["indptr"], d["indices"], d["data"], d["b"], n), Dd, n, ny, np.float64)
    prob.set_multipliers(mu, y)
    prob.profile_enable(True)
    runs = [prob.eval_al_gradient(x) for _ in range(2)]
    p = prob.profile2()
    prob.close()
    assert p["gemv"]["form"].startswith("k_spmv_t_finish<L=") and p["gemv"]["form"].endswith("SEG=1>"), p["gemv"]["form"]
    assert p["gemv"]["launches"] == 4 and 2 <= p["misc"]["launches"]       # two gradients: two passes each, and the folds
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    al = ref.AugLagFun(ref.DiagQuadratic(d["q"], d["fb"]), CsrOracle(d["indptr"], d["indices"], d["data"], d["b"], n), Dr,
                       mu.copy(), y.copy(), x)
    g_ref = np.empty(n)
    lx = float(al.gradient(g_ref, x))
    g_dev, vals = runs[0]
    print(f"max|g - g_ref| / max|g_ref| = {np.max(np.abs(g_dev - g_ref)) / np.max(np.abs(g_ref)):.3e}, "
          f"value {abs(vals[0] - lx) / max(1.0, abs(lx)):.3e}")
    assert np.max(np.abs(g_dev - g_ref)) <= 1e-12 * np.max(np.abs(g_ref))
    assert abs(vals[0] - lx) <= 1e-12 * max(1.0, abs(lx))


def iterate_problem(bz, ref, which, dtype):
    if which == "cfg4":
        ny, n = 64, 512
        d, dev, orc = make_cfg4(bz, ref, ny, n, dtype, density=0.05)
        dev = dev[:2] + (bz.SparseAffine.from_dense(d["A"], d["b"]),) + dev[3:]      # (oracle: ref.DenseAffine of the matrix)
        return n, ny, dev, orc
    if which == "budget_bands":
        n, m = 2000, 300
        d = bz.synth.budget_bands(n, m, dtype)
        csr = (d["indptr"], d["indices"], d["data"], d["b"], n)
        dev = (bz.DiagQuadratic(d["q"], d["fb"]), bz.IndBox(0.0, 1.0), bz.SparseAffine(*csr), bz.ClosedSet(bz.IndBox(d["lo"], d["hi"])))
        orc = (ref.DiagQuadratic(d["q"], d["fb"]), ref.IndBox(dtype(0), dtype(1)), CsrOracle(*csr), ref.ClosedSet(ref.IndBox(d["lo"], d["hi"])))
        return n, m + 1, dev, orc
    N = 500
    d = bz.synth.obstacle_1d(N, dtype)
    csr = (d["indptr"], d["indices"], d["data"], d["b"], d["n"])
    dev = (bz.DiagQuadratic(d["q"], d["fb"]), bz.NormL1Nonneg(0.1), bz.SparseAffine(*csr), bz.ZeroSet())
    orc = (ref.DiagQuadratic(d["q"], d["fb"]), ref.NormL1Nonneg(0.1), CsrOracle(*csr), ref.ZeroSet())
    return d["n"], N, dev, orc


@pytest.mark.parametrize("which,dtype", [("cfg4", np.float64), ("cfg4", np.float32), ("budget_bands", np.float64),
                                         ("obstacle_1d", np.float64)])
def test_iterates_follow_the_oracle(bz, ref, which, dtype):
    """30 states: x and z inside max(base, 100 * sens) — base 1e-9 / 5e-5, sens the oracle's own extended-precision
    envelope — and gamma equal to 1e-12 / 1e-5 relative: the rule and the numbers of tests/test_gpu_dense.py"""
    n, ny, dev, orc = iterate_problem(bz, ref, which, dtype)
    mu, y = np.full(ny, 0.1, dtype), (0.1 * np.random.default_rng(2).standard_normal(ny)).astype(dtype)
    x0 = np.zeros(n, dtype)
    eps = float(np.finfo(dtype).eps)
    prob, st, rows = run_traces(bz, ref, dev, orc, n, mu, y, x0, 30, minimum_gamma=eps, dtype=dtype, ny=ny)
    stats = prob.panoc_stats()
    prob.close()
    base = 1e-9 if dtype == np.float64 else 5e-5
    for k, ex, ez, g_d, g_r, sn_d, sn_r, fused, sens in rows:
        print(f"k={k} ex={ex:.3e} ez={ez:.3e} gamma {g_d:.9g} / {g_r:.9g} sens={sens:.3e}")
    for k, ex, ez, g_d, g_r, sn_d, sn_r, fused, sens in rows:
        assert abs(g_d - g_r) <= (1e-12 if dtype == np.float64 else 1e-5) * g_r, k
        assert ex <= max(base, 100 * sens) and ez <= max(base, 100 * sens), (k, ex, ez, sens)
    assert stats.n_affine_images == 0


def solve_problem(bz, ref, which):
    if which == "budget_bands":
        n, m = 300, 100
        d = bz.synth.budget_bands(n, m)
        csr = (d["indptr"], d["indices"], d["data"], d["b"], n)
        dev = (bz.DiagQuadratic(d["q"], d["fb"]), bz.IndBox(0.0, 1.0), bz.SparseAffine(*csr), bz.ClosedSet(bz.IndBox(d["lo"], d["hi"])))
        orc = (ref.DiagQuadratic(d["q"], d["fb"]), ref.IndBox(0.0, 1.0), CsrOracle(*csr), ref.ClosedSet(ref.IndBox(d["lo"], d["hi"])))
        gval = lambda x: 0.0
        proj = lambda v: np.clip(v, d["lo"], d["hi"])
        return n, m + 1, dev, orc, d, gval, proj
    N = 64
    d = bz.synth.obstacle_1d(N)
    csr = (d["indptr"], d["indices"], d["data"], d["b"], d["n"])
    dev = (bz.DiagQuadratic(d["q"], d["fb"]), bz.NormL1Nonneg(0.1), bz.SparseAffine(*csr), bz.ZeroSet())
    orc = (ref.DiagQuadratic(d["q"], d["fb"]), ref.NormL1Nonneg(0.1), CsrOracle(*csr), ref.ZeroSet())
    gval = lambda x: 0.1 * np.sum(x)
    proj = lambda v: np.zeros_like(v)
    return d["n"], N, dev, orc, d, gval, proj


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("which", ["budget_bands", "obstacle_1d"])
def test_whole_solves(bz, ref, which):
    """bz.alps, resident and through the host outer loop, against ref.alps: first_order on both sides, feasibility <= 1e-5,
    objective within 1e-4 relative, x within 1e-4 (the bounds of test_dense_panoc_and_alps_fp64).  Iteration counts are not
    compared: the oracle's own count moves by a few per cent when only the summation order of A x changes."""
    n, ny, dev, orc, d, gval, proj = solve_problem(bz, ref, which)
    sub = lambda **kw: bz.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
    subr = lambda **kw: ref.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
    o = ref.alps(*orc, np.zeros(n), np.zeros(ny), subsolver=subr, subsolver_maxit=100000)
    assert o[5] == "first_order"
    obj = lambda x: float(np.sum(x * (0.5 * d["q"] * x - d["fb"])) + gval(x))
    cO = CsrOracle(d["indptr"], d["indices"], d["data"], d["b"], n)
    for resident in (True, False):
        a = bz.alps(*dev, np.zeros(n), np.zeros(ny), subsolver=sub, subsolver_maxit=100000, resident=resident)
        cx = np.empty(ny)
        cO.eval(cx, a[0])
        feas = float(np.max(np.abs(cx - proj(cx))))
        print(f"{which} resident={resident}: status {a[5]} outer {a[2]}/{o[2]} inner {a[3]}/{o[3]} feas {feas:.3e} "
              f"obj {obj(a[0]):.9g}/{obj(o[0]):.9g} max|x - x_ref| {np.max(np.abs(a[0] - o[0])):.3e}")
        assert a[5] == "first_order"
        assert feas <= 1e-5
        assert abs(obj(a[0]) - obj(o[0])) <= 1e-4 * abs(obj(o[0]))
        assert np.max(np.abs(a[0] - o[0])) <= 1e-4


def raw_desc(bz, indptr, indices, data, b, n, D=None, slack=0):
    from bazinga_jl_amd.oracles import lower
    L = bz._lib
    ny = b.shape[0]
    good = bz.SparseAffine(np.array([0] + [0] * ny, np.int64), np.zeros(0, np.int32), np.zeros(0), b, n)
    desc, keep = lower(bz.Zero(), bz.NormL1(1.0), good, bz.ZeroSet(), n, ny, np.float64)
    arrs = (np.ascontiguousarray(indptr, np.int64), np.ascontiguousarray(indices, np.int32), np.ascontiguousarray(data, np.float64))
    desc.c_sp_rowptr, desc.c_sp_col, desc.c_sp_val = (a.ctypes.data for a in arrs)
    desc.c_sp_nnz = arrs[1].shape[0]
    desc.slack = slack
    if D is not None:
        desc.D_kind = D
    return desc, (keep, arrs)


def test_creation_validates_the_matrix_and_refuses_what_is_not_lowered(bz):
    L = bz._lib
    lib = L.load()
    ctx = bz.default_context()
    indptr, indices, data = np.array([0, 2, 3, 5]), np.array([0, 3, 1, 2, 3]), np.arange(1.0, 6.0)
    b, n = np.zeros(3), 4

    def create(desc):
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
        assert rc == L.BZ_ERR_ARG and not made and row in msg, msg
    desc, keep = raw_desc(bz, np.array([0, 2, 3, 4]), indices, data, b, n)              # rowptr[ny] != nnz
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_ARG and not made and "nnz" in msg
    desc, keep = raw_desc(bz, indptr, np.array([0, 3, 1, 4, 3]), data, b, n)            # a column = n, in row 2
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_ARG and not made and "row 2" in msg, msg
    desc, keep = raw_desc(bz, indptr, indices, data, b, n, slack=1)
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_UNSUPPORTED and not made and "slack" in msg
    desc, keep = raw_desc(bz, indptr[:3], indices[:3], data[:3], b[:2], n, D=L.BZ_D_CC_PAIRS)
    rc, made, msg = create(desc)
    assert rc == L.BZ_ERR_UNSUPPORTED and not made and "pairwise" in msg
    # the Python layer raises before any device call
    with pytest.raises(ValueError):
        bz.SparseAffine(np.array([0, 3, 2, 5]), indices, data, b, n)
    with pytest.raises(ValueError):
        bz.SparseAffine(indptr, np.array([0, 3, 1, 4, 3]), data, b, n)
    c = bz.SparseAffine(indptr, indices, data, b, n)
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(bz.Zero(), bz.NormL1(1.0), c, bz.ZeroSet(), n, 3, np.float64, slack=True)
    with pytest.raises(bz.UnsupportedOracle):
        bz.Problem(bz.Zero(), bz.NormL1(1.0), bz.SparseAffine(indptr[:3], indices[:3], data[:3], b[:2], n), bz.XorPairs(), n, 2, np.float64)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", [(257, 500, 0.03, "zero"), (257, 1031, 0.9, "vecbox")])
def test_launches_and_bytes_of_one_gradient(bz, ref, shape, dtype):
    """one AL gradient = one k_spmv_yupd + one k_spmv_t_finish launch (and, for a cut matrix, its fold, counted apart),
    moving what DESIGN 4's model says: per pass both CSR arrays, the (virtual) row pointers, the virtual-row tables of a
    cut matrix, one read of the gathered vector, the per-row vectors in and out"""
    ny, n, p, D = shape
    rng = np.random.default_rng(3)
    A = structured(ny, n, p, rng, False, dtype)
    indptr, indices, data = csr_of(A, np.random.default_rng(2))
    b = rng.standard_normal(ny).astype(dtype)
    q, fb = rng.uniform(0.5, 2.0, n).astype(dtype), rng.standard_normal(n).astype(dtype)
    Dd = bz.ZeroSet() if D == "zero" else bz.ClosedSet(bz.IndBox(np.full(ny, -1.0, dtype), np.full(ny, 2.0, dtype)))
    prob = bz.Problem(bz.DiagQuadratic(q, fb), bz.NormL1(1.0), bz.SparseAffine(indptr, indices, data, b, n), Dd, n, ny, dtype)
    prob.set_multipliers(np.full(ny, 0.5, dtype), rng.standard_normal(ny).astype(dtype))
    prob.profile_reset()
    prob.profile_enable(True)
    prob.eval_al_gradient(rng.standard_normal(n).astype(dtype))
    pr = prob.profile2()
    prob.close()
    sz, nnz = np.dtype(dtype).itemsize, data.shape[0]
    La, nva, sega = plan(indptr, nnz)
    Lt, nvt, segt = plan(transpose_ptr(indices, n), nnz)
    assert sega == (n == 1031) and not segt
    model = 0.0
    for nv, seg, gathered in ((nva, sega, n), (nvt, segt, ny)):
        model += nnz * (sz + 4) + (nv + 1) * 8 + (nv * 8 if seg else 0) + gathered * sz
    model += (4 + (2 if D == "vecbox" else 0)) * ny * sz        # b, mu, mu*y (the bounds of D), yhat
    model += 4 * n * sz                                         # x, q, b of f, the gradient
    assert pr["gemv"]["launches"] == 2 and pr["gemv"]["bytes"] == model, (pr["gemv"], model)
    assert pr["gemv"]["form"] == f"k_spmv_t_finish<L={Lt},SEG=0>"
    assert pr["k_gemv_t_mfma"]["launches"] == 0 and pr["al_gradient"]["launches"] == 0
