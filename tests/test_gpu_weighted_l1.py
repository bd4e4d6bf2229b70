"""g = NormL1 with a per-element lambda (bz_problem_desc.g_lambda_vec) on the device, and lambda changed on a live problem
(bz_problem_set_g_lambda): creation and refusals through the raw ABI, one prox against the oracle's array arm, thirty states
of every path that evaluates the prox, ALS, a constant vector against the number, an unpenalised intercept, the setter.

lambda is 0.5 U(0, 1) with exact zeros at the first index, the last one and one in the middle throughout."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_parity import make_cfg2, make_cfg3, make_cfg4, run_traces
from tests.test_gpu_sparse import csr_of, sets, structured
from tests.test_gpu_sparse_glm import GLMOracle, glm_of, what_of
from tests.test_gpu_sparse_least_squares import CsrOracle
from tests.test_gpu_sparse_logistic import TOL
from tests.test_weighted_l1_host import weights

pytestmark = pytest.mark.gpu

SHAPES = [(41, 121, 0.1), (257, 1031, 0.03)]          # of tests/test_gpu_sparse_least_squares.py
DT = lambda t: "f64" if t == np.float64 else "f32"


def l1_pair(bz, ref, lam):
    return bz.NormL1(lam), ref.NormL1(lam)


def with_intercept(shape, dtype, seed_shift=0):
    """the structured matrix of the sparse tests with one more column of ones (the last one, where lambda is zero), b, and
    its CSR arrays with every row's entries in a shuffled order"""
    m, n, p = shape
    rng = np.random.default_rng(m * 11 + n + seed_shift)
    A = np.concatenate([structured(m, n, p, rng, False, dtype), np.ones((m, 1), dtype)], axis=1)
    b = rng.standard_normal(m).astype(dtype)
    return A, b, csr_of(A, np.random.default_rng(1)), rng


# ---- 1. creation and refusals through the raw ABI
def test_creation_and_refusals_through_the_raw_abi(bz):
    from bazinga_jl_amd.oracles import lower
    L = bz._lib
    lib = L.load()
    ctx = bz.default_context()
    n = 12
    u = np.ones(n)

    def create(desc):
        h = C.c_void_p()
        rc = lib.bz_problem_create(ctx._h, C.byref(desc), C.byref(h))
        msg = lib.bz_last_error().decode() if rc else ""
        if h.value:
            lib.bz_problem_destroy(h)
        return rc, bool(h.value), msg

    def desc_of(lam, kind=L.BZ_G_NORM_L1):
        desc, keep = lower(bz.Zero(), bz.NormL1(1.0), bz.IdentityFunction(), bz.FreeSet(), n, n, np.dtype(np.float64))
        desc.g_kind, desc.g_lambda_vec, desc.g_u, desc.g_p = kind, lam.ctypes.data, u.ctypes.data, 0.5
        return desc, keep

    lam = weights(n)
    assert create(desc_of(lam)[0])[:2] == (0, True)
    desc, keep = desc_of(lam)
    desc.g_lambda = -1.0                                       # ignored beside the vector
    assert create(desc)[:2] == (0, True)
    for bad in (-0.25, np.nan, np.inf):
        worse = lam.copy()
        worse[5] = bad
        rc, made, msg = create(desc_of(worse)[0])
        assert rc == L.BZ_ERR_ARG and not made and "NormL1" in msg and "entry 5" in msg, msg
    for kind in (L.BZ_G_ZERO, L.BZ_G_NORM_L1_NONNEG, L.BZ_G_NORM_L1_BOX, L.BZ_G_IND_BOX, L.BZ_G_NORM_L0_BOX,
                 L.BZ_G_NORM_LP_NONNEG, L.BZ_G_NORM_LP_BOX):
        rc, made, msg = create(desc_of(lam, kind)[0])
        assert rc == L.BZ_ERR_ARG and not made and "NormL1" in msg, (kind, msg)
    # ... and the same kinds without the vector are created
    for kind in (L.BZ_G_NORM_L1_NONNEG, L.BZ_G_NORM_L1_BOX):
        desc, keep = desc_of(lam, kind)
        desc.g_lambda_vec = None
        assert create(desc)[:2] == (0, True)


# ---- 2. one prox against the oracle
SPECIALS = ("nan", "+inf", "-inf", "+0", "-0", "+gl", "-gl")


def special(name, gl_i):
    return {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "+0": 0.0, "-0": -0.0, "+gl": gl_i, "-gl": -gl_i}[name]


@pytest.mark.parametrize("n", [1, 3, 2121])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=DT)
def test_one_prox_against_the_oracle(bz, ref, dtype, n):
    """z bit-equal to ref.NormL1(array).prox (zeros compared with ==, the NaN pattern equal), g(z) inside TOL of sum
    lambda |z|.  Shorter than the three zeros of the rule (n = 1, 3) the plain draw without zeros is run as well."""
    gamma = 0.37
    draws = [weights(n, 4)] + ([0.5 * np.random.default_rng(4).uniform(0.0, 1.0, n)] if n < 5 else [])
    for lam in draws:
        gd, gr = l1_pair(bz, ref, lam)
        prob = bz.Problem(bz.Zero(), gd, bz.IdentityFunction(), bz.FreeSet(), n, n, dtype)
        gl = dtype(gamma) * lam.astype(dtype)
        rng = np.random.default_rng(5)
        xs = []
        if n >= 64:
            x = (0.3 * rng.standard_normal(n)).astype(dtype)
            # every special at a positive lambda, at a zero lambda (the middle one) and in the ragged last pack
            for j, name in enumerate(SPECIALS):
                for i in (7 + j, n - 9 + j):
                    x[i] = special(name, gl[i])
            x[n // 2], x[0], x[n - 1] = np.nan, -0.0, np.inf
            xs.append(x)
        else:
            for j, name in enumerate(SPECIALS):
                x = (0.3 * rng.standard_normal(n)).astype(dtype)
                x[j % n] = special(name, gl[j % n])
                xs.append(x)
        xs.append((0.3 * rng.standard_normal(n)).astype(dtype))           # finite: the value
        for x in xs:
            zr = np.empty(n, dtype)
            with np.errstate(invalid="ignore"):
                vr = float(gr.prox(zr, x, gamma))
            zd, vd = prob.eval_prox(x, gamma)
            assert zd.dtype == dtype
            assert np.array_equal(np.isnan(zd), np.isnan(zr))
            assert np.array_equal(zd, zr, equal_nan=True), (x, zd, zr)
            if np.isfinite(vr):
                scale = float(np.sum(lam * np.abs(zr.astype(np.float64))))
                print(f"n={n} g(z) {vd:.17g} / {vr:.17g}")
                assert abs(vd - vr) <= TOL[dtype] * scale
            else:
                assert (np.isnan(vd) and np.isnan(vr)) or vd == vr
        prob.close()


# ---- 3. thirty states follow the oracle
def follow(bz, ref, dev, orc, n, ny, dtype, seed=2, **kw):
    """the rule of test_iterates_follow_the_oracle in tests/test_gpu_sparse_least_squares.py; returns the profile and how
    many states were held to `base` itself"""
    mu, y = np.full(ny, 0.1, dtype), (0.1 * np.random.default_rng(seed).standard_normal(ny)).astype(dtype)
    x0 = np.zeros(n, dtype)
    eps = float(np.finfo(dtype).eps)
    prob, st, rows = run_traces(bz, ref, dev, orc, n, mu, y, x0, 30, minimum_gamma=eps, dtype=dtype, ny=ny, **kw)
    pr = prob.profile2()
    prob.close()
    base = 1e-9 if dtype == np.float64 else 5e-5
    for k, ex, ez, g_d, g_r, sn_d, sn_r, fused, sens in rows:
        print(f"k={k} ex={ex:.3e} ez={ez:.3e} gamma {g_d:.9g} / {g_r:.9g} sens={sens:.3e} fused={fused}")
    for k, ex, ez, g_d, g_r, sn_d, sn_r, fused, sens in rows:
        assert abs(g_d - g_r) <= (1e-12 if dtype == np.float64 else 1e-5) * g_r, k
        assert ex <= max(base, 100 * sens) and ez <= max(base, 100 * sens), (k, ex, ez, sens)
    tight = sum(1 for r in rows if 100 * r[8] <= base)
    assert tight >= (25 if dtype == np.float64 else 8), tight
    return pr


def setup_diag(bz, ref, dtype):
    n = 2121
    d, dev, orc = make_cfg2(bz, ref, n, dtype=dtype)
    gd, gr = l1_pair(bz, ref, weights(n, 6))
    return n, n, (dev[0], gd) + dev[2:], (orc[0], gr) + orc[2:]


def setup_sparse_ls(bz, ref, dtype, beside_c=False):
    A, b, (indptr, indices, data), rng = with_intercept(SHAPES[0], dtype)
    n = A.shape[1]
    gd, gr = l1_pair(bz, ref, weights(n, 7))
    f, fo = bz.SparseLeastSquares(indptr, indices, data, b, n), ref.LeastSquares(A, b)
    Dd, Dr = sets(bz, ref, "box", dtype)
    if not beside_c:
        return n, n, (f, gd, bz.IdentityFunction(), Dd), (fo, gr, ref.IdentityFunction(), Dr)
    ny = 30
    Ac = structured(ny, n, 0.2, rng, False, dtype)
    bc = rng.standard_normal(ny).astype(dtype)
    csr = csr_of(Ac, np.random.default_rng(3)) + (bc, n)
    return n, ny, (f, gd, bz.SparseAffine(*csr), Dd), (fo, gr, CsrOracle(*csr), Dr)


def setup_glm(bz, ref, dtype, data_seed=0):
    m, n, p = SHAPES[0]
    rng = np.random.default_rng(m * 13 + n + data_seed)
    A = structured(m, n, p, rng, False, dtype)
    b = np.where(rng.random(m) < 0.5, -1.0, 1.0).astype(dtype)
    w = (0.5 + rng.random(m)).astype(dtype)
    f = glm_of(bz, A, b, "logistic", None, w, 1.0 / m)[0]
    fo = GLMOracle(f.toarray(), b, "logistic", None, what_of(w, 1.0 / m, dtype))
    gd, gr = l1_pair(bz, ref, weights(n, 8) / m)
    Dd, Dr = sets(bz, ref, "box", dtype)
    return n, n, (f, gd, bz.IdentityFunction(), Dd), (fo, gr, ref.IdentityFunction(), Dr)


def setup_stencil(bz, ref, dtype):
    nx, ny = 12, 14
    d, n, dev, orc = make_cfg3(bz, ref, nx, ny)
    gd, gr = l1_pair(bz, ref, weights(n, 9) * float(np.max(np.abs(dev[0].b))))
    return n, n, (dev[0], gd) + dev[2:], (orc[0], gr) + orc[2:]


def setup_dense(bz, ref, dtype):
    ny, n = 5, 12                                              # the smallest shape of tests/test_gpu_dense.py
    d, dev, orc = make_cfg4(bz, ref, ny, n, dtype, density=0.5)
    gd, gr = l1_pair(bz, ref, 2.0 * weights(n, 10))
    return n, ny, (dev[0], gd) + dev[2:], (orc[0], gr) + orc[2:]


# (set-up, dtype, the seed of y).  Seeds were chosen on the oracle alone, so that at least 25 / 8 states are held to `base`:
# the first draw did for all but the logistic GLM (10 states; the third draw of its data: 26)
FOLLOW = [("diag", np.float64, 2), ("diag", np.float32, 2), ("sparse-ls", np.float64, 2), ("sparse-ls", np.float32, 2),
          ("sparse-ls+c", np.float64, 2), ("glm", np.float64, 2), ("stencil", np.float64, 2), ("dense", np.float32, 2)]


def setup_of(bz, ref, which, dtype):
    return {"diag": setup_diag, "sparse-ls": setup_sparse_ls, "sparse-ls+c": lambda *a: setup_sparse_ls(*a, beside_c=True),
            "glm": lambda *a: setup_glm(*a, data_seed=2), "stencil": setup_stencil, "dense": setup_dense}[which](bz, ref, dtype)


@pytest.mark.parametrize("which,dtype,seed", FOLLOW, ids=[f"{w}-{DT(t)}" for w, t, _ in FOLLOW])
def test_thirty_states_follow_the_oracle(bz, ref, which, dtype, seed):
    n, ny, dev, orc = setup_of(bz, ref, which, dtype)
    pr = follow(bz, ref, dev, orc, n, ny, dtype, seed)
    # the host keeps the vector out of the family kernels (and of every other iterate-history pass)
    assert pr["k_fused_iterates"]["launches"] == 0, pr["k_fused_iterates"]
    if which == "diag":
        assert pr["k_fused_sep"]["form"].startswith("k_fused_compact<XR=0,SPEC=0"), pr["k_fused_sep"]["form"]
    if which.startswith("sparse") or which == "glm":
        assert pr["gemv"]["form"].startswith("k_spmv_"), pr["gemv"]["form"]
    if which == "stencil":
        assert pr["k_stencil_fb"]["launches"] > 0


# ---- 4. ALS
def als_case(bz, ref, which):
    nx = 100
    q, fb = 0.5 + bz.synth.uniform(1, nx), 2 * bz.synth.uniform(2, nx) - 1
    lam = 0.2 * weights(nx, 11)
    gd, gr = l1_pair(bz, ref, lam)
    obj = lambda x: float(np.sum(x * (0.5 * q * x - fb)) + np.sum(lam * np.abs(x)))
    if which == "identity":
        dev = (bz.DiagQuadratic(q, fb), gd, bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(-0.1, 0.2)))
        orc = (ref.DiagQuadratic(q, fb), gr, ref.IdentityFunction(), ref.ClosedSet(ref.IndBox(-0.1, 0.2)))
        return nx, nx, dev, orc, obj, lambda x: x
    ny = 20
    d = bz.synth.basis_pursuit(ny, nx, dtype=np.float64, density=0.05)
    dev = (bz.DiagQuadratic(q, fb), gd, bz.DenseAffine(d["A"], d["b"]), bz.ClosedSet(bz.IndBox(-0.1, 0.2)))
    orc = (ref.DiagQuadratic(q, fb), gr, ref.DenseAffine(d["A"], d["b"]), ref.ClosedSet(ref.IndBox(-0.1, 0.2)))
    return nx, ny, dev, orc, obj, lambda x: d["A"] @ x - d["b"]


@pytest.mark.parametrize("which", ["identity", "dense"])
def test_als_against_the_oracle(bz, ref, which):
    """the comparison of test_whole_solves in tests/test_gpu_als_dense.py; the fast slack kernels are not taken"""
    nx, ny, dev, orc, obj, cfun = als_case(bz, ref, which)
    sub_kw = dict(maxit=100000, minimum_gamma=2.3e-16)
    x0 = np.zeros(nx)
    o = ref.als(*orc, x0.copy(), np.zeros(ny), subsolver=lambda **k: ref.PANOCplus(**sub_kw, **k), subsolver_maxit=100000)
    assert o[5] == "first_order"
    prob = bz.Problem(*dev, nx, ny, np.float64, slack=True)
    a = bz.als(*dev, x0, np.zeros(ny), subsolver=lambda **k: bz.PANOCplus(**sub_kw, **k), subsolver_maxit=100000, problem=prob)
    pr = prob.profile2()
    prob.close()
    cx = cfun(a[0])
    feas = float(np.max(np.abs(cx - np.clip(cx, -0.1, 0.2))))
    print(f"{which}: status {a[5]} outer {a[2]}/{o[2]} inner {a[3]}/{o[3]} feas {feas:.3e} obj {obj(a[0]):.9g}/{obj(o[0]):.9g} "
          f"max|x - x_ref| {np.max(np.abs(a[0] - o[0])):.3e} forms {pr['k_fused_iterates']['form']!r} {pr['k_fused_sep']['form']!r}")
    assert a[5] == "first_order"
    assert feas <= 1e-5
    assert abs(obj(a[0]) - obj(o[0])) <= 1e-4 * abs(obj(o[0]))
    assert np.max(np.abs(a[0] - o[0])) <= 1e-4
    assert np.max(np.abs(a[8] - np.clip(a[8], -0.1, 0.2))) == 0.0
    assert "fast" not in pr["k_fused_iterates"]["form"]
    if which == "identity":
        assert pr["k_fused_iterates"]["launches"] + pr["k_fused_sep"]["launches"] > 0      # (the run-time one-pass forms)


# ---- 5. a constant vector equals the number
def stepped(bz, dev, n, ny, dtype, x0, steps, mu, y, before=None):
    """the states (x, z, the sixteen scalars) of `steps` steps from x0; before(prob): run first, on the same problem"""
    prob = bz.Problem(*dev, n, ny, dtype)
    prob.set_multipliers(mu, y)
    if before is not None:
        before(prob)
    out = trace(bz, prob, x0, steps)
    pr = prob.profile2()
    prob.close()
    return out, pr


def trace(bz, prob, x0, steps, fuse=True):
    sub = bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=float(np.finfo(prob.dtype).eps), fuse=fuse)
    prob.panoc_begin(sub.c_opts(), x0)
    out = []
    for k in range(steps + 1):
        sc = prob.panoc_scalars()
        out.append((prob.panoc_vector("x"), prob.panoc_vector("z"), [sc[name] for name in prob.SCALAR_NAMES]))
        if k < steps:
            prob.panoc_step()
    prob.panoc_finish()
    return out


def lasso_ls(bz, dtype=np.float64):
    A, b, (indptr, indices, data), rng = with_intercept(SHAPES[0], dtype)
    n = A.shape[1]
    rest = (bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(-1.0, 2.0)))
    mu, y = np.full(n, 0.1, dtype), (0.1 * np.random.default_rng(2).standard_normal(n)).astype(dtype)
    return n, lambda: bz.SparseLeastSquares(indptr, indices, data, b, n), rest, mu, y


def test_constant_vector_equals_the_number(bz):
    n, f, rest, mu, y = lasso_ls(bz)
    x0 = np.zeros(n)
    # lambda = 0.5: gamma * lambda and lambda * |z| are exact scalings, so every bit of every state is the same
    a, pra = stepped(bz, (f(), bz.NormL1(0.5)) + rest, n, n, np.float64, x0, 30, mu, y)
    b, prb = stepped(bz, (f(), bz.NormL1(np.full(n, 0.5))) + rest, n, n, np.float64, x0, 30, mu, y)
    for k, ((xa, za, sa), (xb, zb, sb)) in enumerate(zip(a, b)):
        assert np.array_equal(xa, xb) and np.array_equal(za, zb), k
        assert sa == sb, (k, sa, sb)
    assert {c: pra[c]["launches"] for c in pra} == {c: prb[c]["launches"] for c in prb}          # the same kernels
    assert any(np.any(x != 0) for x, _, _ in a)
    # lambda = 0.3: the first step's x and z bit-equal, g(z) inside TOL
    a, _ = stepped(bz, (f(), bz.NormL1(0.3)) + rest, n, n, np.float64, x0, 1, mu, y)
    b, _ = stepped(bz, (f(), bz.NormL1(np.full(n, 0.3))) + rest, n, n, np.float64, x0, 1, mu, y)
    for (xa, za, sa), (xb, zb, sb) in zip(a, b):
        assert np.array_equal(xa, xb) and np.array_equal(za, zb)
        gz_a, gz_b = sa[4], sb[4]
        print(f"g_z {gz_a:.17g} / {gz_b:.17g}")
        assert abs(gz_a - gz_b) <= TOL[np.float64] * 0.3 * float(np.sum(np.abs(za)))


# ---- 6. the intercept is unpenalised
def test_intercept_is_unpenalised(bz, ref):
    """a whole alps on the 257 x 1031 Lasso with a column of ones and lambda = 0 there: first_order, the gradient of f at that
    column within 10 x the returned inner_tol, x within 1e-4 of ref.alps (the bound of the whole solves in
    tests/test_gpu_sparse_least_squares.py).  Both sides run with tol = 1e-8 instead of the default 1e-6: with m < n the default
    does not determine the minimiser to 1e-4 — the oracle alone, started 1e-9 away from x0 = 0, ends 2.5e-4 away from itself
    (3563 against 3668 inner iterations); at 1e-8 the same two oracle runs end 1.3e-6 apart.  The bounds are unchanged, and the
    gradient's is the tighter for it."""
    A, b, (indptr, indices, data), rng = with_intercept(SHAPES[1], np.float64)
    n = A.shape[1]
    lam = weights(n, 12)
    assert lam[n - 1] == 0.0 and np.all(A[:, n - 1] == 1.0)
    gd, gr = l1_pair(bz, ref, lam)
    dev = (bz.SparseLeastSquares(indptr, indices, data, b, n), gd, bz.IdentityFunction(), bz.FreeSet())
    orc = (ref.LeastSquares(A, b), gr, ref.IdentityFunction(), ref.FreeSet())
    sub = lambda **kw: bz.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
    subr = lambda **kw: ref.PANOCplus(maxit=100000, minimum_gamma=2.3e-16, **kw)
    o = ref.alps(*orc, np.zeros(n), np.zeros(n), subsolver=subr, subsolver_maxit=100000, tol=1e-8)
    a = bz.alps(*dev, np.zeros(n), np.zeros(n), subsolver=sub, subsolver_maxit=100000, tol=1e-8)
    grad = A.T @ (A @ a[0] - b)
    print(f"status {a[5]} / {o[5]} outer {a[2]}/{o[2]} inner {a[3]}/{o[3]} inner_tol {a[6]:.3e} |grad_intercept| {abs(grad[n - 1]):.3e} "
          f"x_intercept {a[0][n - 1]:.6g} max|x - x_ref| {np.max(np.abs(a[0] - o[0])):.3e}")
    assert o[5] == "first_order" and a[5] == "first_order"
    assert abs(grad[n - 1]) <= 10 * a[6]
    assert np.max(np.abs(a[0] - o[0])) <= 1e-4
    assert a[0][n - 1] != 0.0


# ---- 7. the setter
def assert_same_states(a, b):
    assert len(a) == len(b)
    for k, ((xa, za, sa), (xb, zb, sb)) in enumerate(zip(a, b)):
        assert np.array_equal(xa, xb) and np.array_equal(za, zb), k
        assert sa == sb, (k, sa, sb)


def test_set_g_lambda_vector_equals_a_fresh_problem(bz):
    n, f, rest, mu, y = lasso_ls(bz)
    lam1, lam2 = weights(n, 13), 0.3 * weights(n, 14)
    x0 = (0.1 * np.random.default_rng(3).standard_normal(n))
    held = {}

    def before(prob):
        held["first"] = trace(bz, prob, x0, 20)                # a solve at lambda_1 on the same problem
        prob.set_g_lambda(lam2)
    a, _ = stepped(bz, (f(), bz.NormL1(lam1)) + rest, n, n, np.float64, x0, 20, mu, y, before)
    b, _ = stepped(bz, (f(), bz.NormL1(lam2)) + rest, n, n, np.float64, x0, 20, mu, y)
    assert_same_states(a, b)
    assert not np.array_equal(held["first"][-1][1], a[-1][1])  # ... and lambda_1 gave something else


def test_set_g_lambda_number_keeps_the_one_pass_form(bz, ref):
    n = 2121
    d, dev, orc = make_cfg2(bz, ref, n)
    lam1, lam2 = float(d["lam"]), 0.4 * float(d["lam"])
    mu, y = np.full(n, 0.1), 0.1 * np.random.default_rng(2).standard_normal(n)
    x0 = np.zeros(n)
    held = {}

    def before(prob):
        held["first"] = trace(bz, prob, x0, 20)
        prob.set_g_lambda(lam2)
    a, pra = stepped(bz, (dev[0], bz.NormL1(lam1)) + dev[2:], n, n, np.float64, x0, 20, mu, y, before)
    b, prb = stepped(bz, (dev[0], bz.NormL1(lam2)) + dev[2:], n, n, np.float64, x0, 20, mu, y)
    assert_same_states(a, b)
    assert not np.array_equal(held["first"][-1][1], a[-1][1])
    fused = prob_names(bz).index("fused")
    # (a step whose trial point is rejected ends in the kernel chain: the flags are the fresh problem's, by the equality above)
    served = sum(int(s[fused]) for _, _, s in a[1:])
    print(f"one-pass steps after the setter: {served} of 20; before it: {sum(int(s[fused]) for _, _, s in held['first'][1:])}")
    assert served >= 10 and a[-1][2][fused] == b[-1][2][fused]
    assert pra["k_fused_iterates"]["launches"] > prb["k_fused_iterates"]["launches"] > 0
    assert pra["k_fused_iterates"]["form"].startswith("k_fused_compact<XR=2"), pra["k_fused_iterates"]["form"]


def prob_names(bz):
    return list(bz.Problem.SCALAR_NAMES)


def test_set_g_lambda_refusals(bz):
    L = bz._lib
    lib = L.load()
    n, f, rest, mu, y = lasso_ls(bz)
    lam = weights(n, 15)
    x0 = np.zeros(n)
    set_raw = lambda prob, number, vec: (lib.bz_problem_set_g_lambda(prob._h, number, None if vec is None else vec.ctypes.data),
                                         lib.bz_last_error().decode())
    vecp = bz.Problem(f(), bz.NormL1(lam), *rest, n, n, np.float64)
    nump = bz.Problem(f(), bz.NormL1(0.5), *rest, n, n, np.float64)
    boxp = bz.Problem(f(), bz.IndBox(-1.0, 1.0), *rest, n, n, np.float64)
    for prob in (vecp, nump, boxp):
        prob.set_multipliers(mu, y)
    sub = bz.PANOCplus(tol=0.0, maxit=10 ** 9)
    # between begin and finish
    for prob, args in ((vecp, (0.0, lam)), (nump, (0.25, None))):
        prob.panoc_begin(sub.c_opts(), x0)
        prob.panoc_step()
        rc, msg = set_raw(prob, *args)
        assert rc == L.BZ_ERR_STATE and "bz_panoc_finish" in msg, msg
        prob.panoc_finish()
        assert set_raw(prob, *args)[0] == 0
    # a vector on a problem made with a number and the reverse ; a negative or NaN entry, a negative number ; g = IndBox
    rc, msg = set_raw(nump, 0.0, lam)
    assert rc == L.BZ_ERR_ARG and "NormL1" in msg, msg
    rc, msg = set_raw(vecp, 0.25, None)
    assert rc == L.BZ_ERR_ARG and "NormL1" in msg, msg
    for bad in (-0.5, np.nan):
        worse = lam.copy()
        worse[3] = bad
        rc, msg = set_raw(vecp, 0.0, worse)
        assert rc == L.BZ_ERR_ARG and "entry 3" in msg, msg
    assert set_raw(nump, -0.25, None)[0] == L.BZ_ERR_ARG
    for args in ((0.25, None), (0.0, lam)):
        rc, msg = set_raw(boxp, *args)
        assert rc == L.BZ_ERR_ARG and "NormL1" in msg, msg
    # a refused call changes nothing: the vector problem still runs on lam
    z1, g1 = vecp.eval_prox(np.full(n, 0.4), 1.0)
    fresh = bz.Problem(f(), bz.NormL1(lam), *rest, n, n, np.float64)
    z2, g2 = fresh.eval_prox(np.full(n, 0.4), 1.0)
    assert np.array_equal(z1, z2) and g1 == g2
    with pytest.raises(bz.BazingaHipError) as ei:
        nump.set_g_lambda(lam)
    assert ei.value.code == L.BZ_ERR_ARG
    with pytest.raises(ValueError):
        vecp.set_g_lambda(lam[:-1])
    for prob in (vecp, nump, boxp, fresh):
        prob.close()
