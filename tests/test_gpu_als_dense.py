"""The slack (ALS) form with a dense affine constraint c(x) = A x - b (halves of unequal length: x has nx elements, s has
ny), and a dense f beside a dense c in both forms: creation and the refusals that stay, the lifted AL gradient bit for
bit on exact data and to the dense tolerances on real data, the lifted prox step element by element, thirty PANOCplus
states and whole solves against the oracle's als (src/algorithms/als.jl, src/utilities/auglagfunslack.jl)."""
import ctypes as C
import warnings

import numpy as np
import pytest

from tests.test_gpu_parity import LongDoubleReducer, _err

pytestmark = pytest.mark.gpu

# (ny, nx): nx whole packs in both types; ny odd (a ragged s half), ny > nx and ny < nx, nx % 64 == 0 in fp32 (the MFMA
# transposed product) and not, and (257, 1028) more rows than one row chunk (plan_chunks: 2048 chunks at most)
SHAPES = [(3, 8), (20, 100), (257, 1028), (120, 40)]
CASES = [(np.float64, s) for s in SHAPES] + [(np.float32, s) for s in SHAPES + [(64, 512)]]
case_id = lambda c: f"{'f64' if c[0] == np.float64 else 'f32'}-{c[1][0]}x{c[1][1]}"


def pack_of(dtype):
    return 16 // np.dtype(dtype).itemsize


def row_chunks(rows, cols, dtype):
    """plan_chunks of the transposed product, restated: enough row chunks to fill the chip, a function of the shape"""
    colblocks = max(1, (cols // pack_of(dtype) + 255) // 256)
    chunks = max(1, min(rows, (2048 + colblocks - 1) // colblocks))
    rpc = -(-rows // chunks)
    return -(-rows // rpc)


def smooth_costs(bz, ref, which, nx, dtype, rng, integer=False):
    if which == "zero":
        return bz.Zero(), ref.Zero()
    if which == "diag":
        if integer:
            q, fb = rng.integers(1, 4, nx).astype(dtype), rng.integers(-3, 4, nx).astype(dtype)
        else:
            q, fb = rng.uniform(0.5, 2.0, nx).astype(dtype), rng.standard_normal(nx).astype(dtype)
        return bz.DiagQuadratic(q, fb), ref.DiagQuadratic(q, fb)
    if which == "quadratic":
        F = rng.standard_normal((nx, max(1, nx // 8)))
        Q = (F @ F.T / nx + np.diag(rng.uniform(0.5, 1.5, nx)))
        Q = (0.5 * (Q + Q.T)).astype(dtype)
        q = rng.standard_normal(nx).astype(dtype)
        return bz.Quadratic(Q, q), ref.Quadratic(Q, q)
    FA = (rng.standard_normal((30, nx)) / np.sqrt(nx)).astype(dtype)         # LeastSquares, 30 rows
    fb = rng.standard_normal(30).astype(dtype)
    return bz.LeastSquares(FA, fb), ref.LeastSquares(FA, fb)


# ------------------------------------------------------------------ (1) creation and the refusals that stay
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_creation_and_refusals(bz, ref, dtype):
    """The slack form takes DenseAffine with f in {Zero, DiagQuadratic, Quadratic, LeastSquares}, and a dense f sits
    beside a dense c without slack too (before this feature: BZ_ERR_UNSUPPORTED for every one of them).  What stays
    refused keeps its code."""
    from bazinga_jl_amd.oracles import lower, lower_generic
    L = bz._lib
    lib = L.load()
    ctx = bz.default_context()
    ny, nx = 5, 8
    rng = np.random.default_rng(0)
    A, b = rng.standard_normal((ny, nx)).astype(dtype), rng.standard_normal(ny).astype(dtype)
    g, D = bz.NormL1(1.0), bz.ClosedSet(bz.IndBox(-1.0, 1.0))
    for which in ("zero", "diag", "quadratic", "ls"):
        f = smooth_costs(bz, ref, which, nx, dtype, rng)[0]
        bz.Problem(f, g, bz.DenseAffine(A, b), D, nx, ny, dtype, slack=True).close()
        if which in ("quadratic", "ls"):
            bz.Problem(f, g, bz.DenseAffine(A, b), D, nx, ny, dtype).close()

    def create(desc, context=ctx):
        h = C.c_void_p()
        rc = lib.bz_problem_create(context._h, C.byref(desc), C.byref(h))
        msg = lib.bz_last_error().decode() if rc else ""
        if h.value:
            lib.bz_problem_destroy(h)
        return rc, bool(h.value), msg

    def refused(desc, code, word, context=ctx):
        rc, made, msg = create(desc, context)
        assert rc == code and not made and word in msg, (rc, made, msg)

    sp = bz.SparseAffine.from_dense(A, b)
    # the slack form with a sparse c
    desc, keep = lower(bz.Zero(), g, sp, bz.ZeroSet(), nx, ny, dtype)
    desc.slack = 1
    refused(desc, L.BZ_ERR_UNSUPPORTED, "slack")
    # ... with the stencil f (c = Identity, and beside a dense c)
    desc, keep = lower(bz.Stencil5ptQuadratic(2, 4, np.zeros(nx, dtype)), g, bz.IdentityFunction(), bz.FreeSet(), nx, nx, dtype)
    desc.slack = 1
    refused(desc, L.BZ_ERR_UNSUPPORTED, "slack")
    desc, keep = lower(bz.Zero(), g, bz.DenseAffine(A, b), D, nx, ny, dtype, slack=True)
    keep_b = np.zeros(nx, dtype)
    desc.f_kind, desc.f_grid_nx, desc.f_grid_ny, desc.f_b = L.BZ_F_STENCIL5, 2, 4, keep_b.ctypes.data
    refused(desc, L.BZ_ERR_UNSUPPORTED, "slack")
    # ... with a dense f and c = Identity (not asked for: the one case where a slack variable buys nothing)
    desc, keep = lower(smooth_costs(bz, ref, "quadratic", nx, dtype, rng)[0], g, bz.IdentityFunction(), bz.FreeSet(), nx, nx, dtype)
    desc.slack = 1
    refused(desc, L.BZ_ERR_UNSUPPORTED, "slack")
    # ... with pairwise D
    for kind in ("vc", "cc", "eitheror", "xor"):
        with pytest.raises(bz.BazingaHipError) as e:
            bz.Problem(bz.Zero(), bz.Zero(), bz.IdentityFunction(), bz.PairwiseSet(kind), nx, nx, dtype, slack=True)
        assert e.value.code == L.BZ_ERR_UNSUPPORTED and "no slack" in str(e.value)
    desc, keep = lower(bz.Zero(), g, bz.DenseAffine(A[:4], b[:4]), D, nx, 4, dtype, slack=True)
    desc.D_kind = L.BZ_D_CC_PAIRS
    refused(desc, L.BZ_ERR_UNSUPPORTED, "pairwise")
    # ... with generic callbacks
    class Gen:
        def gradient(self, dfx, x): dfx[...] = 0; return 0.0
        def prox(self, z, x, gamma): z[...] = x; return 0.0
        def eval(self, cx, x): cx[...] = 0
        def jtprod(self, jtv, x, v): jtv[...] = 0
        def proj(self, s, v): s[...] = v
    G = Gen()
    desc, keep = lower_generic(G, G, G, G, nx, ny, dtype)
    desc.slack = 1
    refused(desc, L.BZ_ERR_UNSUPPORTED, "slack")
    # ... on more than one rank (which is also how a dense c is row-sharded)
    ctx2 = bz.Context(device=0, rank=0, nranks=2, comm_id=None)
    desc, keep = lower(bz.Zero(), g, bz.DenseAffine(A, b), D, nx, ny, dtype, slack=True)
    refused(desc, L.BZ_ERR_UNSUPPORTED, "not sharded", ctx2)
    ctx2.close()
    # a dense f beside a sparse c
    desc, keep = lower(bz.Zero(), g, sp, bz.ZeroSet(), nx, ny, dtype)
    fq, keep2 = lower(smooth_costs(bz, ref, "quadratic", nx, dtype, rng)[0], g, bz.DenseAffine(A, b), D, nx, ny, dtype)
    desc.f_kind, desc.f_A, desc.f_b, desc.f_rows = fq.f_kind, fq.f_A, fq.f_b, fq.f_rows
    refused(desc, L.BZ_ERR_UNSUPPORTED, "sparse")
    # the pack rule on nx, with its text
    pk = pack_of(dtype)
    A1, x1 = rng.standard_normal((ny, pk + 1)).astype(dtype), pk + 1
    with pytest.raises(bz.BazingaHipError) as e:
        bz.Problem(bz.Zero(), g, bz.DenseAffine(A1, b), D, x1, ny, dtype, slack=True)
    assert e.value.code == L.BZ_ERR_ARG and "multiple of 16 bytes" in str(e.value)
    # als(resident=False, warm_start=True)
    with pytest.raises(bz.UnsupportedOracle):
        bz.als(bz.Zero(), g, bz.DenseAffine(A, b), D, np.zeros(nx, dtype), np.zeros(ny, dtype), resident=False, warm_start=True)
    # the two entry points keep to their own form
    prob = bz.Problem(bz.Zero(), g, bz.DenseAffine(A, b), D, nx, ny, dtype, slack=True)
    assert prob.n == nx + ny
    prob.close()


# ------------------------------------------------------------------ (2) the lifted AL gradient bit for bit
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_exact_lifted_gradient_bit_for_bit(bz, ref, case):
    """Integer A in {-2, -1, 1, 2}, integer b, x, s, y, q and f's b, mu = 1/4: every product and every sum is exact in
    the number format (asserted below on the oracle's side), so no summation order can change a bit — both halves of
    dFxs and the value equal the oracle's BIT FOR BIT.  (fp32: x has six non-zeros, so that the sums of a 257 x 1028
    matrix stay below 2^24.)  One gradient is one row product and one transposed product: the bytes of A twice."""
    dtype, (ny, nx) = case
    rng = np.random.default_rng(ny * 7 + nx)
    A = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), (ny, nx)).astype(dtype)
    b = rng.integers(-3, 4, ny).astype(dtype)
    x = rng.integers(-4, 5, nx).astype(dtype)
    if dtype == np.float32:
        x = np.zeros(nx, dtype)
        x[rng.choice(nx, min(nx, 6), replace=False)] = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), min(nx, 6))
    s = rng.integers(-3, 4, ny).astype(dtype)
    y = rng.integers(-3, 4, ny).astype(dtype)
    mu = np.full(ny, 0.25, dtype)
    xs = np.concatenate([x, s])
    f_d, f_r = smooth_costs(bz, ref, "diag", nx, dtype, rng, integer=True)
    prob = bz.Problem(f_d, bz.NormL1(1.0), bz.DenseAffine(A, b), bz.ClosedSet(bz.IndBox(-1.0, 2.0)), nx, ny, dtype, slack=True)
    prob.set_multipliers(mu, y)
    prob.profile_reset()
    prob.profile_enable(True)
    g_dev, vals = prob.eval_al_gradient(xs)
    pr = prob.profile2()
    prob.close()
    F = ref.AugLagFunSlack(f_r, ref.DenseAffine(A, b), mu.copy(), y.copy(), x)
    g_ref = np.empty(nx + ny, dtype)
    Fxs = F.gradient(g_ref, xs)
    # exactness of every partial sum, whatever its order: the sums of magnitudes in units of the finest granularity
    # (1/8: mu y^2 / 2; w = cx + y/4 - s is a multiple of 1/4, w^2/mu of 1/4) stay below 2^24 (fp32) / 2^53 (fp64)
    lim = 2.0 ** (24 if dtype == np.float32 else 53)
    absA, x64, y64, s64 = np.abs(A.astype(np.float64)), x.astype(np.float64), y.astype(np.float64), s.astype(np.float64)
    cx = A.astype(np.float64) @ x64 - b
    w = cx + 0.25 * y64 - s64
    yupd = F.yupd.astype(np.float64)
    assert np.array_equal(yupd, y64 + 4.0 * (cx - s64))
    assert (np.max(absA @ np.abs(x64) + np.abs(b)) + np.max(np.abs(s64)) + 1) * 4 < lim
    assert np.max(absA.T @ np.abs(yupd)) + np.max(np.abs(f_r.q * x - f_r.b)) < lim
    assert 8 * (np.sum(w * w / 0.25) + np.sum(np.abs(x64 * (0.5 * f_r.q * x64 - f_r.b))) + np.sum(0.25 * y64 ** 2)) < lim
    assert g_dev.dtype == dtype
    assert np.array_equal(g_dev[:nx], g_ref[:nx]), "x half"
    assert np.array_equal(g_dev[nx:], g_ref[nx:]) and np.array_equal(g_dev[nx:], -F.yupd), "s half"
    assert vals[0] == float(Fxs) and vals[1] == float(f_r(x))
    # launches and bytes: A x - b (the matrix, x, b, cx) and A' yupd (the matrix, yupd, the row-chunk partials)
    mfma = dtype == np.float32 and nx % 64 == 0
    sz = np.dtype(dtype).itemsize
    rows_bytes = (ny * nx + nx + 2 * ny) * sz
    cols_bytes = (ny * nx + ny + row_chunks(ny, nx, dtype) * nx) * sz
    assert pr["gemv"]["launches"] == (1 if mfma else 2) and pr["k_gemv_t_mfma"]["launches"] == (1 if mfma else 0)
    assert pr["gemv"]["bytes"] + pr["k_gemv_t_mfma"]["bytes"] == rows_bytes + cols_bytes, (pr["gemv"], pr["k_gemv_t_mfma"])
    assert pr["gemv"]["bytes"] + pr["k_gemv_t_mfma"]["bytes"] - (3 * ny + nx + row_chunks(ny, nx, dtype) * nx) * sz == 2 * ny * nx * sz
    assert pr["gemv"]["form"] == ("k_gemv_n" if mfma else "k_gemv_t") and (not mfma or pr["k_gemv_t_mfma"]["form"] == "k_gemv_t_mfma")
    # the ny-length kernel between the passes, and no kernel of its own for the s half of the gradient
    assert pr["al_gradient"]["launches"] == 1 and pr["al_gradient"]["form"] == "k_algrad_slack_rows"
    assert pr["al_gradient"]["bytes"] == 7 * ny * sz
    assert pr["misc"]["launches"] == 1                      # the finish: dFxs[:nx] = grad f + A' yupd
    assert pr["fb_step"]["launches"] == 0 and pr["k_fused_iterates"]["launches"] == 0


# ------------------------------------------------------------------ (3) the lifted gradient on real data
@pytest.mark.parametrize("which", ["zero", "diag", "quadratic", "ls"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_lifted_gradient_on_real_data(bz, ref, case, which):
    """random real data, non-uniform penalties 10^U(-2, 0): the tolerances of test_dense_al_gradient for order-dependent
    sums — 1e-12 (fp64) / 2e-5 (fp32) of the gradient's largest entry, of max(1, |F|) for the value.  With a dense f the
    gradient of the alps form (no slack) is checked against ref.AugLagFun at the same tolerances."""
    dtype, (ny, nx) = case
    rng = np.random.default_rng(ny * 11 + nx)
    A = (rng.standard_normal((ny, nx)) / np.sqrt(nx)).astype(dtype)
    b = rng.standard_normal(ny).astype(dtype)
    xs = rng.standard_normal(nx + ny).astype(dtype)
    mu = (10.0 ** rng.uniform(-2, 0, ny)).astype(dtype)
    y = rng.standard_normal(ny).astype(dtype)
    f_d, f_r = smooth_costs(bz, ref, which, nx, dtype, rng)
    D_d, D_r = bz.ClosedSet(bz.IndBox(-1.0, 2.0)), ref.ClosedSet(ref.IndBox(dtype(-1), dtype(2)))
    tol = 1e-12 if dtype == np.float64 else 2e-5
    prob = bz.Problem(f_d, bz.NormL1(1.0), bz.DenseAffine(A, b), D_d, nx, ny, dtype, slack=True)
    prob.set_multipliers(mu, y)
    g_dev, vals = prob.eval_al_gradient(xs)
    g_again, vals_again = prob.eval_al_gradient(xs)
    prob.close()
    assert np.array_equal(g_dev, g_again) and vals == vals_again
    F = ref.AugLagFunSlack(f_r, ref.DenseAffine(A, b), mu.copy(), y.copy(), xs[:nx])
    g_ref = np.empty(nx + ny, dtype)
    Fxs = float(F.gradient(g_ref, xs))
    scale = float(np.max(np.abs(g_ref)))
    ex = float(np.max(np.abs(g_dev[:nx].astype(np.float64) - g_ref[:nx]))) / scale
    es = float(np.max(np.abs(g_dev[nx:].astype(np.float64) - g_ref[nx:]))) / scale
    print(f"slack {which}: x half {ex:.3e}, s half {es:.3e}, value {abs(vals[0] - Fxs) / max(1.0, abs(Fxs)):.3e} (tol {tol:g})")
    assert ex <= tol and es <= tol
    assert abs(vals[0] - Fxs) <= tol * max(1.0, abs(Fxs))
    assert abs(vals[1] - float(f_r(xs[:nx]))) <= tol * max(1.0, abs(Fxs))
    if which in ("quadratic", "ls"):
        x = xs[:nx]
        prob = bz.Problem(f_d, bz.NormL1(1.0), bz.DenseAffine(A, b), D_d, nx, ny, dtype)
        prob.set_multipliers(mu, y)
        prob.profile_reset()
        prob.profile_enable(True)
        g_dev, vals = prob.eval_al_gradient(x)
        pr = prob.profile2()
        prob.close()
        al = ref.AugLagFun(f_r, ref.DenseAffine(A, b), D_r, mu.copy(), y.copy(), x)
        g_ref = np.empty(nx, dtype)
        lx = float(al.gradient(g_ref, x))
        scale = float(np.max(np.abs(g_ref)))
        e = float(np.max(np.abs(g_dev.astype(np.float64) - g_ref))) / scale
        print(f"alps form {which}: gradient {e:.3e}, value {abs(vals[0] - lx) / max(1.0, abs(lx)):.3e} (tol {tol:g})")
        assert e <= tol
        assert abs(vals[0] - lx) <= tol * max(1.0, abs(lx))
        assert abs(vals[1] - float(al.fx)) <= tol * max(1.0, abs(lx))
        # the two-kernel form: the two passes over A and f's own products (LeastSquares two, Quadratic one), no one-pass kernel
        assert pr["gemv"]["launches"] + pr["k_gemv_t_mfma"]["launches"] == (4 if which == "ls" else 3)


# ------------------------------------------------------------------ (4) the lifted prox step, element by element
G_KINDS = ["l1", "l1box", "l0box", "lpbox", "indbox"]
D_KINDS = ["zero", "free", "box", "boxvec"]
GAMMA_EL = 0.37


def nonsmooth(bz, ref, g, D, nx, ny, dtype, rng):
    u = np.where(rng.random(nx) < 0.1, 0.0, rng.uniform(0.2, 1.5, nx)).astype(dtype)
    g_d, g_r = {"l1": lambda: (bz.NormL1(0.7), ref.NormL1(0.7)),
                "l1box": lambda: (bz.NormL1Box(0.7, u=u), ref.NormL1Box(0.7, u=u)),
                "l0box": lambda: (bz.NormL0Box(0.7, u=u), ref.NormL0Box(0.7, u=u)),
                "lpbox": lambda: (bz.NormLpPowerBox(0.5, 0.7, u=u), ref.NormLpPowerBox(0.5, 0.7, u=u)),
                "indbox": lambda: (bz.IndBox(-0.5, 0.8), ref.IndBox(dtype(-0.5), dtype(0.8)))}[g]()
    lo = np.where(rng.random(ny) < 0.3, -np.inf, rng.uniform(-1.0, 0.0, ny)).astype(dtype)
    hi = np.where(rng.random(ny) < 0.3, np.inf, rng.uniform(0.0, 1.0, ny)).astype(dtype)
    D_d, D_r = {"zero": lambda: (bz.ZeroSet(), ref.ZeroSet()), "free": lambda: (bz.FreeSet(), ref.FreeSet()),
                "box": lambda: (bz.ClosedSet(bz.IndBox(-0.5, 0.25)), ref.ClosedSet(ref.IndBox(dtype(-0.5), dtype(0.25)))),
                "boxvec": lambda: (bz.ClosedSet(bz.IndBox(lo, hi)), ref.ClosedSet(ref.IndBox(lo, hi)))}[D]()
    return g_d, g_r, D_d, D_r, u


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", [(3, 8), (257, 100)], ids=["3x8", "257x100"])
@pytest.mark.parametrize("D", D_KINDS)
@pytest.mark.parametrize("g", G_KINDS)
def test_lifted_prox_step_element_by_element(bz, ref, g, D, shape, dtype):
    """prox!(z, G::NonsmoothCostFunSlack, ., gamma) (auglagfunslack.jl:136-154) applied to the forward step xs - gamma grad:
    z = [prox_g ; proj_D] bit for bit for the closed-form kinds; for the Newton kind (NormLpPowerBox) the x half follows the
    rule of tests/test_gpu_als_table.py — the same support but for ties, 1e-10 on it in fp64, within 10 x the fp32
    oracle's own distance to the fp64 oracle in fp32 — and the s half is still bit for bit.  The three sums of the
    forward-backward launch (g terms, <grad, res>, ||res||^2) are the same bits on every run."""
    ny, nx = shape
    rng = np.random.default_rng(ny * 5 + nx + G_KINDS.index(g) * 31 + D_KINDS.index(D))
    g_d, g_r, D_d, D_r, u = nonsmooth(bz, ref, g, D, nx, ny, dtype, rng)
    A = (rng.standard_normal((ny, nx)) / np.sqrt(nx)).astype(dtype)
    b = rng.standard_normal(ny).astype(dtype)
    mu = (10.0 ** rng.uniform(-2, 0, ny)).astype(dtype)
    y = rng.standard_normal(ny).astype(dtype)
    xs = (2 * rng.standard_normal(nx + ny)).astype(dtype)
    f_d, f_r = smooth_costs(bz, ref, "diag", nx, dtype, rng)
    F = ref.AugLagFunSlack(f_r, ref.DenseAffine(A, b), mu.copy(), y.copy(), xs[:nx])
    grad = np.empty(nx + ny, dtype)
    F.gradient(grad, xs)
    v = xs - dtype(GAMMA_EL) * grad                       # the forward step
    G = ref.NonsmoothCostFunSlack(g_r, D_r, nx, ny)
    z_ref = np.empty(nx + ny, dtype)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gz_ref = float(G.prox(z_ref, v, dtype(GAMMA_EL)))
    fp64 = dtype == np.float64
    prob = bz.Problem(f_d, g_d, bz.DenseAffine(A, b), D_d, nx, ny, dtype, slack=True)
    try:
        prob.set_multipliers(mu, y)
        prob.profile_reset()
        prob.profile_enable(True)
        z_dev, gz_dev = prob.eval_prox(v, GAMMA_EL)
        pr = prob.profile2()
        assert pr["fb_step"]["launches"] == 1 and pr["fb_step"]["form"] == f"k_fbstep_lifted<LP={int(g == 'lpbox')}>"
        assert z_dev.dtype == dtype and np.array_equal(z_dev[nx:], z_ref[nx:]), "proj_D"
        if g != "lpbox":
            assert np.array_equal(z_dev[:nx], z_ref[:nx]), "prox_g"
            # (fp32: the oracle adds nx non-negative terms in fp32, the device in fp64: the bound of that fp32 sum)
            assert abs(gz_dev - gz_ref) <= (1e-13 if fp64 else nx * float(np.finfo(np.float32).eps)) * max(1.0, abs(gz_ref))
        else:
            zx_d, zx_r = z_dev[:nx], z_ref[:nx]
            same = (zx_d != 0) == (zx_r != 0)
            assert np.mean(same) >= (0.9999 if nx >= 1000 else 1.0)
            if fp64:
                assert np.max(np.abs(zx_d[same] - zx_r[same]), initial=0.0) <= 1e-10
                assert abs(gz_dev - gz_ref) <= 1e-6 * max(1.0, abs(gz_ref))
            else:
                g64 = ref.NormLpPowerBox(0.5, 0.7, u=u.astype(np.float64))
                z64 = np.empty(nx)
                with np.errstate(all="ignore"):
                    g64.prox(z64, v[:nx].astype(np.float64), GAMMA_EL)
                m = same & ((z64 != 0) == (zx_r != 0))
                own = float(np.max(np.abs(zx_r[m] - z64[m]), initial=0.0))
                got = float(np.max(np.abs(zx_d[m] - z64[m]), initial=0.0))
                print(f"fp32 Lp prox: device - fp64 oracle {got:.3e}, fp32 oracle - fp64 oracle {own:.3e}")
                assert got <= 10.0 * max(own, float(np.finfo(np.float32).eps) * float(np.max(np.abs(z64[m]), initial=1.0)))
                # the g value alpha * sum z^p, loosely: with the same support (asserted above for these lengths) and z within
                # the bound just checked, 1e-3 of max(1, |g|) leaves room for fp32 pow on either side and catches a sum that
                # misses or doubles a term (the fp64 branch and the closed-form kinds check it tightly)
                assert abs(gz_dev - gz_ref) <= 1e-3 * max(1.0, abs(gz_ref)), (gz_dev, gz_ref)
        # a solve's first forward-backward launch, twice from the same point: the three sums, bit for bit
        sums = []
        for _ in range(2):
            prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9, gamma=GAMMA_EL).c_opts(), xs)
            sc = prob.panoc_scalars()
            sums.append((sc["g_z"], sc["dot_grad_res"], sc["ss_res"]))
        assert sums[0] == sums[1], sums
        assert np.all(np.isfinite(sums[0]))
        # ... and the state's z is the prox of the forward step the kernel made itself from the device's gradient
        if g != "lpbox":
            z_state, gx = prob.panoc_vector("z"), prob.panoc_vector("grad_x")
            z2 = np.empty(nx + ny, dtype)
            G.prox(z2, xs - dtype(GAMMA_EL) * gx, dtype(GAMMA_EL))
            assert np.array_equal(z_state, z2), "forward step + prox"
            assert np.array_equal(prob.panoc_vector("res"), xs - z2)
    finally:
        prob.close()


# ------------------------------------------------------------------ (5) thirty PANOCplus states against the oracle
def iterate_case(bz, ref, which, dtype):
    """(nx, ny, device oracles, reference oracles, the starting point of x and of s)"""
    if which == "bp":
        ny, nx = 64, 512
        d = bz.synth.basis_pursuit(ny, nx, dtype=dtype, density=0.05)
        dev = (bz.Zero(), bz.NormL1(1.0), bz.DenseAffine(d["A"], d["b"]), bz.ZeroSet())
        orc = (ref.Zero(), ref.NormL1(1.0), ref.DenseAffine(d["A"], d["b"]), ref.ZeroSet())
        return nx, ny, dev, orc, 0.0
    if which == "diag":
        ny, nx = 20, 100
        d = bz.synth.basis_pursuit(ny, nx, dtype=dtype, density=0.05)
        q, fb = (0.5 + bz.synth.uniform(1, nx)).astype(dtype), (2 * bz.synth.uniform(2, nx) - 1).astype(dtype)
        dev = (bz.DiagQuadratic(q, fb), bz.NormL1(0.1), bz.DenseAffine(d["A"], d["b"]), bz.ClosedSet(bz.IndBox(-0.1, 0.2)))
        orc = (ref.DiagQuadratic(q, fb), ref.NormL1(0.1), ref.DenseAffine(d["A"], d["b"]), ref.ClosedSet(ref.IndBox(dtype(-0.1), dtype(0.2))))
        return nx, ny, dev, orc, 1.0
    nx, ny = 40, 2
    p = bz.synth.portfolio(nx, dtype)
    dev = (bz.Quadratic(p["Q"], np.zeros(nx, dtype)), bz.NormL1Box(1.0, u=p["ub"]), bz.DenseAffine(p["A"], p["b"]),
           bz.ClosedSet(bz.IndBox(p["lo"], p["hi"])))
    orc = (ref.Quadratic(p["Q"], np.zeros(nx, dtype)), ref.NormL1Box(1.0, u=p["ub"]), ref.DenseAffine(p["A"], p["b"]),
           ref.ClosedSet(ref.IndBox(p["lo"], p["hi"])))
    return nx, ny, dev, orc, 0.0


@pytest.mark.parametrize("which,dtype", [("bp", np.float64), ("bp", np.float32), ("diag", np.float64), ("portfolio", np.float64)])
def test_iterates_follow_the_oracle(bz, ref, which, dtype):
    """30 states, the oracle stepped on AugLagFunSlack / NonsmoothCostFunSlack: x and z inside max(base, 100 * sens) — base
    1e-9 / 5e-5, sens the oracle's own extended-precision envelope — and gamma equal to 1e-12 / 1e-5 relative (the rule and
    the numbers of test_iterates_follow_the_oracle in tests/test_gpu_sparse.py).  The starting points ([0; 0], [1; 1],
    [0; 0]) are ones from which the oracle's 30 states take tau backtracks (every case) and gamma halvings (at the start
    of every case, and inside an iteration of the last two): the device's counters must show them.  The generic kernel
    chain serves every iteration: no one-pass kernel, no affine images."""
    nx, ny, dev, orc, start = iterate_case(bz, ref, which, dtype)
    mu, y = np.full(ny, 0.1, dtype), (0.1 * np.random.default_rng(2).standard_normal(ny)).astype(dtype)
    xs0 = np.full(nx + ny, start, dtype)
    eps = float(np.finfo(dtype).eps)
    prob = bz.Problem(*dev, nx, ny, dtype, slack=True)
    prob.set_multipliers(mu, y)
    prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=eps).c_opts(), xs0)
    its, sts = [], []
    for red in (None, LongDoubleReducer()):
        ref.set_reducer(red)
        F = ref.AugLagFunSlack(orc[0], orc[2], mu.copy(), y.copy(), xs0[:nx])
        it = ref.PANOCplusIteration(F, ref.NonsmoothCostFunSlack(orc[1], orc[3], nx, ny), xs0, minimum_gamma=eps)
        its.append(it)
        sts.append(it.init())
    ref.set_reducer(None)
    base = 1e-9 if dtype == np.float64 else 5e-5
    env, rows, bt_ref = 0.0, [], 0
    for k in range(30):
        st = sts[0]
        env = max(env, _err(sts[1].x, st.x), _err(sts[1].z, st.z))
        rows.append((k + 1, _err(prob.panoc_vector("x"), st.x), _err(prob.panoc_vector("z"), st.z),
                     prob.panoc_scalars()["gamma"], float(st.gamma), env))
        if k + 1 < 30:
            prob.panoc_step()
            sts[0] = its[0].step(sts[0])
            bt_ref += sts[0].n_backtracks
            ref.set_reducer(LongDoubleReducer())
            sts[1] = its[1].step(sts[1])
            ref.set_reducer(None)
    stats = prob.panoc_stats()
    prob.close()
    for k, ex, ez, g_d, g_r, sens in rows:
        print(f"k={k} ex={ex:.3e} ez={ez:.3e} gamma {g_d:.9g} / {g_r:.9g} sens={sens:.3e}")
    print(f"tau backtracks {stats.n_backtracks} (oracle {bt_ref}), gamma halvings {stats.n_gamma_halvings} (oracle {sts[0].n_gamma_halvings})")
    for k, ex, ez, g_d, g_r, sens in rows:
        assert abs(g_d - g_r) <= (1e-12 if dtype == np.float64 else 1e-5) * g_r, k
        assert ex <= max(base, 100 * sens) and ez <= max(base, 100 * sens), (k, ex, ez, sens)
    assert bt_ref >= 1 and sts[0].n_gamma_halvings >= 1          # (what the starting points were chosen for)
    assert stats.n_backtracks >= 1 and stats.n_gamma_halvings >= 1
    assert stats.n_fused_iters == 0 and stats.n_affine_images == 0 and stats.n_dense_onepass == 0


# ------------------------------------------------------------------ (6) whole solves
def portfolio_oracles(bz, ref, n, g, lam):
    p = bz.synth.portfolio(n)
    gd, gr = {"l1": lambda: (bz.NormL1Box(lam, u=p["ub"]), ref.NormL1Box(lam, u=p["ub"])),
              "l0": lambda: (bz.NormL0Box(lam, u=p["ub"]), ref.NormL0Box(lam, u=p["ub"])),
              "lp": lambda: (bz.NormLpPowerBox(0.5, lam, u=p["ub"]), ref.NormLpPowerBox(0.5, lam, u=p["ub"]))}[g]()
    dev = (bz.Quadratic(p["Q"], np.zeros(n)), gd, bz.DenseAffine(p["A"], p["b"]), bz.ClosedSet(bz.IndBox(p["lo"], p["hi"])))
    orc = (ref.Quadratic(p["Q"], np.zeros(n)), gr, ref.DenseAffine(p["A"], p["b"]), ref.ClosedSet(ref.IndBox(p["lo"], p["hi"])))
    return p, dev, orc


def solve_case(bz, ref, which):
    """(nx, ny, device oracles, reference oracles, x0, objective, c, proj_D, subsolver keywords, als keywords)"""
    long_sub = dict(maxit=100000, minimum_gamma=2.3e-16)
    if which in ("bp-20x100", "bp-3x8"):
        ny, nx = (20, 100) if which == "bp-20x100" else (3, 8)
        d = bz.synth.basis_pursuit(ny, nx, dtype=np.float64, density=0.05)
        dev = (bz.Zero(), bz.NormL1(1.0), bz.DenseAffine(d["A"], d["b"]), bz.ZeroSet())
        orc = (ref.Zero(), ref.NormL1(1.0), ref.DenseAffine(d["A"], d["b"]), ref.ZeroSet())
        return (nx, ny, dev, orc, np.zeros(nx), lambda x: float(np.sum(np.abs(x))), lambda x: d["A"] @ x - d["b"],
                lambda v: np.zeros_like(v), long_sub, dict(subsolver_maxit=100000))
    if which == "diag-20x100":
        ny, nx = 20, 100
        d = bz.synth.basis_pursuit(ny, nx, dtype=np.float64, density=0.05)
        q, fb = 0.5 + bz.synth.uniform(1, nx), 2 * bz.synth.uniform(2, nx) - 1
        dev = (bz.DiagQuadratic(q, fb), bz.NormL1(0.1), bz.DenseAffine(d["A"], d["b"]), bz.ClosedSet(bz.IndBox(-0.1, 0.2)))
        orc = (ref.DiagQuadratic(q, fb), ref.NormL1(0.1), ref.DenseAffine(d["A"], d["b"]), ref.ClosedSet(ref.IndBox(-0.1, 0.2)))
        return (nx, ny, dev, orc, np.zeros(nx), lambda x: float(np.sum(x * (0.5 * q * x - fb)) + 0.1 * np.sum(np.abs(x))),
                lambda x: d["A"] @ x - d["b"], lambda v: np.clip(v, -0.1, 0.2), long_sub, dict(subsolver_maxit=100000))
    n = int(which.split("-")[1])
    p, dev, orc = portfolio_oracles(bz, ref, n, "l1", 1.0)
    # x0 = ones, y0 = 0, subsolver maxit = 1000, minimum_gamma = 1e-32: as demo/portfolio.jl:129-139,168-169 sets them
    return (n, 2, dev, orc, np.ones(n), lambda x: float(0.5 * x @ p["Q"] @ x + np.sum(x)), lambda x: p["A"] @ x - p["b"],
            lambda v: np.clip(v, p["lo"], p["hi"]), dict(maxit=1000, minimum_gamma=1e-32), {})


REF_SOLVES = {}          # the oracle's solves, computed once and shared (never changed)


def ref_solve(ref, key, fn, orc, x0, ny, sub_kw, kw):
    if key not in REF_SOLVES:
        REF_SOLVES[key] = fn(*orc, x0.copy(), np.zeros(ny), subsolver=lambda **k: ref.PANOCplus(**sub_kw, **k), **kw)
    return REF_SOLVES[key]


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host-loop"])
@pytest.mark.parametrize("which", ["bp-20x100", "bp-3x8", "diag-20x100", "portfolio-40", "portfolio-200"])
def test_whole_solves(bz, ref, which, resident):
    """bz.als, resident and through the host outer loop, against ref.als: first_order on both sides, feasibility
    ||c(x) - proj_D(c(x))||_inf <= 1e-5, objective within 1e-4 relative, x within 1e-4 (the bounds of test_whole_solves in
    tests/test_gpu_sparse.py).  Iteration counts are printed, not compared."""
    nx, ny, dev, orc, x0, obj, cfun, proj, sub_kw, kw = solve_case(bz, ref, which)
    o = ref_solve(ref, ("als", which), ref.als, orc, x0, ny, sub_kw, kw)
    assert o[5] == "first_order"
    a = bz.als(*dev, x0, np.zeros(ny), subsolver=lambda **k: bz.PANOCplus(**sub_kw, **k), resident=resident, **kw)
    cx = cfun(a[0])
    feas = float(np.max(np.abs(cx - proj(cx))))
    print(f"{which} resident={resident}: status {a[5]} outer {a[2]}/{o[2]} inner {a[3]}/{o[3]} feas {feas:.3e} "
          f"obj {obj(a[0]):.9g}/{obj(o[0]):.9g} max|x - x_ref| {np.max(np.abs(a[0] - o[0])):.3e}")
    assert a[5] == "first_order"
    assert feas <= 1e-5
    assert abs(obj(a[0]) - obj(o[0])) <= 1e-4 * abs(obj(o[0]))
    assert np.max(np.abs(a[0] - o[0])) <= 1e-4
    assert a[0].shape == (nx,) and a[1].shape == a[8].shape == a[9].shape == (ny,)
    assert np.max(np.abs(a[8] - proj(a[8]))) == 0.0          # the slack certificate s lies in D
    assert not np.any(x0 - x0[0])                            # x0 is never mutated


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host-loop"])
@pytest.mark.parametrize("g", ["l0", "lp"])
def test_whole_solves_nonconvex_portfolio(bz, ref, g, resident):
    """NormL0Box and NormLpPowerBox on the portfolio problem, n = 40: another rounding may end in another stationary point,
    so x and the objective are not compared with the oracle's — status first_order, the feasibility bound, and sum(x) = 1,
    mu'x >= rho, 0 <= x <= ub, each to 1e-5.  The weight is 1e-4: the prox of NormL0Box (normL0Box.jl:33-58) keeps an entry
    above its bound u wherever y^2 > gamma lambda + (u - y)^2, so with a heavy weight its stationary points concentrate
    the budget on a few assets beyond ub — on the oracle too (lambda = 1: two assets, 0.34 over the bound); with 1e-4
    the oracle's stationary point holds 21 assets, all at least 0.014 below their bounds."""
    n, lam = 40, 1e-4
    p, dev, orc = portfolio_oracles(bz, ref, n, g, lam)
    sub_kw = dict(maxit=1000, minimum_gamma=1e-32)
    o = ref_solve(ref, ("als", g), ref.als, orc, np.ones(n), 2, sub_kw, {})
    assert o[5] == "first_order"
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = bz.als(*dev, np.ones(n), np.zeros(2), subsolver=lambda **k: bz.PANOCplus(**sub_kw, **k), resident=resident)
    x = a[0]
    cx = p["A"] @ x - p["b"]
    feas = float(np.max(np.abs(cx - np.clip(cx, p["lo"], p["hi"]))))
    print(f"{g} resident={resident}: status {a[5]} outer {a[2]}/{o[2]} inner {a[3]}/{o[3]} feas {feas:.3e} sum(x) - 1 {x.sum() - 1:.3e} "
          f"mu'x - rho {p['mu'] @ x - p['rho']:.3e} nnz {np.count_nonzero(x)}/{np.count_nonzero(o[0])} max(x - ub) {np.max(x - p['ub']):.3e}")
    assert a[5] == "first_order"
    assert feas <= 1e-5
    assert abs(x.sum() - 1) <= 1e-5 and p["mu"] @ x >= p["rho"] - 1e-5
    assert x.min() >= -1e-5 and np.max(x - p["ub"]) <= 1e-5


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host-loop"])
def test_alps_with_a_dense_f_beside_a_dense_c(bz, ref, resident):
    """bz.alps with Quadratic + DenseAffine (portfolio n = 40, NormL1Box) against ref.alps, to the bounds of the whole solves"""
    n = 40
    p, dev, orc = portfolio_oracles(bz, ref, n, "l1", 1.0)
    sub_kw = dict(maxit=1000, minimum_gamma=1e-32)
    o = ref_solve(ref, ("alps", "l1"), ref.alps, orc, np.ones(n), 2, sub_kw, {})
    assert o[5] == "first_order"
    a = bz.alps(*dev, np.ones(n), np.zeros(2), subsolver=lambda **k: bz.PANOCplus(**sub_kw, **k), resident=resident)
    obj = lambda x: float(0.5 * x @ p["Q"] @ x + np.sum(x))
    cx = p["A"] @ a[0] - p["b"]
    feas = float(np.max(np.abs(cx - np.clip(cx, p["lo"], p["hi"]))))
    print(f"alps resident={resident}: status {a[5]} outer {a[2]}/{o[2]} inner {a[3]}/{o[3]} feas {feas:.3e} "
          f"obj {obj(a[0]):.9g}/{obj(o[0]):.9g} max|x - x_ref| {np.max(np.abs(a[0] - o[0])):.3e}")
    assert a[5] == "first_order"
    assert feas <= 1e-5
    assert abs(obj(a[0]) - obj(o[0])) <= 1e-4 * abs(obj(o[0]))
    assert np.max(np.abs(a[0] - o[0])) <= 1e-4
