"""The slack (ALS) form with a dense affine constraint and a dense f beside a dense c: what can be checked without a
GPU — the lowering into the problem descriptor, the combinations refused before any device call, the portfolio
generator of bz.synth, and the host mirrors of AugLagFunSlack / NonsmoothCostFunSlack on halves of unequal length."""
import numpy as np
import pytest


def _matrix(ny, n, dtype=np.float64):
    rng = np.random.default_rng(ny * 13 + n)
    return rng.standard_normal((ny, n)).astype(dtype), rng.standard_normal(ny).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("fk", ["zero", "diag", "quadratic", "ls"])
def test_lowering_of_the_slack_form_with_a_dense_c(bz, fk, dtype):
    from bazinga_jl_amd.oracles import lower
    L = bz._lib
    ny, n = 3, 8
    A, b = _matrix(ny, n, dtype)
    rng = np.random.default_rng(1)
    Q = rng.standard_normal((n, n))
    FA, fb = _matrix(5, n, dtype)
    f, kind = {"zero": (bz.Zero(), L.BZ_F_ZERO),
               "diag": (bz.DiagQuadratic(np.ones(n, dtype), np.zeros(n, dtype)), L.BZ_F_DIAG_QUADRATIC),
               "quadratic": (bz.Quadratic((Q @ Q.T).astype(dtype), np.zeros(n, dtype)), L.BZ_F_QUADRATIC),
               "ls": (bz.LeastSquares(FA, fb), L.BZ_F_LEAST_SQUARES)}[fk]
    D = bz.ClosedSet(bz.IndBox(np.array([-1.0, -np.inf, 0.0], dtype), np.array([1.0, 2.0, np.inf], dtype)))
    for slack in (True, False):
        d, keep = lower(f, bz.NormL1Box(1.0, u=np.ones(n, dtype)), bz.DenseAffine(A, b), D, n, ny, dtype, slack=slack)
        assert d.slack == int(slack) and d.c_kind == L.BZ_C_DENSE_AFFINE and d.f_kind == kind
        assert (d.n, d.ny) == (n, ny) and d.c_A and d.c_b and d.D_kind == L.BZ_D_BOX and d.D_lo_vec and d.D_hi_vec
        assert d.dtype == (L.BZ_F64 if dtype == np.float64 else L.BZ_F32)
        if fk == "quadratic":
            assert d.f_rows == n and d.f_A and d.f_b
        if fk == "ls":
            assert d.f_rows == 5 and d.f_A and d.f_b
        if fk == "diag":
            assert d.f_q and d.f_b


def test_refusals_before_any_device_call(bz):
    """what is refused before any device call raises UnsupportedOracle in lower(), the first thing bz.Problem does: the slack
    form with a sparse c or with callbacks, a dense f beside a sparse c, als(resident=False, warm_start=True).  The stencil
    f, the pairwise sets, more than one rank and the pack rule on nx in the slack form are the library's own refusals
    (BazingaHipError, pinned by the GPU tests), so lower() lets them through unchanged."""
    from bazinga_jl_amd.oracles import lower
    L = bz._lib
    n = 8
    A, b = _matrix(3, n)
    sp = bz.SparseAffine.from_dense(A, b)
    Q = np.eye(n)
    g = bz.NormL1(1.0)
    cases = [
        (bz.Zero(), sp, bz.ZeroSet(), 3, True),                                                   # slack with a sparse c
        (bz.Quadratic(Q, np.zeros(n)), sp, bz.ZeroSet(), 3, False),                                # dense f beside a sparse c
        (bz.LeastSquares(A, b), sp, bz.ZeroSet(), 3, False),
    ]
    d, keep = lower(bz.Stencil5ptQuadratic(2, 4, np.zeros(n)), g, bz.IdentityFunction(), bz.FreeSet(), n, n, np.float64, slack=True)
    assert d.slack == 1 and d.f_kind == L.BZ_F_STENCIL5                                            # (the library refuses it)
    d, keep = lower(bz.Zero(), bz.Zero(), bz.IdentityFunction(), bz.PairwiseSet("cc"), n, n, np.float64, slack=True)
    assert d.slack == 1 and d.D_kind == L.BZ_D_CC_PAIRS
    for f, c, D, ny, slack in cases:
        with pytest.raises(bz.UnsupportedOracle):
            lower(f, g, c, D, n, ny, np.float64, slack=slack)
        with pytest.raises(bz.UnsupportedOracle):
            bz.Problem(f, g, c, D, n, ny, np.float64, slack=slack)

    class Generic:
        def gradient(self, dfx, x):
            dfx[...] = 0
            return 0.0

    with pytest.raises(bz.UnsupportedOracle):                                                      # slack with callbacks
        lower(Generic(), g, bz.DenseAffine(A, b), bz.ZeroSet(), n, 3, np.float64, slack=True)
    with pytest.raises(bz.UnsupportedOracle):                                                      # als(resident=False, warm_start=True)
        bz.als(bz.Zero(), g, bz.DenseAffine(A, b), bz.ZeroSet(), np.zeros(n), np.zeros(3), resident=False, warm_start=True)


@pytest.mark.parametrize("n", [40, 200])
def test_portfolio_generator(bz, n):
    a, b = bz.synth.portfolio(n), bz.synth.portfolio(n)
    for k in a:
        assert np.array_equal(a[k], b[k]), k                    # reproducible
    Q, mu, ub, rho = a["Q"], a["mu"], a["ub"], a["rho"]
    assert Q.shape == (n, n) and mu.shape == ub.shape == (n,)
    assert np.array_equal(Q, Q.T) and np.linalg.eigvalsh(Q).min() > 0
    assert mu.min() >= 0 and mu.max() <= 0.1 and ub.min() > 0
    # the set {sum x = 1, mu'x >= rho, 0 <= x <= ub} holds the generator's own point, and the return constraint cuts:
    # the uniform spread ub/sum(ub) misses it
    x = a["xfeas"]
    assert abs(x.sum() - 1) <= 1e-14 and mu @ x >= rho - 1e-15 and x.min() >= 0 and np.all(x <= ub + 1e-16)
    assert mu @ (ub / ub.sum()) < rho
    # the demo's constraint as matrices: c(x) = [mu'x; e'x], D = [rho, inf) x {1}
    assert np.array_equal(a["A"], np.stack([mu, np.ones(n)])) and not a["b"].any()
    assert np.array_equal(a["lo"], [rho, 1.0]) and np.array_equal(a["hi"], [np.inf, 1.0])
    f32 = bz.synth.portfolio(n, np.float32)
    assert f32["Q"].dtype == np.float32 and np.array_equal(f32["Q"], Q.astype(np.float32))
    # a different length is a different prefix of the same stream, not a reshuffle of it
    assert np.array_equal(bz.synth.portfolio(n + 1)["mu"][:n], mu)


def test_host_mirrors_on_halves_of_unequal_length(bz, ref):
    """AugLagFunSlack / NonsmoothCostFunSlack of bz.solvers carry (nx, ny) with nx != ny and the scalar caches the outer
    loop reads; the oracle's functors on the same data accept the lifted vector of length nx + ny and no other"""
    nx, ny = 8, 3
    A, b = _matrix(ny, nx)
    rng = np.random.default_rng(4)
    mu, y, x = 10.0 ** rng.uniform(-2, 0, ny), rng.standard_normal(ny), rng.standard_normal(nx)
    F = bz.AugLagFunSlack(bz.Zero(), bz.DenseAffine(A, b), mu, y, x)
    G = bz.NonsmoothCostFunSlack(bz.NormL1(1.0), bz.ZeroSet(), nx, ny)
    assert (F.nx, F.ny) == (nx, ny) == (G.nx, G.ny)
    assert F.muy.shape == (ny,) and np.array_equal(F.muy, mu * y) and F.musqy == 0.5 * np.sum(mu * y * y)
    with pytest.raises(ValueError):
        bz.AugLagFunSlack(bz.Zero(), bz.DenseAffine(A, b), -mu, y, x)
    Fr = ref.AugLagFunSlack(ref.Zero(), ref.DenseAffine(A, b), mu.copy(), y.copy(), x)
    Gr = ref.NonsmoothCostFunSlack(ref.NormL1(1.0), ref.ZeroSet(), nx, ny)
    xs = rng.standard_normal(nx + ny)
    g = np.empty(nx + ny)
    val = Fr.gradient(g, xs)
    cx = A @ xs[:nx] - b
    yupd = y + (cx - xs[nx:]) / mu
    assert np.allclose(g[:nx], A.T @ yupd, rtol=0, atol=1e-13) and np.array_equal(g[nx:], -yupd)
    assert abs(val - (0.5 * np.sum((cx + mu * y - xs[nx:]) ** 2 / mu) - 0.5 * np.sum(mu * y * y))) <= 1e-12
    z = np.empty(nx + ny)
    Gr.prox(z, xs, 0.3)
    assert not z[nx:].any() and np.array_equal(z[:nx], np.sign(xs[:nx]) * np.maximum(np.abs(xs[:nx]) - 0.3, 0))
    for bad in (nx + nx, ny + ny):
        with pytest.raises(ValueError):
            Fr.gradient(np.empty(bad), np.empty(bad))
        with pytest.raises(ValueError):
            Gr.prox(np.empty(bad), np.empty(bad), 0.3)
