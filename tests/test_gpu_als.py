"""ALS — the slack-variable sibling of ALPS (src/algorithms/als.jl, src/utilities/auglagfunslack.jl;
SURVEY.md §8(f-3)) — through the device path, against the CPU oracle's restatement of the same files."""
import numpy as np
import pytest

from tests.test_gpu_parity import RTOL_ITER, LongDoubleReducer, iter_tol, make_cfg2, rel

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [2, 1000, 70002])
@pytest.mark.parametrize("D", ["box", "free", "zero"])
def test_slack_gradient_and_prox_bit_exact(bz, ref, n, D):
    """gradient!(dFxs, F::AugLagFunSlack, xs) (auglagfunslack.jl:78-97) and
    prox!(z, G::NonsmoothCostFunSlack, xs, gamma) (:136-154): element-wise bit-exact."""
    d, dev, orc = make_cfg2(bz, ref, n, D=D)
    rng = np.random.default_rng(n + 3)
    xs = rng.standard_normal(2 * n)
    mu = 10.0 ** rng.uniform(-2, 0, n)
    y = rng.standard_normal(n)
    prob = bz.Problem(*dev, n, n, np.float64, slack=True)
    prob.set_multipliers(mu, y)
    g_dev, vals = prob.eval_al_gradient(xs)
    F = ref.AugLagFunSlack(orc[0], orc[2], mu.copy(), y.copy(), xs[:n])
    g_ref = np.empty(2 * n)
    Fxs = F.gradient(g_ref, xs)
    assert np.array_equal(g_dev, g_ref)
    assert abs(vals[0] - Fxs) <= 1e-13 * max(1.0, abs(Fxs))
    z_dev, gz_dev = prob.eval_prox(xs, 0.41)
    G = ref.NonsmoothCostFunSlack(orc[1], orc[3], n, n)
    z_ref = np.empty(2 * n)
    gz_ref = G.prox(z_ref, xs, 0.41)
    assert np.array_equal(z_dev, z_ref)
    assert abs(gz_dev - gz_ref) <= 1e-13 * max(1.0, abs(gz_ref))
    prob.close()


@pytest.mark.parametrize("n,dt", [(1000, "float64"), (400002, "float64"), (1000, "float32"), (400004, "float32")],
                         ids=["1000", "400002", "1000-f32", "400004-f32"])
def test_slack_panoc_iterates_match_oracle(bz, ref, n, dt):
    """fp32 (the same kernels in the other type, hardware quotients instead of div_u): the rule of the family table — x and
    z within max(2e-5, 100 x the oracle's own rounding sensitivity), gamma to 1e-5 while that tolerance is still 2e-5, and
    at least 10 of the 25 states compared within 1e-3."""
    dtype = np.dtype(dt).type
    fp64 = dtype == np.float64
    d, dev, orc = make_cfg2(bz, ref, n, dtype=dtype)
    rng = np.random.default_rng(8)
    mu, y = np.full(n, 0.1, dtype), rng.standard_normal(n).astype(dtype)
    xs0 = np.concatenate([np.zeros(n), np.clip(rng.standard_normal(n), -1, 1)]).astype(dtype)
    prob = bz.Problem(*dev, n, n, dtype, slack=True)
    prob.set_multipliers(mu, y)
    prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9).c_opts(), xs0)
    its, sts = [], []
    for red in (None, LongDoubleReducer()):
        ref.set_reducer(red)
        F = ref.AugLagFunSlack(orc[0], orc[2], mu.copy(), y.copy(), xs0[:n])
        it = ref.PANOCplusIteration(F, ref.NonsmoothCostFunSlack(orc[1], orc[3], n, n), xs0)
        its.append(it)
        sts.append(it.init())
    ref.set_reducer(None)
    env = 0.0
    tight = 0
    for k in range(25):
        env = max(env, rel(sts[1].x, sts[0].x), rel(sts[1].z, sts[0].z))
        ex, ez = rel(prob.panoc_vector("x"), sts[0].x), rel(prob.panoc_vector("z"), sts[0].z)
        if fp64:
            assert ex <= iter_tol(env) and ez <= iter_tol(env), (k, ex, ez, env)
            if k < 10:
                assert ex <= RTOL_ITER and ez <= RTOL_ITER
        else:
            tol = max(2e-5, 100 * env)
            print("fp32 slack state %d: x %.3e z %.3e (tol %.3e)" % (k, ex, ez, tol))
            assert ex <= tol and ez <= tol, (k, ex, ez, env)
            if tol == 2e-5:
                g_d, g_r = prob.panoc_scalars()["gamma"], float(sts[0].gamma)
                assert abs(g_d - g_r) <= 1e-5 * g_r, (k, g_d, g_r)
            tight += tol <= 1e-3
        prob.panoc_step()
        sts[0] = its[0].step(sts[0])
        ref.set_reducer(LongDoubleReducer())
        sts[1] = its[1].step(sts[1])
        ref.set_reducer(None)
    assert fp64 or tight >= 10, tight
    prob.close()


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_slack_form_refuses_a_length_that_is_not_whole_packs(bz, ref, dt):
    """The slack kernels work on 16-byte packs of each half of [x; s]: creation refuses nx that is not a multiple of the
    pack (2 fp64 / 4 fp32 elements) with BZ_ERR_ARG, and takes the next multiple."""
    dtype = np.dtype(dt).type
    pk = 16 // np.dtype(dtype).itemsize
    for n in (pk + 1, 1001 if pk == 2 else 1002, 40 * pk - 1):
        assert n % pk
        d, dev, orc = make_cfg2(bz, ref, n, dtype=dtype)
        with pytest.raises(bz.BazingaHipError) as e:
            bz.Problem(*dev, n, n, dtype, slack=True)
        assert e.value.code == bz._lib.BZ_ERR_ARG and "multiple of 16 bytes" in str(e.value), str(e.value)
    d, dev, orc = make_cfg2(bz, ref, 40 * pk, dtype=dtype)
    bz.Problem(*dev, 40 * pk, 40 * pk, dtype, slack=True).close()


@pytest.mark.parametrize("resident", [True, False])
def test_als_matches_oracle_and_alps(bz, ref, resident):
    n = 3000
    d, dev, orc = make_cfg2(bz, ref, n)
    x0, y0 = np.zeros(n), np.zeros(n)
    a = bz.als(*dev, x0, y0, resident=resident)
    o = ref.als(*orc, x0, y0)
    assert a[5] == o[5] == "first_order"
    assert a[2] == o[2]
    assert abs(a[3] - o[3]) <= max(3, 0.03 * o[3])
    assert rel(a[0], o[0]) <= 1e-7
    assert np.max(np.abs(a[1] - o[1])) <= 1e-6 * max(1.0, np.max(np.abs(o[1])))
    assert np.max(np.abs(a[8] - o[8])) <= 1e-6                       # slack certificate s
    b = bz.alps(*dev, x0, y0)                                        # same minimiser as ALPS
    assert np.max(np.abs(a[0] - b[0])) <= 1e-5
    assert not np.any(x0)


@pytest.mark.parametrize("D", ["box", "free"])
@pytest.mark.parametrize("n", [4098, 150_001 * 2])
def test_fused_slack_pass_follows_the_kernel_chain(bz, ref, n, D):
    """k_fused_slack (the whole ALS inner iteration on [x; s] in one pass, compact L-BFGS form) against the kernel chain
    (fuse = False: k_compact_xd, k_algrad_slack_elem x 2, k_fbstep_slack, k_update_c): the same element arithmetic,
    reductions over the index instead of over the lifted vector — 40 states agree to rounding, the one-pass kernel
    serves the iterations, and the oracle's ALS inner iterates are followed to the north-star tolerance."""
    d, dev, orc = make_cfg2(bz, ref, n, D=D)
    rng = np.random.default_rng(5)
    mu, y = np.full(n, 0.1), 0.3 * rng.standard_normal(n)
    xs0 = np.concatenate([0.05 * rng.standard_normal(n), np.zeros(n)])
    runs = []
    for fuse in (True, False):
        prob = bz.Problem(*dev, n, n, np.float64, slack=True)
        prob.set_multipliers(mu, y)
        prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9, fuse=fuse, minimum_gamma=float(np.finfo(float).eps)).c_opts(), xs0)
        prob.profile_enable(True)
        tr = []
        for k in range(40):
            prob.panoc_step()
            if k in (0, 5, 15, 39):
                tr.append((prob.panoc_vector("x"), prob.panoc_scalars()))
        runs.append((tr, prob.panoc_stats(), prob.profile2()))
        prob.close()
    (ta, sa, pa), (tb, sb, pb) = runs
    assert sa.n_fused_iters >= 30 and sb.n_fused_iters == 0
    # (the iterate-history pass from the first iteration on — an empty memory is m = 0 iterates behind the current one; the
    # stored-pair pass k_fused_slack only after a broken run of plain iterations)
    assert pa["k_fused_iterates"]["form"].startswith("k_fused_slack_xr")
    assert pa["k_fused_sep"]["launches"] + pa["k_fused_iterates"]["launches"] >= 30 and pa["k_fused_iterates"]["launches"] >= 20
    for (xa, ca), (xb, cb) in zip(ta, tb):
        assert ca["gamma"] == cb["gamma"] and ca["lbfgs_mem"] == cb["lbfgs_mem"]
        assert np.max(np.abs(xa - xb)) <= 1e-10 * max(1.0, np.max(np.abs(xb)))
        assert abs(ca["stop_norm"] - cb["stop_norm"]) <= 1e-8 * max(1.0, cb["stop_norm"])
    # ... and the oracle
    al = ref.AugLagFunSlack(orc[0], orc[2], mu.copy(), y.copy(), xs0[:n])
    it = ref.PANOCplusIteration(al, ref.NonsmoothCostFunSlack(orc[1], orc[3], n, n), xs0,
                                minimum_gamma=float(np.finfo(float).eps))
    st = it.init()
    for k in range(16):
        st = it.step(st)
    assert np.max(np.abs(ta[2][0] - st.x)) <= 1e-10 * max(1.0, np.max(np.abs(st.x)))


def test_als_long_subproblems_through_the_fused_pass(bz, ref):
    """Subproblems of several hundred iterations (the one-pass kernel then keeps z in registers: the outer loop must ask
    for it — it once read a stale buffer here, tests/stress/stress_als.py seed 26): the closed form of min f + g when D is
    the whole space, the oracle's counts loosely (the usual chaos of long subsolves), its point to the solve's tolerance."""
    rng = np.random.default_rng(7026)
    n = 4834
    q, b = rng.uniform(0.2, 5.0, n), rng.standard_normal(n) * 4
    lam = 1.7
    x0, y0 = rng.standard_normal(n) * 0.1, rng.standard_normal(n) * 0.1
    o = ref.als(ref.DiagQuadratic(q, b), ref.NormL1(lam), ref.IdentityFunction(), ref.FreeSet(), x0, y0, maxit=40)
    a = bz.als(bz.DiagQuadratic(q, b), bz.NormL1(lam), bz.IdentityFunction(), bz.FreeSet(), x0, y0, maxit=40)
    xs = np.sign(b) * np.maximum(np.abs(b) - lam, 0) / q
    assert a[5] == o[5] == "first_order" and abs(a[2] - o[2]) <= 1
    assert o[3] >= 1000 and abs(a[3] - o[3]) <= 0.3 * o[3]
    assert np.max(np.abs(a[0] - xs)) <= 2e-5 and np.max(np.abs(a[0] - o[0])) <= 2e-5


def test_als_warm_start_matches_the_warm_started_oracle(bz, ref):
    """als(warm_start=True) (bz_alps_opts.warm_start through bz_als_solve): the step size carried across subproblems, as
    in alps — the resident loop against the oracle restated with the same option; the host loop refuses it."""
    n = 3000
    d, dev, orc = make_cfg2(bz, ref, n)
    x0, y0 = np.zeros(n), np.zeros(n)
    a = bz.als(*dev, x0, y0, resident=True, warm_start=True)
    o = ref.als(*orc, x0, y0, warm_start=True)
    cold = ref.als(*orc, x0, y0)
    assert a[5] == o[5] == "first_order" and a[2] == o[2]
    assert abs(a[3] - o[3]) <= max(3, 0.03 * o[3])
    assert rel(a[0], o[0]) <= 1e-7 and rel(a[0], cold[0]) <= 1e-4
    with pytest.raises(bz.UnsupportedOracle):
        bz.als(*dev, x0, y0, resident=False, warm_start=True)


def test_als_rejects_unsupported(bz, ref):
    n = 64
    d = bz.synth.obstacle_grid(8, 8)
    with pytest.raises(bz.BazingaHipError):
        bz.Problem(bz.Stencil5ptQuadratic(8, 8, d["b"]), bz.Zero(), bz.IdentityFunction(), bz.FreeSet(), n, n,
                   np.float64, slack=True)
    d2, dev, orc = make_cfg2(bz, ref, n)
    prob = bz.Problem(*dev, n, n, np.float64)
    ao, po = bz._lib.AlpsOpts(), bz.PANOCplus().c_opts()
    prob.slack = True                       # force the ALS entry point onto an ALPS problem
    import ctypes as C
    bz._lib.load().bz_alps_default_opts(C.byref(ao), 0)
    with pytest.raises(bz.BazingaHipError):
        prob.alps_solve(ao, po, np.zeros(n), np.zeros(n))
    prob.slack = False
    prob.close()


def test_als_with_compact_lbfgs_and_no_acceleration(bz, ref):
    """The slack path has no fused kernel: with the compact L-BFGS form every iteration takes the generic
    route (k_gram_dots + read-back for p, w; k_compact_xd for x_d).  Same minimiser as the oracle's ALS; and
    `NoAcceleration` (demo/rosenbrock.jl:96-97) on the slack problem as well."""
    n = 2000
    d, dev, orc = make_cfg2(bz, ref, n)
    x0, y0 = np.zeros(n), np.zeros(n)
    o = ref.als(*orc, x0, y0)
    a = bz.als(*dev, x0, y0, subsolver=lambda **kw: bz.PANOCplus(directions=bz.LBFGS(5, compact=True), **kw), resident=True)
    assert a[5] == o[5] == "first_order" and a[2] == o[2]
    assert abs(a[3] - o[3]) <= max(3, 0.1 * o[3])
    assert rel(a[0], o[0]) <= 1e-6
    o2 = ref.als(*orc, x0, y0, subsolver=lambda **kw: ref.PANOCplus(directions=ref.NoAcceleration(), **kw))
    a2 = bz.als(*dev, x0, y0, subsolver=lambda **kw: bz.PANOCplus(directions=bz.NoAcceleration(), **kw), resident=True)
    assert a2[5] == o2[5] and a2[2] == o2[2] and abs(a2[3] - o2[3]) <= max(3, 0.1 * o2[3])
    assert rel(a2[0], o2[0]) <= 1e-6


@pytest.mark.timeout(300)
@pytest.mark.parametrize("g,D,dt", [(g, D, dt) for dt in ("float64", "float32") for g, D in (("l1", "box"), ("l1", "free"), ("zero", "box"))],
                         ids=["l1-box", "l1-free", "zero-box", "l1-box-f32", "l1-free-f32", "zero-box-f32"])
def test_als_with_zero_smooth_cost_terminates_like_the_reference(bz, ref, g, D, dt):
    """f = Zero in the slack form: grad F(xs + 1) = grad F(xs), so `lower_bound_smoothness_constant` is 0 and gamma = alpha / 0 =
    inf.  The reference's step-size loop compares NaNs there and leaves; its solve then runs on NaN iterates to the subsolver's
    iteration cap and `als` ends with :exception, or :max_iter when the objective stays a number (als.jl:68-72,96-110).  The
    device loop once halved the infinite gamma for ever (a hang, fixed in r02 `71ac09b` with no test: VERDICT r02 item 1(d)):
    it must terminate, with the oracle's status and counts."""
    import warnings
    n = 400
    T = np.dtype(dt).type
    rng = np.random.default_rng(11)
    x0, y0 = (0.1 * rng.standard_normal(n)).astype(T), (0.1 * rng.standard_normal(n)).astype(T)
    g_d, g_r = (bz.NormL1(0.5), ref.NormL1(T(0.5))) if g == "l1" else (bz.Zero(), ref.Zero())
    D_d, D_r = ((bz.ClosedSet(bz.IndBox(-0.5, 0.7)), ref.ClosedSet(ref.IndBox(T(-0.5), T(0.7)))) if D == "box"
                else (bz.FreeSet(), ref.FreeSet()))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        o = ref.als(ref.Zero(), g_r, ref.IdentityFunction(), D_r, x0, y0, maxit=4)
    a = bz.als(bz.Zero(), g_d, bz.IdentityFunction(), D_d, x0, y0, maxit=4)
    assert o[5] in ("exception", "max_iter")
    assert a[5] == o[5] and a[2] == o[2] and a[3] == o[3], (a[5], a[2], a[3], o[5], o[2], o[3])
    # ... and a single inner solve started there stops at its iteration cap instead of spinning
    prob = bz.Problem(bz.Zero(), g_d, bz.IdentityFunction(), D_d, n, n, T, slack=True)
    prob.set_multipliers(np.full(n, 0.1, T), y0)
    z, st = prob.panoc_solve(bz.PANOCplus(tol=1e-8, maxit=50).c_opts(), np.concatenate([x0, x0]))
    assert st.iters == 50 and not np.isfinite(st.gamma)
    prob.close()


@pytest.mark.parametrize("D,g", [("box", "l1"), ("free", "l1box"), ("zero", "nonneg")])
@pytest.mark.parametrize("n,iters,start", [(30_010, 150, "random"), (400_002, 60, "random"), (100_002, 300, "zero")])
def test_slack_iterate_history_form_is_bitwise_neutral(bz, ref, n, iters, start, D, g, monkeypatch):
    """ALS in the iterate-history form (k_fused_slack_xr: the m + 1 last iterates of [x; s] in, their residuals re-evaluated
    in registers, xs_d out — 1.5 GB per iteration at n = 1e7 instead of 2.96) against the stored-pair pass (k_fused_slack)
    on one grid: the same bits in x, z, res and every scalar, through tau backtracks, gamma halvings and skipped pairs
    (where the pairs are re-materialised from the iterates, k_pairs_from_iterates_slack), with z stored or kept in
    registers (auglagfunslack.jl:78-97,136-154)."""
    d, dev, orc = make_cfg2(bz, ref, n, D=D, g=g)
    rng = np.random.default_rng(n % 1000 + 3)
    mu = 10.0 ** rng.uniform(-1.5, -0.5, n)
    y = 0.5 * rng.standard_normal(n)
    xs0 = np.zeros(2 * n) if start == "zero" else np.concatenate([0.3 * rng.standard_normal(n), 0.3 * rng.standard_normal(n)])
    pin = {"BZ_GFC": "2", "BZ_GRID": "512"}
    runs = {}
    for name, env in (("pairs", dict(pin, BZ_XR="0")), ("iterates", dict(pin, BZ_XR="2")), ("iterates-z", dict(pin, BZ_XR="2", BZ_SKIPZ="0")),
                      ("iterates-nt", dict(pin, BZ_XR="2", BZ_NT="1")), ("iterates-generic", dict(pin, BZ_XR="2", BZ_SLACKFAST="0")),
                      # (the fast instantiations with run-time kinds of g and D)
                      ("iterates-rtkinds", dict(pin, BZ_XR="2", BZ_SLACKKIND="0"))):
        for k in ("BZ_XR", "BZ_SKIPZ", "BZ_NT", "BZ_GFC", "BZ_GRID", "BZ_SLACKFAST", "BZ_SLACKKIND"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        prob = bz.Problem(*dev, n, n, np.float64, slack=True)
        prob.set_multipliers(mu, y)
        prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=float(np.finfo(float).eps)).c_opts(), xs0)
        for _ in range(iters):
            prob.panoc_step()
        st = prob.panoc_stats()
        p = prob.profile2()
        runs[name] = (prob.panoc_vector("x"), prob.panoc_vector("z"), prob.panoc_vector("res"), prob.panoc_scalars(),
                      (st.n_backtracks, st.n_gamma_halvings, st.n_lbfgs_skips, st.n_fused_iters, st.n_grad, st.n_prox),
                      p["k_fused_iterates"]["launches"], p["k_fused_iterates"]["form"])
        prob.close()
    base = runs["pairs"]
    assert base[5] == 0
    for name in ("iterates", "iterates-z", "iterates-nt", "iterates-generic", "iterates-rtkinds"):
        r = runs[name]
        assert r[5] >= max(4, iters - 12 - 7 * base[4][2] - 2 * base[4][0] - base[4][1]), (name, r[5], base[4])
        assert r[6].startswith("k_fused_slack_xr<NT=1>" if name == "iterates-nt" else "k_fused_slack_xr<NT=0>"), r[6]
        # (the compile-time instantiations serve f = DiagQuadratic without vector-valued parameters: NormL1Box's u is one)
        assert ("(fast" in r[6]) == (g != "l1box" and name != "iterates-generic"), (name, r[6])
        for a, b in zip(r[:3], base[:3]):
            assert np.array_equal(a, b), name
        for key in ("k", "gamma", "tau", "f_x", "g_z", "dot_grad_res", "ss_res", "stop_norm", "last_ys", "lbfgs_mem", "lbfgs_H", "FBE"):
            assert r[3][key] == base[3][key], (name, key)
        assert r[4][:3] == base[4][:3]


@pytest.mark.parametrize("yzero", [True, False])
def test_slack_uniform_penalties_travel_as_numbers_bitwise(bz, ref, yzero, monkeypatch):
    """alps.jl:42 / als.jl:45 give every constraint the same mu whenever c(x0) is in D, and y0 = 0 holds through the first
    subproblem: the slack passes then take mu (and mu*y = y = 0) as NUMBERS — two or three streams fewer — and the
    quotients by mu through two Markstein steps (div_u).  Same operands, same operations: BZ_UNI=0 (everything streamed,
    hardware division) gives the same bits, in both forms of the history."""
    n = 120_002
    d, dev, orc = make_cfg2(bz, ref, n, D="box", g="l1")
    rng = np.random.default_rng(17)
    mu = np.full(n, 0.1)
    y = np.zeros(n) if yzero else 0.5 * rng.standard_normal(n)
    xs0 = np.concatenate([0.3 * rng.standard_normal(n), 0.3 * rng.standard_normal(n)])
    outs = {}
    for uni in ("0", "2"):
        for xr in ("0", "2"):
            monkeypatch.setenv("BZ_UNI", uni); monkeypatch.setenv("BZ_XR", xr)
            monkeypatch.setenv("BZ_GFC", "2"); monkeypatch.setenv("BZ_GRID", "512")
            prob = bz.Problem(*dev, n, n, np.float64, slack=True)
            prob.set_multipliers(mu, y)
            prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=float(np.finfo(float).eps)).c_opts(), xs0)
            prob.profile_reset()
            prob.profile_enable(True)
            for _ in range(60):
                prob.panoc_step()
            p = prob.profile2()
            cat = "k_fused_iterates" if xr == "2" else "k_fused_sep"
            outs[(uni, xr)] = (prob.panoc_vector("x"), prob.panoc_vector("z"), prob.panoc_scalars(),
                               p[cat]["bytes"] / max(1, p[cat]["launches"]) / (8.0 * n))
            prob.close()
    base = outs[("0", "0")]
    for key, r in outs.items():
        assert np.array_equal(r[0], base[0]) and np.array_equal(r[1], base[1]), key
        for k in ("gamma", "f_x", "g_z", "stop_norm", "last_ys", "lbfgs_H", "FBE"):
            assert r[2][k] == base[2][k], (key, k)
    # streams per launch of the iterate-history pass at m = 5: 12 iterate halves + q, b (+ mu, mu*y, y) + 2 out (+ 2 with z)
    saved = 3 if yzero else 1
    assert outs[("0", "2")][3] - outs[("2", "2")][3] >= saved - 0.5
