"""LeastSquares(A, b) and Quadratic(Q, q) with c = Identity on the device (dense_f_eval: k_gemv_n, k_gemv_t, k_gemv_t_mfma,
gemv_t_fold; k_algrad_elem in its modes 1 and 2) against the oracle.  tests/test_dense_f_host.py holds the table of shapes,
the generators, the extended-precision twins, the forward bound and the proof that every run case keeps the conditions
the comparisons below rest on; this file runs the same cases on the device:
  (1) one AL gradient on exact data, bit for bit, over both f kinds, both types, every shape and every D the path takes,
      with the route (which kernel, how many launches, how many bytes) read from the profile;
  (2) one AL gradient on real data: the suite's 1e-12 / 2e-5 against the oracle, and component by component against the
      twin within twice the a-priori forward bound; two evaluations give the same bits;
  (3) NaN, +inf, -inf and the largest finite number in single entries of x, and +inf in single entries of b: the oracle's
      NaN / inf pattern;
  (4) the start of a solve against the oracle's init();
  (5) thirty states against the oracle in the three forms of the L-BFGS operator, compared over the range of states the
      host file proves settled;
  (6) the wide case on the persistent two-loop kernel;
  (7) Anderson, Broyden and max_backtracks = 2;
  (8) whole solves.
In (5) to (7) both sides start from one step size, as tests/test_gpu_linesearch_table.py does (the device is given the
oracle's Lipschitz estimate as `gamma` with adaptive=True); the device's own estimate is the subject of (4)."""
import warnings

import numpy as np
import pytest

from tests import test_dense_f_host as H
from tests.test_dense_f_host import F32, F64

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]


def one_gradient(bz, dev, n, dt, mu, y, x, times=1):
    prob = bz.Problem(*dev, n, n, dt)
    try:
        prob.set_multipliers(mu, y)
        prob.profile_reset()
        prob.profile_enable(True)
        with np.errstate(all="ignore"):
            runs = [prob.eval_al_gradient(x) for _ in range(times)]
        pr = prob.profile2()
    finally:
        prob.close()
    return runs, pr


# ------------------------------------------------------------------ (1) one AL gradient on exact data, bit for bit
EXACT = H.exact_cases()


@pytest.mark.parametrize("case", EXACT, ids=H.case_id)
def test_exact_gradient_bit_for_bit(bz, ref, case):
    """Integer data, mu = 1/4 (tests/test_dense_f_host.py proves that no summation order can change a bit): gradient, L and
    f equal the oracle's with ==.  The route: k_gemv_n once per product; the transposed product of LeastSquares on the
    matrix cores exactly where fp32 and n % 64 == 0, k_gemv_t elsewhere; none for Quadratic; the bytes of the mv() calls of
    gemv_rows and gemv_cols; one k_algrad_elem launch."""
    kind, shape, dt, D = case
    n = H.n_of(kind, shape)
    dev, orc, mu, y, x = H.gradient_case(bz, ref, kind, shape, dt, D, "exact")
    g_ref, lx, fx = H.assert_exact(ref, kind, dt, orc, mu, y, x)
    [(g_dev, vals)], pr = one_gradient(bz, dev, n, dt, mu, y, x)
    assert g_dev.dtype == np.dtype(dt)
    bad = np.flatnonzero(g_dev != g_ref)
    assert bad.size == 0, (H.case_id(case), bad[:8], g_dev[bad[:8]], g_ref[bad[:8]])
    assert vals[0] == float(lx) and vals[1] == float(fx), (vals, float(lx), float(fx))
    rows = shape[0] if kind == "ls" else n
    mfma = kind == "ls" and H.route(rows, n, dt)["mfma"]
    assert pr["gemv"]["launches"] == (2 if kind == "ls" and not mfma else 1), pr["gemv"]
    assert pr["k_gemv_t_mfma"]["launches"] == (1 if mfma else 0), pr["k_gemv_t_mfma"]
    assert pr["gemv"]["form"] == ("k_gemv_t" if kind == "ls" and not mfma else "k_gemv_n"), pr["gemv"]["form"]
    assert pr["gemv"]["bytes"] + pr["k_gemv_t_mfma"]["bytes"] == H.gemv_bytes(rows, n, dt, kind == "ls", kind == "ls"), \
        (pr["gemv"], pr["k_gemv_t_mfma"])
    assert pr["al_gradient"]["launches"] == 1 and pr["k_fused_iterates"]["launches"] == 0 and pr["fb_step"]["launches"] == 0


# ------------------------------------------------------------------ (2) one AL gradient on real data
REAL = [c + (D,) for c in H.REAL_SHAPES for D in ("box", "vc") if not (D == "vc" and H.n_of(c[0], c[1]) % 2)]


@pytest.mark.parametrize("case", REAL, ids=H.case_id)
def test_real_gradient_against_oracle_and_forward_bound(bz, ref, case):
    """Real data, per-element penalties 10^U(-2, 0).  (a) 1e-12 / 2e-5 of the gradient's largest entry, of max(1, |L|) for
    the values; (b) every component within twice H.forward_bound of the twin's, L and f within twice theirs; the second
    evaluation gives the bits of the first.  Prints the worst error / bound (NEXT.md keeps the worst of the file)."""
    kind, shape, dt, D = case
    n = H.n_of(kind, shape)
    dev, orc, mu, y, x = H.gradient_case(bz, ref, kind, shape, dt, D, "real")
    runs, pr = one_gradient(bz, dev, n, dt, mu, y, x, times=2)
    (g_dev, vals), (g2, vals2) = runs
    g_ref, lx, fx, _ = H.oracle_gradient(ref, orc, mu, y, x)
    g_tw, lt, ft, al_t = H.oracle_gradient(ref, orc, mu, y, x, twin=True)
    bound, EL, Ef = H.forward_bound(kind, dt, orc, mu, y, x, g_tw, al_t)
    tol = 1e-12 if dt == F64 else 2e-5
    scale = float(np.max(np.abs(g_ref)))
    ea = float(np.max(np.abs(g_dev.astype(F64) - g_ref.astype(F64)))) / scale
    ratio = float(np.max(np.abs(g_dev.astype(F64) - g_tw.astype(F64)) / bound))
    rl, rf = abs(vals[0] - float(lt)) / EL, abs(vals[1] - float(ft)) / Ef
    print(f"{H.case_id(case)}: (a) gradient {ea:.3e} L {abs(vals[0] - float(lx)) / max(1.0, abs(float(lx))):.3e} (tol {tol:g}); "
          f"(b) error / bound: gradient {ratio:.3e} L {rl:.3e} f {rf:.3e}")
    assert np.array_equal(g_dev, g2) and vals == vals2
    assert ea <= tol
    assert abs(vals[0] - float(lx)) <= tol * max(1.0, abs(float(lx))) and abs(vals[1] - float(fx)) <= tol * max(1.0, abs(float(lx)))
    assert ratio <= 2.0 and rl <= 2.0 and rf <= 2.0


# ------------------------------------------------------------------ (3) special arguments
def _pattern(v):
    v = np.asarray(v, dtype=F64)
    return np.isnan(v), np.isposinf(v), np.isneginf(v)


def _cls(v):
    return "nan" if np.isnan(v) else ("+inf" if v == np.inf else ("-inf" if v == -np.inf else "finite"))


@pytest.mark.parametrize("case", H.SPECIAL_SHAPES, ids=H.case_id)
def test_special_arguments_give_the_oracles_pattern(bz, ref, case):
    """x_j in {NaN, +inf, -inf, the largest finite number} at column 0, on both sides of the first pack boundary and at the
    last column, one at a time: the NaN / inf pattern of the gradient and the class (finite, +inf, -inf, NaN) of L and f are
    the oracle's.  A sum is NaN iff it holds a NaN or infinities of both signs, whatever its order; for the largest finite
    number the host file proves that no sum of a product overflows."""
    kind, shape, dt = case
    n = H.n_of(kind, shape)
    dev, orc, mu, y, x0 = H.special_case(bz, ref, kind, shape, dt)
    prob = bz.Problem(*dev, n, n, dt)
    try:
        prob.set_multipliers(mu, y)
        for j in H.special_positions(n, dt):
            for v in H.special_values(dt):
                x = x0.copy()
                x[j] = v
                g_dev, vals = prob.eval_al_gradient(x)
                g_ref, lx, fx, _ = H.oracle_gradient(ref, orc, mu, y, x)
                for a, b, what in zip(_pattern(g_dev), _pattern(g_ref), ("nan", "+inf", "-inf")):
                    assert np.array_equal(a, b), (H.case_id(case), j, v, what, int(np.sum(a)), int(np.sum(b)))
                assert _cls(vals[0]) == _cls(float(lx)) and _cls(vals[1]) == _cls(float(fx)), (H.case_id(case), j, v, vals, float(lx), float(fx))
    finally:
        prob.close()


@pytest.mark.parametrize("dt", H.BOTH, ids=H.tname)
def test_overflow_corner_gradient(bz, ref, dt):
    """Quadratic, n = 514, x_0 the largest finite number and q_0 = -2 sign(Q_00) (H.overflow_corner): the gradient's NaN / inf
    pattern is the oracle's.  (L = f + an infinite penalty term follows f: see the next test.)"""
    dev, orc, mu, y, x = H.overflow_corner(bz, ref, dt)
    [(g_dev, vals)], _ = one_gradient(bz, dev, 514, dt, mu, y, x)
    g_ref, lx, fx, _ = H.oracle_gradient(ref, orc, mu, y, x)
    for a, b, what in zip(_pattern(g_dev), _pattern(g_ref), ("nan", "+inf", "-inf")):
        assert np.array_equal(a, b), (what, int(np.sum(a)), int(np.sum(b)))


@pytest.mark.xfail(strict=True, reason="the device sums x (Q x / 2 + q) element by element where ProximalOperators forms <x, Q x> / 2 + <x, q>: "
                   "an infinity where the oracle's f is inf - inf = NaN (NEXT.md, 'Dense f with c = Identity against the oracle: findings')")
@pytest.mark.parametrize("dt", H.BOTH, ids=H.tname)
def test_overflow_corner_value_of_f(bz, ref, dt):
    """the same point: the oracle's f is NaN in the type (proved in the host file; its extended-precision twin, which does not
    overflow at x_0 q_0, gives the device's value); the device's is an infinity of the sign of Q_00, because k_algrad_elem in its mode 2 (and k_fvalue_elem) add x_0 q_0 to x_0 Q_00 x_0 / 2 before either can
    overflow alone.  L = f + (+inf) follows: NaN on the oracle, +inf on the device where Q_00 > 0 (fp32's draw), NaN by
    inf - inf where Q_00 < 0 (fp64's).  `alps` tests isnan(f + g), so a solve through such a point ends "exception" on the
    oracle only.  Open."""
    dev, orc, mu, y, x = H.overflow_corner(bz, ref, dt)
    [(g_dev, vals)], _ = one_gradient(bz, dev, 514, dt, mu, y, x)
    fx = H.oracle_gradient(ref, orc, mu, y, x)[2]
    assert _cls(vals[1]) == _cls(float(fx)), (vals[1], float(fx))


B_SHAPES = [((7, 64), F32), ((5000, 128), F32), ((5000, 128), F64), ((16400, 64), F32), ((257, 1031), F64)]


@pytest.mark.parametrize("case", B_SHAPES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{H.tname(c[1])}")
def test_one_infinite_residual_stays_in_its_row(bz, ref, case):
    """b_i = +inf in one row — row 0, the first row of the second row chunk, the last row — makes r_i = -inf and every other
    residual finite: the gradient is -inf * A[i, :] + finite, an infinity of the sign of -A[i, j] in every column and no NaN,
    f = L = +inf.  A row chunk whose ragged tail multiplies the masked rows' zeros with the residuals behind its end (the
    matrix-core product feeds four rows a step) would turn the neighbour's infinity into NaNs."""
    (m, n), dt = case
    dev, orc, mu, y, x = H.gradient_case(bz, ref, "ls", (m, n), dt, "box", "real")
    rpc = H.plan_chunks(m, n, dt)[0]
    for i in sorted({0, min(rpc, m - 1), m - 1}):
        b = orc[0].b.copy()
        b[i] = np.inf
        [(g_dev, vals)], _ = one_gradient(bz, (bz.LeastSquares(orc[0].A, b),) + tuple(dev[1:]), n, dt, mu, y, x)
        g_ref, lx, fx, _ = H.oracle_gradient(ref, (ref.LeastSquares(orc[0].A, b),) + tuple(orc[1:]), mu, y, x)
        assert not np.any(np.isnan(g_ref)) and np.all(np.isinf(g_ref)) and _cls(float(fx)) == "+inf"
        for u, v, what in zip(_pattern(g_dev), _pattern(g_ref), ("nan", "+inf", "-inf")):
            assert np.array_equal(u, v), (case, i, what, int(np.sum(u)), int(np.sum(v)))
        assert _cls(vals[0]) == _cls(float(lx)) and _cls(vals[1]) == "+inf", (case, i, vals)


# ------------------------------------------------------------------ (4) the start of a solve
@pytest.mark.parametrize("case", H.START_CASES, ids=H.ids(H.START_CASES))
def test_start_of_a_solve_is_the_oracles_init(bz, ref, case):
    """panoc_begin without a step size at x0 != 0 (k_add_scalar, the second gradient, k_diff_ss2 on a matrix f): gamma, f_x and
    stop_norm within 100 x the distance of the oracle's two roundings, floored at 4 eps — of the value for gamma, of
    max(1, |f_x|) for f_x, of the size of its operands for stop_norm (measured before: 8 eps of its own value at 5000 x 128,
    fp64, where the two roundings happened to coincide); n_grad == 3 + halvings and the halvings are the oracle's.  With gamma given there is
    no second gradient: n_grad == 2."""
    p = H.pair_of(bz, ref, case)
    dev, orc, n, ny, mu, y, x0 = case.build(bz, ref)
    eps = float(np.finfo(case.dtype).eps)
    prob = bz.Problem(*dev, n, n, case.dtype)
    try:
        prob.set_multipliers(mu, y)
        prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=eps).c_opts(), x0)
        sc, st = prob.panoc_scalars(), prob.panoc_stats()
        worst = 0.0
        # the scale of a value: gamma its own size ; f_x max(1, |f_x|) ; stop_norm = max |res / gamma - grad(x) + grad(z)| is a
        # difference of gradients: each operand is known to a few eps of ITS size, so the floor is 4 eps of the operands' size
        # (what motivated it: at (5000, 128) in fp64 the two roundings coincide and the device is 8 eps of stop_norm's own
        # value away, 1.4e-14 at 8.04, with operands of some 1e2)
        o = p.o.st
        ops = float(np.max(np.abs(o.res / o.gamma)) + np.max(np.abs(o.grad_f_x)) + np.max(np.abs(o.grad_f_z)))
        for key, vo, vt, scale in (("gamma", float(o.gamma), float(p.t.st.gamma), abs(float(o.gamma))), ("f_x", float(o.f_x), float(p.t.st.f_x), max(1.0, abs(float(o.f_x)))),
                                   ("stop_norm", float(p.o.it.stop_norm(o)), float(p.t.it.stop_norm(p.t.st)), max(1.0, ops))):
            tol = max(100 * abs(vo - vt), 4 * eps * scale)
            worst = max(worst, abs(sc[key] - vo) / scale / eps)
            print(f"{case.name}: {key} device {sc[key]!r} oracle {vo!r} twin {vt!r} tol {tol:.3e}")
            assert abs(sc[key] - vo) <= tol, (case.name, key, sc[key], vo, vt, tol)
        print(f"{case.name}: worst distance {worst:.3f} eps; halvings {st.n_gamma_halvings}, n_grad {st.n_grad}")
        assert st.n_gamma_halvings == p.o.start_halvings == p.t.start_halvings
        assert st.n_grad == 3 + st.n_gamma_halvings
        prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=eps, gamma=float(p.o.st.gamma)).c_opts(), x0)
        assert prob.panoc_stats().n_grad == 2 and prob.panoc_scalars()["gamma"] == float(p.o.st.gamma)
    finally:
        prob.close()


# ------------------------------------------------------------------ (5) thirty states against the oracle
def begin(bz, case, built, gamma, compact, persist=True):
    dev, orc, n, ny, mu, y, x0 = built
    prob = bz.Problem(*dev, n, ny, case.dtype)
    prob.set_multipliers(mu, y)
    dirs = bz.LBFGS(5, compact=compact) if case.direction == "lbfgs" else case.directions(bz)
    prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=float(np.finfo(case.dtype).eps), max_backtracks=case.M,
                                  directions=dirs, persist=persist, gamma=float(gamma), adaptive=True).c_opts(), x0)
    prob.profile_reset()
    prob.profile_enable(True)
    return prob


def follow(bz, ref, case, compact, oracle_compact, persist=True):
    """the device in lockstep with the oracle over the case's compared range: gamma, tau and the counts (tau backtracks,
    gamma halvings, skipped pairs) equal at every state, x and z within max(1e-9 | 5e-5, 100 sens).  Returns the states
    (x, z, gamma) of the whole run, the forms of the x_d launch seen and the profile."""
    p = H.pair_of(bz, ref, case.with_form(oracle_compact))
    built = case.build(bz, ref)
    sup = case.g in H.SUPPORT_G
    states, xd_forms, worst = [], set(), 0.0
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        prob = begin(bz, case, built, p.o.gamma_start, compact, persist)
        try:
            for j in range(case.states):
                x, z, sc, st = prob.panoc_vector("x"), prob.panoc_vector("z"), prob.panoc_scalars(), prob.panoc_stats()
                states.append((x, z, sc["gamma"]))
                if j < p.compared:
                    xo, zo, go = p.o.states[j]
                    label = (case.name, compact, j + 1)
                    assert sc["gamma"] == go, label + (sc["gamma"], go)
                    assert (st.n_backtracks, st.n_gamma_halvings, st.n_lbfgs_skips) == p.counts(j), label + (st.n_backtracks, st.n_gamma_halvings, st.n_lbfgs_skips, p.counts(j))
                    if j:
                        s = p.o.steps[j - 1]
                        assert sc["tau"] == s.tau and sc["n_backtracks"] == s.nbt, label + (sc["tau"], s.tau, sc["n_backtracks"], s.nbt)
                    if sup:          # (a discontinuous prox: the same support but for ties, test_lp_power_prox's rule)
                        assert np.mean((z != 0) == (zo != 0)) >= (0.9999 if x.shape[0] >= 1000 else 1.0), label
                    ex, ez, tol = H.dist(x, xo, sup), H.dist(z, zo, sup), p.tol(j)
                    worst = max(worst, ex / tol, ez / tol)
                    assert ex <= tol and ez <= tol, f"{label}: iterate mismatch {ex} {ez} (tol {tol}, sens {p.sens[j]})"
                if j + 1 < case.states:
                    prob.panoc_step()
                    xd_forms.add(prob.profile2()["x_d"]["form"])
            pr = prob.profile2()
        finally:
            prob.close()
    print(f"{case.name} compact={compact}: {p.compared} states compared, worst error / tolerance {worst:.3e}, sens {p.sens[p.compared - 1]:.3e}, "
          f"counts {p.counts(p.compared - 1)}")
    return states, xd_forms, pr


def assert_form(pr, xd_forms, form):
    """which form of the operator ran, from the profile: the compact form (k_compact_xd, no two-loop kernel), the kernel
    chain (k_axpy_dot) or the persistent kernel"""
    if form == "compact":
        assert pr["k_axpy_dot"]["launches"] == 0 and pr["k_twoloop_persist"]["launches"] == 0, (pr["k_axpy_dot"], pr["k_twoloop_persist"])
        assert any(f.startswith("k_compact_xd<") for f in xd_forms), xd_forms
    elif form == "chain":
        assert pr["k_axpy_dot"]["launches"] >= 1 and pr["k_twoloop_persist"]["launches"] == 0, (pr["k_axpy_dot"], pr["k_twoloop_persist"])
        assert not any(f.startswith("k_compact_xd<") for f in xd_forms), xd_forms
    else:
        assert pr["k_twoloop_persist"]["launches"] >= 1, pr["k_twoloop_persist"]
    assert pr["k_fused_iterates"]["launches"] == 0 and pr["gemv"]["launches"] >= 1


LBFGS_CASES = H.TABLE + H.EVENT_CASES


@pytest.mark.parametrize("case", LBFGS_CASES, ids=H.ids(LBFGS_CASES))
def test_thirty_states_follow_the_oracle_in_every_form(bz, ref, case):
    """LBFGS(5) as it comes (auto), compact=False against the oracle's two-loop operator and compact=True against its compact
    operator.  Auto takes the compact form on this path (n below the persistent kernel's threshold: the two-loop would be
    a chain of kernels), so it is held to the compact run bit for bit and to the same oracle."""
    s_chain, f_chain, pr = follow(bz, ref, case, False, False)
    assert_form(pr, f_chain, "chain")
    s_comp, f_comp, pr = follow(bz, ref, case, True, True)
    assert_form(pr, f_comp, "compact")
    s_auto, f_auto, pr = follow(bz, ref, case, None, True)
    assert_form(pr, f_auto, "compact")
    for j, (a, b) in enumerate(zip(s_auto, s_comp)):
        assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True) and a[2] == b[2], (case.name, j + 1)
    p = H.pair_of(bz, ref, case.with_form(False))
    bt, hv, sk = p.counts(p.compared - 1)
    if "b" in case.claims:
        assert bt >= 2
    if "h" in case.claims:
        assert hv - p.o.start_halvings >= 1


# ------------------------------------------------------------------ (6) the wide case
def test_wide_case_runs_the_persistent_two_loop(bz, ref):
    """(8, 300034), fp64, LBFGS(5, compact=False), 15 states: k_twoloop_persist launches; it agrees with persist=False to 1e-12
    on x and z with equal gamma (the rule of test_persistent_two_loop_matches_kernel_chain) and with the oracle as in (5)"""
    case = H.WIDE_CASE
    s_p, forms, pr = follow(bz, ref, case, False, False, persist=True)
    assert_form(pr, forms, "persist")
    s_c, forms, pr = follow(bz, ref, case, False, False, persist=False)
    assert_form(pr, forms, "chain")
    for j, (a, b) in enumerate(zip(s_p, s_c)):
        assert H.dist(a[0], b[0]) <= 1e-12 and H.dist(a[1], b[1]) <= 1e-12 and a[2] == b[2], (j + 1, H.dist(a[0], b[0]), H.dist(a[1], b[1]))


# ------------------------------------------------------------------ (7) other directions and the line search at its limit
@pytest.mark.parametrize("case", H.OTHER, ids=H.ids(H.OTHER))
def test_other_directions_and_two_backtracks_follow_the_oracle(bz, ref, case):
    """AndersonAcceleration(3) (against the twin of tests/test_directions_host.py), Broyden() and max_backtracks = 2: the counts
    exact, the iterates by the rule of (5)"""
    states, forms, pr = follow(bz, ref, case, case.compact, case.compact)
    assert pr["k_fused_iterates"]["launches"] == 0 and pr["gemv"]["launches"] >= 1
    p = H.pair_of(bz, ref, case)
    if "b" in case.claims:
        assert p.counts(p.compared - 1)[0] >= 2
    if case.M == 2:          # every backtrack of this limit is the tau = 0 one
        assert all(s.tau in (0.0, 1.0) for s in p.o.steps)


# ------------------------------------------------------------------ (8) whole solves
def lasso_reference(dt):
    T = np.dtype(dt).type
    A, b = np.array(H.REFERENCE_A, dt), np.array(H.REFERENCE_B, dt)
    lam = T(0.1) * np.max(np.abs(A.T @ b))
    return A, b, lam, np.array([-3.877278911564627e-01, 0, 0, 2.174149659863943e-02, 6.168435374149660e-01])


FP32_SOLVE = dict(tol=1e-4, maxit=20, subsolver_maxit=1000)      # (sqrt(eps) of fp32 is 3.5e-4: residuals are not resolved far below it)


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host-loop"])
def test_reference_lasso_in_fp32(bz, resident):
    """test_verbose.jl in Float32: x_star to 1e-3"""
    A, b, lam, x_star = lasso_reference(F32)
    out = bz.alps(bz.LeastSquares(A, b), bz.NormL1(float(lam)), bz.IdentityFunction(), bz.FreeSet(), np.zeros(5, F32), np.zeros(5, F32),
                  resident=resident, subsolver=lambda **kw: bz.PANOCplus(maxit=1000, **kw), **FP32_SOLVE)
    err = float(np.max(np.abs(out[0].astype(F64) - x_star)))
    print(f"fp32 lasso resident={resident}: status {out[5]} outer {out[2]} inner {out[3]} max|x - x_star| {err:.3e}")
    assert out[0].dtype == np.float32 and err <= 1e-3


@pytest.mark.parametrize("n", [2, 100])
def test_reference_nonconvex_qp_in_fp32(bz, n):
    """test_nonconvex_qp.jl in Float32 (n = 2: its tiny problem; n = 100: seed 1 of tests/test_gpu_reference_tests.py): the
    fixed-point property ||x - proj(x - gamma (Q x + q))|| / gamma <= 1e-3, evaluated in float64"""
    if n == 2:
        Q, q, Lip = np.diag([-0.5, 1.0]), np.array([0.3, 0.5]), 1.0
    else:
        rng = np.random.default_rng(1)
        U, _ = np.linalg.qr(rng.standard_normal((n, n)))
        ev = 2.0 * rng.random(n) - 1.0
        Q = U @ np.diag(ev) @ U.T
        Q, q, Lip = 0.5 * (Q + Q.T), rng.standard_normal(n), float(np.max(np.abs(ev)))
    Q32, q32 = Q.astype(F32), q.astype(F32)
    gamma = 0.95 / Lip
    for g in (bz.IndBox(-1.0, 1.0), bz.IndFree()):
        for resident in (True, False):
            out = bz.alps(bz.Quadratic(Q32, q32), g, bz.IdentityFunction(), bz.ClosedSet(bz.IndBox(-1.0, 1.0)), np.zeros(n, F32), np.zeros(n, F32),
                          resident=resident, subsolver=lambda **kw: bz.PANOCplus(maxit=1000, **kw), **FP32_SOLVE)
            x = out[0].astype(F64)
            fp = float(np.max(np.abs(x - np.clip(x - gamma * (Q32.astype(F64) @ x + q32), -1.0, 1.0)))) / gamma
            print(f"fp32 qp n={n} g={type(g).__name__} resident={resident}: status {out[5]} outer {out[2]} inner {out[3]} fixed point {fp:.3e}")
            assert out[0].dtype == np.float32 and fp <= 1e-3


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host-loop"])
@pytest.mark.parametrize("which", ["lasso", "qp"])
def test_alps_whole_solves(bz, ref, which, resident):
    """bz.alps on the 257 x 1031 Lasso and on the nonconvex QP of n = 514 against ref.alps: the status and the outer count are
    the oracle's; x within 1e-4 (the bound of the suite's whole solves; the QP may end in another stationary point under another
    rounding, so it is held to the reference's own fixed-point property at 1e-4 as well as to x).  alps returns no objective:
    what carries f(x0) out of the resident loop — the one consumer of fvalue()'s dense arm — is the returned mu, which is
    max(1, d^2 / 2) / max(1, f(x0) + g(x0)) / 10 halved a whole number of times.  So mu / mu_oracle is within the relative
    forward bound of f (twice H.forward_bound's, as in (2)) plus 8 eps for the roundings of the formula."""
    dev, orc, n, x0 = H.solve_case(bz, ref, which)
    o = H.ref_solve(bz, ref, which)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = bz.alps(*dev, x0.copy(), np.zeros(n), resident=resident)
    ex = float(np.max(np.abs(a[0] - o[0])))
    mu_ratio = a[9] / o[9]
    # the forward bound of f at the start (the prox of g at x0 with step eps)
    z = np.empty_like(x0)
    gz = orc[1].prox(z, x0, np.finfo(x0.dtype).eps)
    ones, zeros = np.ones(n), np.zeros(n)
    g_tw, lt, ft, al_t = H.oracle_gradient(ref, orc, ones, zeros, z, twin=True)
    Ef = H.forward_bound("ls" if which == "lasso" else "q", F64, orc, ones, zeros, z, g_tw, al_t)[2]
    objx = float(ft) + float(gz)
    rel = 2 * Ef / objx + 8 * float(np.finfo(F64).eps)
    print(f"{which} resident={resident}: status {a[5]}/{o[5]} outer {a[2]}/{o[2]} inner {a[3]}/{o[3]} max|x - x_ref| {ex:.3e} "
          f"max|mu / mu_ref - 1| {float(np.max(np.abs(mu_ratio - 1))):.3e} (bound {rel:.3e})")
    assert a[5] == o[5] == "first_order" and a[2] == o[2]
    assert objx > 1.0 and float(np.max(np.abs(mu_ratio - 1))) <= rel
    assert ex <= 1e-4
    if which == "qp":
        Q, q = orc[0].Q, orc[0].q
        gamma = 0.95 / float(np.max(np.abs(np.linalg.eigvalsh(Q))))
        assert float(np.max(np.abs(a[0] - np.clip(a[0] - gamma * (Q @ a[0] + q), -1.0, 1.0)))) / gamma <= 1e-4
    assert np.array_equal(x0, H.solve_case(bz, ref, which)[3])          # x0 is never mutated
