"""The Lp-power prox kernels (lp_prox behind k_fbstep<LP=1>, k_fbstep_slack<LP=1>, k_fbstep_lifted<LP=1>) against the
extended-precision twin of tests/test_lp_prox_host.py, over that file's table: the bound on z, the exact support on every
settled entry, the value of g in both types, the oracle's NaN / infinity pattern, the kernel form, the same bits from all
three kernels, u read at the element's own index, alpha = 0 and the refusals.  The bounds and why the device can meet them
are derived and proved in the host file; nothing here is fitted to the device's output.

alpha = 0: the prox is min(x, u) (0 for x <= 0).  The loop's first step z0 - (z0 - x) is x up to the rounding of z0 - x, so
the device is held to the oracle's bits and to min(x, u) within eps max(z0, x).  The tiny-argument corner (x below eps / 4,
a tenth of that for the Box kind, whose start is 0.1) returns NaN on the oracle and the device alike; the right value
there is min(x, u).  It is the reference's behaviour and is recorded in NEXT.md, not changed."""
import ctypes as C

import numpy as np
import pytest

from tests import test_lp_prox_host as H

pytestmark = pytest.mark.gpu

LD = np.longdouble
PLAIN_N = (1, 2, 63, 1030, 1031, 4099)
LIFTED_NX, LIFTED_NY = 120, 41
RATIOS = {}                              # (type, kernel) -> largest |z - z*| / bound seen in this run (printed)


def pack_of(dt):
    return 16 // np.dtype(dt).itemsize


def make_g(bz, kind, p, alpha, u):
    return bz.NormLpPowerNonneg(p, alpha=alpha) if kind == "nonneg" else bz.NormLpPowerBox(p, alpha, u=u)


def make_problem(bz, form, g, n, dt):
    """a problem whose eval_prox runs the kernel of `form` over n elements of g; returns (problem, length of the s half)"""
    rng = np.random.default_rng(n)
    d = bz.synth.l1_quadratic(n, dtype=np.dtype(dt))
    f = bz.DiagQuadratic(d["q"], d["b"])
    if form == "plain":
        return bz.Problem(f, g, bz.IdentityFunction(), bz.FreeSet(), n, n, np.dtype(dt)), 0
    if form == "slack":
        prob, ny = bz.Problem(f, g, bz.IdentityFunction(), bz.FreeSet(), n, n, np.dtype(dt), slack=True), n
    else:
        ny = LIFTED_NY
        A = (rng.standard_normal((ny, n)) / np.sqrt(n)).astype(dt)
        prob = bz.Problem(f, g, bz.DenseAffine(A, rng.standard_normal(ny).astype(dt)), bz.FreeSet(), n, ny, np.dtype(dt), slack=True)
    prob.set_multipliers(np.full(ny, 0.5, dt), np.zeros(ny, dt))
    return prob, ny


FORM_NAME = {"plain": "k_fbstep<LP=1>", "slack": "k_fbstep_slack<LP=1>", "lifted": "k_fbstep_lifted<LP=1>"}


def run_prox(prob, ny, form, x, gamma):
    """eval_prox of x (with an s half of ny numbers that D = Free returns as they are); checks the kernel form"""
    n = x.shape[0]
    s = np.linspace(-1.0, 1.0, ny).astype(x.dtype)
    prob.profile_reset()
    prob.profile_enable(True)
    z, gz = prob.eval_prox(np.concatenate([x, s]), gamma)
    pr = prob.profile2()["fb_step"]
    prob.profile_enable(False)
    assert pr["launches"] == 1 and pr["form"] == FORM_NAME[form], pr
    assert z.dtype == x.dtype and np.array_equal(z[n:], s), "proj_D"
    return z[:n], gz


def vectors(p, alpha, gamma, dt, kind, n):
    """the row's block laid out over n elements: (x, u, twin, tags)"""
    x, u, tags, _ = H.block(p, alpha, gamma, dt, kind)
    idx = H.layout(n)
    tw = tuple(v[idx] for v in H.block_twin(p, alpha, gamma, dt, kind))
    return x[idx].copy(), None if u is None else u[idx].copy(), tw, [tags[i] for i in idx]


def hold_to_twin(z, gz, z_fin, gz_fin, x, u, tw, tags, p, alpha, gamma, dt, case):
    """the assertions of one evaluation: z of the whole vector, and (z_fin, gz_fin) of the same vector with the entries that
    are not held to the twin (NaN, infinities, the largest number) set to 0, for the value of g"""
    held = H.judged(x, dt)
    bad, ratio, uns = H.judge(z, x, tw, dt)
    assert bad.size == 0, (case, [(i, tags[i], x[i], None if u is None else u[i], z[i], tw[0][i], tw[1][i]) for i in bad[:6]])
    assert np.all(z[held] >= 0) and not np.any(np.isnan(z[held])), case
    # the NaN / infinity pattern of the oracle on the special arguments (and the same support where it is finite)
    z_o, _ = H.oracle_prox(x, u, p, alpha, gamma, dt)
    sp = ~held
    assert np.array_equal(np.isnan(z[sp]), np.isnan(z_o[sp])) and np.array_equal(np.isinf(z[sp]), np.isinf(z_o[sp])), \
        (case, x[sp], z[sp], z_o[sp])
    fin = sp & np.isfinite(z_o)
    assert np.array_equal(z[fin] != 0, z_o[fin] != 0) and np.all(z[fin] >= 0), (case, x[fin], z[fin], z_o[fin])
    # the held entries do not depend on their neighbours; the value of g over the device's own z
    assert H.same_bits(z_fin[held], z[held]) and np.all(z_fin[sp] == 0), case
    ex = H.g_exact(z_fin, p, alpha, dt)
    assert abs(LD(gz_fin) - ex) <= H.g_bound(x.shape[0], dt) * ex, (case, gz_fin, ex)
    assert np.isfinite(gz) == bool(np.all(np.isfinite(z))), (case, gz)
    return ratio


def sweep(bz, form, dt, kind, p, sizes):
    worst = 0.0
    for n in sizes:
        for gamma in H.GAMMAS:               # (the Box kind's u brackets z* and the ties of its own gamma: a problem each)
            x, u, tw, tags = vectors(p, 0.8, gamma, dt, kind, n)
            prob, ny = make_problem(bz, form, make_g(bz, kind, p, 0.8, u), n, dt)
            try:
                z, gz = run_prox(prob, ny, form, x, gamma)
                x_fin = np.where(H.judged(x, dt), x, 0).astype(dt)
                z_fin, gz_fin = run_prox(prob, ny, form, x_fin, gamma)
            finally:
                prob.close()
            worst = max(worst, hold_to_twin(z, gz, z_fin, gz_fin, x, u, tw, tags, p, 0.8, gamma, dt, (form, dt, kind, p, n, gamma)))
    key = (dt, form)
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
    print("Lp prox %s %s %s p=%.3g: largest |z - z*| / bound %.3f (so far for this type and kernel: %.3f)"
          % (form, dt, kind, p, worst, RATIOS[key]))
    assert worst <= 1.0


@pytest.mark.parametrize("p", H.P_TABLE, ids=lambda p: "p%.3g" % p)
@pytest.mark.parametrize("kind", H.KINDS)
@pytest.mark.parametrize("dt", H.TYPES)
def test_plain_kernel_over_the_table(bz, dt, kind, p):
    """k_fbstep<LP=1> at n = 1, 2, 63, 1030, 1031, 4099: every gamma of the table."""
    sweep(bz, "plain", dt, kind, p, PLAIN_N)


@pytest.mark.parametrize("p", H.P_TABLE, ids=lambda p: "p%.3g" % p)
@pytest.mark.parametrize("kind", H.KINDS)
@pytest.mark.parametrize("dt", H.TYPES)
def test_slack_kernels_over_the_table(bz, dt, kind, p):
    """k_fbstep_slack<LP=1> at n = one pack and 1000, k_fbstep_lifted<LP=1> at nx = 120 beside ny = 41."""
    sweep(bz, "slack", dt, kind, p, (pack_of(dt), 1000))
    sweep(bz, "lifted", dt, kind, p, (LIFTED_NX,))


@pytest.mark.parametrize("p", H.P_TABLE, ids=lambda p: "p%.3g" % p)
@pytest.mark.parametrize("kind", H.KINDS)
@pytest.mark.parametrize("dt", H.TYPES)
def test_three_kernels_give_the_same_bits(bz, dt, kind, p):
    """The same (x, u, p, alpha gamma) through k_fbstep, k_fbstep_slack and k_fbstep_lifted: they call one function, so z
    is the same to the last bit, NaN positions included; alpha = 0 too."""
    n = LIFTED_NX
    for alpha in H.ALPHAS:
        for gamma in H.gammas_of(alpha):
            x, u, _, _ = vectors(p, alpha, gamma, dt, kind, n)
            zs = []
            for form in ("plain", "slack", "lifted"):
                prob, ny = make_problem(bz, form, make_g(bz, kind, p, alpha, u), n, dt)
                try:
                    zs.append(run_prox(prob, ny, form, x, gamma)[0])
                finally:
                    prob.close()
            assert H.same_bits(zs[0], zs[1]) and H.same_bits(zs[0], zs[2]), (dt, kind, p, alpha, gamma)


@pytest.mark.parametrize("n", (1031, 4099))
@pytest.mark.parametrize("dt", H.TYPES)
def test_box_bound_is_read_at_the_elements_own_index(bz, dt, n):
    """NormLpPowerBox with a u of its own per element and neighbouring elements of opposite outcomes: u = 0 (the result is
    0), u = inf (the result is z*), u between z* / 4 and z* / 2 (the result is u, and differs from every neighbour's).
    Every entry is settled, so a u read one element off changes the result."""
    p, alpha, gamma = 0.5, 0.8, 0.37
    T = np.dtype(dt).type
    pl, a = H.held(p, alpha, gamma, dt)
    z_t, x_t, _, _ = H.threshold(pl, a)
    i = np.arange(n)
    x = (x_t * (3 + i.astype(LD) / n)).astype(dt)
    zs = H.stationary(x.astype(LD), pl, a)
    u = np.where(i % 3 == 0, 0, np.where(i % 3 == 1, np.inf, zs * (LD(0.25) + LD(0.25) * ((i * 7) % 11) / 11))).astype(dt)
    tw = H.twin(x, u, pl, a)
    assert not np.any(H.unsettled(x, tw[2], dt))
    assert np.all(tw[0][i % 3 == 0] == 0) and np.all(tw[0][i % 3 == 1] == zs[i % 3 == 1]) and \
        np.array_equal(tw[0][i % 3 == 2], u[i % 3 == 2].astype(LD))
    prob, ny = make_problem(bz, "plain", make_g(bz, "box", p, alpha, u), n, dt)
    try:
        z, gz = run_prox(prob, ny, "plain", x, gamma)
    finally:
        prob.close()
    bad, ratio, _ = H.judge(z, x, tw, dt)
    assert bad.size == 0, (dt, n, [(j, x[j], u[j], z[j], tw[0][j]) for j in bad[:6]])
    assert np.array_equal(z[i % 3 == 2], u[i % 3 == 2])          # (u itself comes back, not a number near it)
    ex = H.g_exact(z, p, alpha, dt)
    assert abs(LD(gz) - ex) <= H.g_bound(n, dt) * ex, (gz, ex)


@pytest.mark.parametrize("kind", H.KINDS)
@pytest.mark.parametrize("dt", H.TYPES)
def test_alpha_zero_is_the_clamp(bz, dt, kind):
    """alpha = 0 (module docstring): the oracle's bits on every entry, the tiny-argument corner's NaN included; min(x, u)
    within eps max(z0, x) wherever x >= 1e-3, 0 wherever x <= 0."""
    eps = float(np.finfo(dt).eps)
    z0 = 1.0 if kind == "nonneg" else 0.1
    for p in H.P_TABLE:
        for form, n in (("plain", 1031), ("slack", 1000), ("lifted", LIFTED_NX)):
            x, u, tw, tags = vectors(p, 0.0, 0.37, dt, kind, n)
            prob, ny = make_problem(bz, form, make_g(bz, kind, p, 0.0, u), n, dt)
            try:
                z, gz = run_prox(prob, ny, form, x, 0.37)
            finally:
                prob.close()
            z_o, _ = H.oracle_prox(x, u, p, 0.0, 0.37, dt)
            bad = np.flatnonzero(~((z == z_o) | (np.isnan(z) & np.isnan(z_o))))
            assert bad.size == 0, (dt, kind, p, form, [(tags[j], x[j], None if u is None else u[j], z[j], z_o[j]) for j in bad[:6]])
            xl = x.astype(np.float64)
            ub = np.full(n, np.inf) if u is None else np.where(np.isnan(u), np.inf, u).astype(np.float64)
            big = H.judged(x, dt) & (xl >= 1e-3) & ((ub == 0) | (ub >= eps * xl))
            assert np.sum(big) >= n // 8
            assert np.all(np.abs(z[big] - np.minimum(xl, ub)[big]) <= eps * np.maximum(z0, xl[big])), (dt, kind, p, form)
            assert np.all(z[np.isfinite(xl) & (xl <= 0)] == 0)
            assert gz == 0 or np.isnan(gz)


def test_refusals(bz):
    """p <= 0, p >= 1, alpha < 0 and a missing u are refused at creation, by the classes and by the library; lambda of
    the Lp kinds cannot be changed between solves."""
    L, lower = bz._lib, bz.oracles.lower
    n = 8
    u = np.ones(n)
    for make in (lambda **k: bz.NormLpPowerNonneg(k["p"], alpha=k["alpha"]), lambda **k: bz.NormLpPowerBox(k["p"], k["alpha"], u=u)):
        for p, alpha, msg in ((0.0, 1.0, "p must be positive"), (-0.5, 1.0, "p must be positive"), (1.0, 1.0, "p must be smaller than one"),
                              (1.5, 1.0, "p must be smaller than one"), (0.5, -1e-3, "alpha must be nonnegative")):
            with pytest.raises(ValueError, match=msg):
                make(p=p, alpha=alpha)
            g = make(p=0.5, alpha=1.0)
            g.p, g.alpha = p, alpha                      # (past the class: the library's own check)
            with pytest.raises(bz.BazingaHipError, match=msg) as e:
                bz.Problem(bz.Zero(), g, bz.IdentityFunction(), bz.FreeSet(), n, n, np.float64)
            assert e.value.code == L.BZ_ERR_ARG
    with pytest.raises(TypeError, match="u"):
        bz.NormLpPowerBox(0.5, 1.0)
    with pytest.raises(ValueError, match="nonnegative entries"):
        bz.NormLpPowerBox(0.5, 1.0, u=-u)
    desc, keep = lower(bz.Zero(), bz.NormLpPowerBox(0.5, 1.0, u=u), bz.IdentityFunction(), bz.FreeSet(), n, n, np.dtype(np.float64), False)
    desc.g_u = None
    h = C.c_void_p()
    with pytest.raises(bz.BazingaHipError, match="need u") as e:
        L.check(L.load().bz_problem_create(bz.default_context()._h, C.byref(desc), C.byref(h)))
    assert e.value.code == L.BZ_ERR_ARG and not h.value
    for g in (bz.NormLpPowerNonneg(0.5, alpha=0.8), bz.NormLpPowerBox(0.5, 0.8, u=u)):
        prob = bz.Problem(bz.Zero(), g, bz.IdentityFunction(), bz.FreeSet(), n, n, np.float64)
        try:
            with pytest.raises(bz.BazingaHipError, match="g must be NormL1, NormL1Nonneg, NormL1Box or NormL0Box") as e:
                prob.set_g_lambda(0.5)
            assert e.value.code == L.BZ_ERR_ARG
            x = np.linspace(-1, 3, n)
            assert np.all(np.isfinite(prob.eval_prox(x, 0.37)[0]))          # (the refused call left the problem usable)
        finally:
            prob.close()


@pytest.mark.parametrize("dt", H.TYPES)
@pytest.mark.parametrize("kind", H.KINDS)
@pytest.mark.parametrize("p", H.TRAJ_P)
def test_short_trajectories_follow_the_oracle(bz, ref, p, kind, dt):
    """20 PANOCplus states of the cfg-2 family with an Lp g at n = 1031, on the kernel chain (the Lp kinds have no one-pass
    form), against the oracle up to the first state in which an entry of a prox argument is unsettled (the host file proves
    at least 10 such states per run).  Tolerance: 1e-10 relative in fp64, the fp32 floor of the family tables in fp32,
    each widened only by 100 x the oracle's own sensitivity to the rounding of its sums."""
    from tests.test_gpu_parity import _err, iter_tol
    states, compared, _ = H.oracle_trajectory(p, kind, dt)
    assert compared >= 10
    dev, mu, y, x0, _ = H.trajectory_problem(bz, p, kind, dt)
    prob = bz.Problem(*dev, H.TRAJ_N, H.TRAJ_N, np.dtype(dt))
    try:
        prob.set_multipliers(mu, y)
        prob.panoc_begin(bz.PANOCplus(tol=0.0, maxit=10 ** 9, minimum_gamma=1e-7, directions=bz.LBFGS(5)).c_opts(), x0)
        worst = 0.0
        for k in range(compared):
            x_o, z_o, gamma_o, sens = states[k]
            sc = prob.panoc_scalars()
            tol = iter_tol(sens) if dt == "float64" else max(2e-5, 100 * sens)
            ex, ez = _err(prob.panoc_vector("x"), x_o), _err(prob.panoc_vector("z"), z_o)
            worst = max(worst, ex / tol, ez / tol)
            assert sc["fused"] == 0.0
            assert abs(sc["gamma"] - gamma_o) <= (1e-12 if dt == "float64" else 1e-5) * gamma_o, (k, sc["gamma"], gamma_o)
            assert ex <= tol and ez <= tol, (p, kind, dt, k, ex, ez, tol)
            assert np.array_equal(prob.panoc_vector("z") != 0, z_o != 0), (p, kind, dt, k)
            if k + 1 < compared:
                prob.panoc_step()
        print("trajectory p=%.1f %s %s: %d states, largest error / tolerance %.3g" % (p, kind, dt, compared, worst))
    finally:
        prob.close()
